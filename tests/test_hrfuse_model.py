"""CPU: the model the HRNet fuse kernel is checked against (tests/hrfuse_ref.py) is the specified function, and the sweep of
tests/test_gpu_hrfuse.py has the power to catch the mistakes listed there. The model equals a float64 sum rounded once wherever fp32
summation is exact (small integers); every bug model differs from the correct one on every sweep shape it applies to, in every
storage type and activation it applies to, and applies to at least three shapes."""

import pytest
import torch
import hrfuse_ref as R

DTYPES = ["fp32", "bf16", "fp16"]
ACTS = [R.NONE, R.RELU]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(len(R.SWEEP)), ids=[R.sweep_id(c) for c in R.SWEEP])
def test_model_equals_float64_sum_rounded_once_on_exact_data(index, dtype):
    case = R.SWEEP[index]
    N, C, H, W, shifts = case
    sources = R.make_sources(case, dtype, seed=index, small_ints=True)
    for act in ACTS:
        y = R.model(sources, shifts, H, W, act)
        assert y.dtype == R.TORCH_DTYPES[dtype] and tuple(y.shape) == (N, H, W, C)
        assert torch.equal(y, R.model_f64(sources, shifts, H, W, act))
        if act == R.RELU:
            assert float(y.float().min()) == 0.0
    # nearest upsampling is what torch does with the same tensors
    up = sum(torch.nn.functional.interpolate(s.float().permute(0, 3, 1, 2), size=(H, W), mode="nearest") for s in sources)
    assert torch.equal(R.model(sources, shifts, H, W, R.NONE).float(), up.permute(0, 2, 3, 1))


def test_sweep_is_the_listed_one():
    assert [tuple(c[:4]) + (tuple(c[4]),) for c in R.SWEEP] == [
        (2, 8, 8, 16, (0, 1, 2, 3)), (2, 24, 4, 6, (0, 1)), (3, 40, 8, 8, (0, 0, 0, 0)), (2, 144, 14, 14, (0, 0, 0, 1)),
        (2, 16, 56, 56, (0, 1, 2, 3)), (2, 8, 8, 8, (3,)), (2, 72, 2, 2, (0, 1)), (1, 32, 16, 24, (1, 0))]
    assert sorted(R.BUGS) == sorted(["shift_h_only", "row_pitch_fine", "image_stride_fine", "round_half", "act_per_term",
                                     "partial_rounding", "drop_last_of_four", "reverse_order"])


@pytest.mark.parametrize("bug", sorted(R.BUGS))
def test_every_bug_model_differs_wherever_it_applies(bug):
    fn, applies = R.BUGS[bug]
    shapes = set()
    for index, case in enumerate(R.SWEEP):
        N, C, H, W, shifts = case
        for dtype in DTYPES:
            for act in ACTS:
                if not applies(case, dtype, act):
                    continue
                sources, want = R.sweep_reference(index, dtype, act)
                got = fn(sources, shifts, H, W, act)
                assert got.shape == want.shape and got.dtype == want.dtype
                assert not torch.equal(got, want), "{} goes unnoticed on {} {} act {}".format(bug, R.sweep_id(case), dtype, act)
                shapes.add(index)
    assert len(shapes) >= 3, "{} applies to {} sweep shapes only".format(bug, len(shapes))


def test_reverse_order_shows_in_fp32_on_the_sweep_data():
    """the one bug that 16-bit inputs can hide (their fp32 sums are mostly exact): it must show in fp32"""
    fn, _ = R.BUGS["reverse_order"]
    hits = 0
    for index, case in enumerate(R.SWEEP):
        if len(case[4]) > 2:
            sources, want = R.sweep_reference(index, "fp32", R.NONE)
            hits += int(not torch.equal(fn(sources, case[4], case[2], case[3], R.NONE), want))
    assert hits >= 3
