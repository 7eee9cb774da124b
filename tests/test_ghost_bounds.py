"""CPU: the float64 reference and derived bound of the ghost-module launch (tests/ghost_ref.py) hold for a correct fp32 restatement of
the launch on every sweep shape of tests/test_gpu_ghost.py, in every storage type, with and without the skip tensor - and each of six
plausible mistakes (cheap half written at offset round8(Cm); a pad channel of m copied into y; the skip tensor added to one half
only; the activation applied to the main half; taps read at pitch Cm; left / right taps swapped at the image border) violates the
bound or the exact-copy check on every sweep shape where it changes anything. A bound that let one of them through would not be
worth sweeping the GPU kernel against."""

import pytest
import torch
import ghost_ref as gr
from ghost_ref import NONE, RELU, CLAMP01

DTYPES = ["fp32", "bf16", "fp16"]


def _case(shape, dtype, act, with_res, seed):
    N, Cm, H, W = shape
    m, w, bn, res = gr.ghost_operands(N, Cm, H, W, dtype, seed, with_res)
    gamma, beta, mean, var = bn
    s = gamma / torch.sqrt(var + 1e-5)
    scale, shift = gr.padded(s), gr.padded(beta - mean * s)
    taps = gr.padded_taps(w, dtype)
    ref, err = gr.ghost_ref(m, taps, scale, shift, Cm, act, res)
    return m, taps, scale, shift, res, ref, gr.ghost_bound(ref, err, dtype, Cm, with_res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", gr.SWEEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_correct_model_is_within_the_bound(shape, dtype):
    Cm = shape[1]
    for i, (act, with_res) in enumerate(((NONE, False), (RELU, True), (RELU, False), (NONE, True), (CLAMP01, True))):
        m, taps, scale, shift, res, ref, bound = _case(shape, dtype, act, with_res, seed=100 + i)
        y = gr.ghost_model(m, taps, scale, shift, Cm, act, res, dtype)
        assert gr.violations(y, ref, bound) == 0, (shape, dtype, act, with_res)
        assert not bool(torch.isnan(y).any())
        if not with_res:
            assert torch.equal(y[..., :Cm], m[..., :Cm])
            assert float(bound[..., :Cm].max()) == 0.0
        assert float(ref.abs().max()) < gr.SENTINEL / 100          # no pad channel reached the reference


def test_bound_is_not_vacuous():
    """the cheap half's bound is a small multiple of the storage rounding: far below the data's spread"""
    for dtype, cap in (("fp32", 1e-5), ("bf16", 6e-2), ("fp16", 8e-3)):
        *_, ref, bound = _case((2, 100, 14, 14), dtype, RELU, True, seed=5)
        assert float(bound.max()) <= cap * max(1.0, float(ref.abs().max()) / 4), dtype
        assert float(ref.std()) > 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bug", gr.BUGS)
def test_bug_model_violates_the_bound(bug, dtype):
    caught = 0
    for i, shape in enumerate(gr.SWEEP_SHAPES):
        N, Cm, H, W = shape
        for act, with_res in ((RELU, True), (RELU, False)):
            if not gr.bug_applies(bug, Cm, W, act, with_res):
                continue
            m, taps, scale, shift, res, ref, bound = _case(shape, dtype, act, with_res, seed=300 + i)
            y = gr.ghost_model(m, taps, scale, shift, Cm, act, res, dtype, bug=bug)
            bad = gr.violations(y, ref, bound)
            assert bad > 0, "{} passes the bound on {} {} res={}".format(bug, shape, dtype, with_res)
            caught += 1
    assert caught >= 3, bug


def test_every_bug_applies_to_some_sweep_shape_and_pitch_bugs_need_an_odd_half_width():
    for bug in gr.BUGS:
        assert any(gr.bug_applies(bug, Cm, W, RELU, True) for _, Cm, _, W in gr.SWEEP_SHAPES)
    assert sorted(Cm for _, Cm, _, _ in gr.SWEEP_SHAPES if Cm % 8) == [12, 20, 36, 60, 92, 100]
    assert not gr.bug_applies("taps_at_pitch_cm", 240, 9, RELU, True)
