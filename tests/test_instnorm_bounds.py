"""CPU: the float64 reference of tests/instnorm_ref.py is InstanceNorm2d, its shape table is the one the sweep was specified with,
and the elementwise bound is tight enough to matter: on the sweep's own inputs (fp32 storage, where the bound is tightest) each
plausible bug - evaluated in float64, the single-pass variance in emulated fp32 - leaves the bound of the correct result somewhere."""

import pytest
import torch
import torch.nn.functional as F
import instnorm_ref as ir
from instnorm_ref import instnorm_ref, make_inputs, out_bound

NONE, RELU = 0, 1


def violates(y_bug, x, gamma, beta, C, Cn, act=NONE, dtype="fp32"):
    ref, err = instnorm_ref(x, gamma, beta, C, Cn, act)
    return bool(((y_bug - ref).abs() > out_bound(ref, err, dtype)).any())


def stats(xn):
    m = xn.mean(dim=1, keepdim=True)
    return m, ((xn - m) ** 2).mean(dim=1, keepdim=True)


def case(shape):
    x, gamma, beta = make_inputs(shape, torch.float32)
    return x, gamma, beta, shape[3], shape[4]


def test_shape_table_is_the_specified_one():
    assert ir.SHAPES == [(2, 1, 1, 8, 8, 8), (3, 7, 9, 64, 32, 64), (2, 5, 5, 24, 8, 24), (2, 33, 31, 40, 40, 40), (1, 56, 56, 16, 16, 16),
                         (2, 12, 12, 512, 256, 512), (2, 6, 6, 32, 16, 48), (4, 14, 14, 256, 128, 256), (2, 9, 7, 64, 0, 64)]
    assert ir.ALL_ACTS_SHAPE in ir.SHAPES and ir.EPS == 1e-5
    hw = {s[1] * s[2] for s in ir.SHAPES}
    assert {1, 63, 1023} <= hw                                   # HW == 1, the unbiased-variance case, the partial last strip
    assert any(s[5] != s[3] for s in ir.SHAPES) and any(s[4] == 0 for s in ir.SHAPES) and any(s[4] == s[3] for s in ir.SHAPES)


@pytest.mark.parametrize("shape", [s for s in ir.SHAPES if s[4] > 0])
def test_reference_is_instance_norm(shape):
    x, gamma, beta, C, Cn = case(shape)
    N, H, W = shape[:3]
    ref, err = instnorm_ref(x, gamma, beta, C, Cn, NONE)
    nchw = x.double()[:, :, :Cn].transpose(1, 2).reshape(N, Cn, H, W)
    if H * W > 1:                # (torch refuses a single spatial element)
        want = F.instance_norm(nchw, weight=gamma.double(), bias=beta.double(), eps=1e-5).reshape(N, Cn, H * W).transpose(1, 2)
        assert float((ref[:, :, :Cn] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    else:
        assert torch.equal(ref[:, :, :Cn], beta.double()[None, None, :].expand(N, 1, Cn))       # var == 0: exactly beta
    assert torch.equal(ref[:, :, Cn:], x.double()[:, :, Cn:C])
    assert bool((err[:, :, Cn:] == 0).all()) and bool((err[:, :, :Cn] > 0).all()) and bool(torch.isfinite(err).all())
    relu, _ = instnorm_ref(x, gamma, beta, C, Cn, RELU)
    assert torch.equal(relu, ref.clamp(min=0))


def test_plan_restates_the_kernel():
    assert ir.plan(3136, 32) == [(25, 7)] * 4                    # 4 chunks: 128 rows in flight, 3136 / 128 -> 25 per thread
    assert ir.plan(3136, 256) == [(49, 6)] * 32                  # groups of 8 chunks: 64 rows
    assert ir.plan(1023, 40) == [(11, 7)] * 5                    # 102 rows
    assert ir.plan(1, 8) == [(1, 0)] and ir.plan(63, 32) == [(1, 6)] * 4
    assert ir.plan(144, 72)[-1] == (1, 8) and len(ir.plan(144, 72)) == 9       # a tail group of one chunk: 512 rows


def test_unbiased_variance_violates():
    x, gamma, beta, C, Cn = case((3, 7, 9, 64, 32, 64))
    m, v = stats(x.double()[:, :, :Cn])
    y, _ = instnorm_ref(x, gamma, beta, C, Cn, NONE, stats=(m, v * 63.0 / 62.0))
    assert violates(y, x, gamma, beta, C, Cn)


def test_missing_eps_violates_on_the_tiny_channel():
    x, gamma, beta, C, Cn = case((3, 7, 9, 64, 32, 64))
    assert abs(float(x[:, :, 3].double().std()) - ir.TINY_STD) < 1e-3
    y, _ = instnorm_ref(x, gamma, beta, C, Cn, NONE, eps=1e-30)
    ref, err = instnorm_ref(x, gamma, beta, C, Cn, NONE)
    bad = (y - ref).abs() > out_bound(ref, err, "fp32")
    assert bool(bad[:, :, 3].any())


def test_batch_pooled_statistics_violate():
    x, gamma, beta, C, Cn = case((4, 14, 14, 256, 128, 256))
    xn = x.double()[:, :, :Cn]
    m = xn.mean(dim=(0, 1), keepdim=True).expand(4, 1, Cn)
    v = ((xn - m) ** 2).mean(dim=(0, 1), keepdim=True).expand(4, 1, Cn)
    y, _ = instnorm_ref(x, gamma, beta, C, Cn, NONE, stats=(m, v))
    assert violates(y, x, gamma, beta, C, Cn)


@pytest.mark.parametrize("moved", [-8, 8])
def test_boundary_moved_by_one_chunk_violates(moved):
    x, gamma, beta, C, Cn = case((3, 7, 9, 64, 32, 64))
    Cb = Cn + moved
    g = torch.cat([gamma, torch.ones(8)])[:Cb]
    b = torch.cat([beta, torch.zeros(8)])[:Cb]
    y, _ = instnorm_ref(x, g, b, C, Cb, NONE)
    assert violates(y, x, gamma, beta, C, Cn)


def test_passthrough_half_normalised_violates():
    x, gamma, beta, C, Cn = case((4, 14, 14, 256, 128, 256))
    y, _ = instnorm_ref(x, torch.cat([gamma, gamma]), torch.cat([beta, beta]), C, C, NONE)
    assert violates(y, x, gamma, beta, C, Cn)


@pytest.mark.parametrize("how", ["c + Cn", "c % 8"])
def test_misindexed_gamma_beta_violate(how):
    """`c + Cn`: the coefficients taken from a C-long vector whose second section is the folded BatchNorm's place (1, 0 here);
    `c % 8`: every chunk reads the first chunk's."""
    x, gamma, beta, C, Cn = case((2, 12, 12, 512, 256, 512))
    if how == "c + Cn":
        g, b = torch.ones(Cn), torch.zeros(Cn)
    else:
        g, b = gamma[:8].repeat(Cn // 8), beta[:8].repeat(Cn // 8)
    y, _ = instnorm_ref(x, g, b, C, Cn, NONE)
    assert violates(y, x, gamma, beta, C, Cn)


def test_missing_last_partial_strip_violates():
    shape = (2, 33, 31, 40, 40, 40)
    x, gamma, beta, C, Cn = case(shape)
    rows = ir.THREADS // (Cn // 8)
    full = (1023 // rows) * rows
    assert 0 < full < 1023
    y, _ = instnorm_ref(x, gamma, beta, C, Cn, NONE, stats=stats(x.double()[:, :full, :Cn]))
    assert violates(y, x, gamma, beta, C, Cn)


def test_cpitch_taken_as_c_violates():
    shape = (2, 6, 6, 32, 16, 48)
    x, gamma, beta, C, Cn = case(shape)
    N, HW, xp = x.shape
    wrong = x.reshape(N, -1)[:, :HW * C].reshape(N, HW, C)          # rows read with a pitch of C
    y, _ = instnorm_ref(wrong, gamma, beta, C, Cn, NONE)
    assert violates(y, x, gamma, beta, C, Cn)


def test_single_pass_fp32_variance_violates_on_the_offset_case_and_two_pass_does_not():
    """A condition on the algorithm, not a measurement: at mean 1024 and deviation 1 in fp32, E[x^2] - mean^2 cancels six of
    fp32's seven digits; the bound of the permitted forms rejects it with room (a factor of 4 is asked here) while a two-pass
    fp32 evaluation stays inside."""
    x, gamma, beta = ir.offset_inputs()
    N, H, W, C, Cn, xp = ir.OFFSET_SHAPE
    ref, err = instnorm_ref(x, gamma, beta, C, Cn, NONE)
    bound = out_bound(ref, err, "fp32")
    y1, _ = instnorm_ref(x, gamma, beta, C, Cn, NONE, stats=ir.fp32_single_pass_stats(x, Cn))
    y2, _ = instnorm_ref(x, gamma, beta, C, Cn, NONE, stats=ir.fp32_two_pass_stats(x, Cn))
    ratio1 = float(((y1 - ref).abs() / bound).max())
    ratio2 = float(((y2 - ref).abs() / bound).max())
    print("offset case: single-pass error / bound = {:.1f}, two-pass error / bound = {:.3f}, bound / |y| max = {:.2e}".format(
        ratio1, ratio2, float((bound / ref.abs().clamp(min=1.0)).max())))
    assert ratio1 > 4.0
    assert ratio2 <= 1.0
    m2, _ = ir.fp32_two_pass_stats(x, Cn)
    m = x.double()[:, :, :Cn].mean(dim=1, keepdim=True)
    assert float((m2 - m).abs().max()) < 2e-3                   # the two-pass mean: about 1e-3 of the deviation (1)
