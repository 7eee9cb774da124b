"""
GPU sweep of pcv_instnorm_act (csrc/instnorm.hpp: instnorm_stats_kernel + instnorm_apply_kernel) against the float64 reference
and the derived elementwise bound of tests/instnorm_ref.py (tests/test_instnorm_bounds.py shows on the CPU that the bound
rejects the plausible bugs), and the kernel's properties: a capped grid and a repeated run give the same bits, an image's
result does not depend on its place in the batch, constant planes come out as act(beta), a NaN stays inside its plane, the
offset case (mean 1024, deviation 1, fp32) is inside the bound, every refusal of the entry point leaves the output untouched,
and an fp16 result beyond the format's range moves the guard counter.
"""

import ctypes
import pytest
import torch
import util
import instnorm_ref as ir
from instnorm_ref import instnorm_ref, make_inputs, out_bound
from test_gpu_dw_se import TDT, CODE, _check

pytestmark = pytest.mark.gpu

NONE, RELU = 0, 1
INVALID, TOO_LARGE = -1, -4


def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def workspace(N, Cn, dev):
    lb, L, ctx = _lib()
    n = ctypes.c_size_t(0)
    assert L.pcv_instnorm_workspace_bytes(N, Cn, ctypes.byref(n)) == 0
    assert n.value == N * Cn * 8
    return torch.full((max(n.value, 16),), 0xFF, dtype=torch.uint8, device=dev)


def launch(x, gamma, beta, C, Cn, act, dtype, eps=ir.EPS, rc_only=False, y=None, ws=None, over=None):
    """pcv_instnorm_act through ctypes into a NaN-filled output: an element no thread writes stays NaN"""
    lb, L, ctx = _lib()
    N, HW, xp = x.shape
    if y is None:
        y = torch.full((N, HW, C), float("nan"), dtype=TDT[dtype], device=x.device)
    if ws is None:
        ws = workspace(N, Cn, x.device)
    a = dict(x=_p(x), gamma=_p(gamma), beta=_p(beta), y=_p(y), ws=_p(ws), N=N, HW=HW, C=C, Cn=Cn, xp=xp, eps=eps, act=act,
             dtype=CODE[dtype])
    a.update(over or {})         # raw argument overrides (the refusal cases): x / gamma / beta / y / ws are passed as given
    rc = L.pcv_instnorm_act(ctx, a["x"], a["gamma"], a["beta"], a["y"], a["ws"], a["N"], a["HW"], a["C"], a["Cn"], a["xp"],
                            ctypes.c_float(a["eps"]), a["act"], a["dtype"], _stream())
    if rc_only:
        return rc, (L.pcv_last_error(ctx) or b"").decode(), y
    lb.check(rc, ctx)
    return y


def on(dev, *ts):
    return [t.to(dev) for t in ts]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", ir.SHAPES, ids=["x".join(str(v) for v in s) for s in ir.SHAPES])
def test_sweep_vs_float64(shape, dtype, cuda_device):
    """every shape x dtype x {NONE, RELU} (all seven codes on one shape): defaults and max_blocks=8 (grid-stride rounds in both kernels)"""
    from pytorchcv_amd import engine
    dev = cuda_device
    quiet = engine.fp16_overflow_count(dev)
    N, H, W, C, Cn, xp = shape
    x, gamma, beta = make_inputs(shape, TDT[dtype])
    xd, gd, bd = on(dev, x, gamma, beta)
    for act in (range(7) if shape == ir.ALL_ACTS_SHAPE else (NONE, RELU)):
        y = launch(xd, gd, bd, C, Cn, act, dtype)
        with util.tuning(max_blocks=8):
            y8 = launch(xd, gd, bd, C, Cn, act, dtype)
        torch.cuda.synchronize()
        ref, err = instnorm_ref(x, gamma, beta, C, Cn, act)
        _check(y.cpu(), ref, out_bound(ref, err, dtype), "instnorm {} {} act{}".format(shape, dtype, act))
        assert torch.equal(y, y8), (shape, dtype, act)
    assert engine.fp16_overflow_count(dev) == quiet


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_constant_plane_and_nan_containment(dtype, cuda_device):
    """channel 5 of image 1 is constant: var == 0 exactly, y = act(beta) within the bound of the folded form and finite; channel 9
    of image 0 holds one NaN: that plane is NaN, nothing else is (the passthrough NaN at channel 40 stays one element)."""
    dev = cuda_device
    shape = (3, 7, 9, 64, 32, 64)
    N, H, W, C, Cn, xp = shape
    x, gamma, beta = make_inputs(shape, TDT[dtype], seed=1)
    x[1, :, 5] = 2.75
    x[0, 17, 9] = float("nan")
    x[2, 3, 40] = float("nan")
    y = launch(*on(dev, x, gamma, beta), C, Cn, NONE, dtype).cpu()
    nan = torch.isnan(y)
    want = torch.zeros_like(nan)
    want[0, :, 9] = True
    want[2, 3, 40] = True
    assert torch.equal(nan, want)
    xc = torch.nan_to_num(x.float(), nan=0.0).to(TDT[dtype])
    ref, err = instnorm_ref(xc, gamma, beta, C, Cn, NONE)
    ok = ~want
    assert bool(((y.double() - ref).abs() <= out_bound(ref, err, dtype))[ok].all())
    plane = y[1, :, 5].double()
    assert bool(torch.isfinite(plane).all()) and bool((plane == plane[0]).all())
    rstd = 1.0 / (ir.EPS ** 0.5)
    slack = 4 * ir.U32 * (2.75 * float(gamma[5]) * rstd) + abs(float(beta[5])) * (ir.ULP[dtype] + ir.U32) + ir.FLOOR[dtype]
    assert abs(float(plane[0]) - float(beta[5])) <= slack       # the m a parts of x a and b cancel to a few u of |m a|
    # HW == 1: every plane is constant
    x1, g1, b1 = make_inputs((2, 1, 1, 8, 8, 8), TDT[dtype], seed=2)
    y1 = launch(*on(dev, x1, g1, b1), 8, 8, RELU, dtype).cpu()
    assert bool(torch.isfinite(y1).all())
    want1 = b1.clamp(min=0).double()[None, None, :].expand(2, 1, 8)
    assert bool(((y1.double() - want1).abs() <= 4 * ir.U32 * (x1.double().abs() * g1.double() * rstd) + want1 * ir.ULP[dtype]
                 + ir.U32 + ir.FLOOR[dtype]).all())


def test_offset_case_fp32(cuda_device):
    """mean 1024, deviation 1, fp32: inside the bound that the single-pass variance misses by a factor of 40 on the CPU"""
    dev = cuda_device
    x, gamma, beta = ir.offset_inputs()
    N, H, W, C, Cn, xp = ir.OFFSET_SHAPE
    y = launch(*on(dev, x, gamma, beta), C, Cn, NONE, "fp32").cpu()
    ref, err = instnorm_ref(x, gamma, beta, C, Cn, NONE)
    bound = out_bound(ref, err, "fp32")
    print("offset case: max error / bound = {:.4f}, max error = {:.3e}".format(float(((y.double() - ref).abs() / bound).max()),
                                                                             float((y.double() - ref).abs().max())))
    _check(y, ref, bound, "offset case")


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_batch_position_and_repeat_keep_their_bits(dtype, cuda_device):
    """image 1 of a batch of 3 whose image 0 is scaled by 100 equals the same image run alone, bit for bit; two runs are identical"""
    dev = cuda_device
    for shape in ((3, 14, 14, 256, 128, 256), (3, 33, 31, 40, 40, 40), (3, 6, 6, 32, 16, 48)):
        N, H, W, C, Cn, xp = shape
        x, gamma, beta = make_inputs(shape, TDT[dtype], seed=3)
        x[0] = (x[0].float() * 100).to(TDT[dtype])
        xd, gd, bd = on(dev, x, gamma, beta)
        y = launch(xd, gd, bd, C, Cn, RELU, dtype)
        y2 = launch(xd, gd, bd, C, Cn, RELU, dtype)
        alone = launch(xd[1:2].contiguous(), gd, bd, C, Cn, RELU, dtype)
        with util.tuning(max_blocks=8):
            alone8 = launch(xd[1:2].contiguous(), gd, bd, C, Cn, RELU, dtype)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), shape
        assert torch.equal(y[1:2], alone) and torch.equal(alone, alone8), shape


def test_refusals_launch_nothing(cuda_device):
    dev = cuda_device
    shape = (2, 6, 6, 32, 16, 48)
    N, H, W, C, Cn, xp = shape
    x, gamma, beta = on(dev, *make_inputs(shape, torch.float16))
    bad = [("null x", dict(x=None)), ("null gamma", dict(gamma=None)), ("null beta", dict(beta=None)), ("null y", dict(y=None)),
           ("null workspace", dict(ws=None)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-1)), ("HW = 0", dict(HW=0)), ("C = 0", dict(C=0)),
           ("Cn < 0", dict(Cn=-8)), ("Cn > C", dict(Cn=40)), ("C % 8", dict(C=28)), ("Cn % 8", dict(Cn=12)), ("x_cpitch % 8", dict(xp=44)),
           ("x_cpitch < C", dict(xp=24)), ("eps = 0", dict(eps=0.0)), ("eps < 0", dict(eps=-1e-5)), ("eps inf", dict(eps=float("inf"))),
           ("eps nan", dict(eps=float("nan"))), ("act 7", dict(act=7)), ("act -1", dict(act=-1)), ("dtype 3", dict(dtype=3)),
           ("dtype -1", dict(dtype=-1))]
    for what, over in bad:
        rc, msg, y = launch(x, gamma, beta, C, Cn, RELU, "fp16", rc_only=True, over=over)
        torch.cuda.synchronize()
        assert rc == INVALID and "pcv_instnorm_act" in msg, (what, rc, msg)
        assert bool(torch.isnan(y).all()), what
    rc, msg, y = launch(x, gamma, beta, C, Cn, RELU, "fp16", rc_only=True, over=dict(N=1 << 20, HW=1 << 10))       # 2^30 * 48 * 2 bytes
    assert rc == TOO_LARGE and "2 GiB" in msg and bool(torch.isnan(y).all())
    lb, L, ctx = _lib()
    assert L.pcv_instnorm_act(None, _p(x), _p(gamma), _p(beta), _p(y), _p(y), N, H * W, C, Cn, xp, ctypes.c_float(1e-5), 1, 2, None) == INVALID
    n = ctypes.c_size_t(0)
    for args in ((0, 8), (2, -8), (2, 12)):
        assert L.pcv_instnorm_workspace_bytes(args[0], args[1], ctypes.byref(n)) == INVALID
        assert "pcv_instnorm_workspace_bytes" in (L.pcv_last_error(None) or b"").decode()
    assert L.pcv_instnorm_workspace_bytes(2, 8, None) == INVALID
    assert L.pcv_instnorm_workspace_bytes(2, 0, ctypes.byref(n)) == 0 and n.value == 0
    # Cn == 0 is a plain activation pass and needs none of gamma / beta / workspace
    rc, msg, y = launch(x, None, None, C, 0, RELU, "fp16", rc_only=True, over=dict(ws=None))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(y, x[:, :, :C].clamp(min=0))


def test_fp16_overflow_moves_the_guard_counter(cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    shape = (2, 5, 5, 24, 8, 24)
    N, H, W, C, Cn, xp = shape
    x, gamma, beta = make_inputs(shape, torch.float16)
    xd, gd, bd = on(dev, x, gamma, beta)
    before = engine.fp16_overflow_count(dev)
    launch(xd, gd, bd, C, Cn, NONE, "fp16")
    assert engine.fp16_overflow_count(dev) == before
    launch(xd, gd * 1e6, bd, C, Cn, NONE, "fp16")
    assert engine.fp16_overflow_count(dev) > before
    mid = engine.fp16_overflow_count(dev)
    launch(xd.to(torch.bfloat16), gd * 1e6, bd, C, Cn, NONE, "bf16")
    assert engine.fp16_overflow_count(dev) == mid
