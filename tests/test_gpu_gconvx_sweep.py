"""
GPU sweep of the any-width grouped 3x3 kernel (csrc/gconvx.hpp) against the float64 reference and the derived bound of
tests/conv_ref.py (tests/test_gconvx_bounds.py proves on the CPU that an fp32 emulation of the kernel's own tiles and K order stays
inside the bound for every case below and that plausible kernel bugs leave it). The sweep drives the C ABI directly with the helpers
of tests/test_gpu_conv_sweep.py. No switch is set: the first assertion of every case restates the library's routing in Python
(tests/gconvx_ref.py: plan_conv's `gconvx`, gconvx_launch_why, plan_gconvx) and checks it against pcv_gconvx_supported. Every case
runs in bf16 and fp16, on the resident grid and under max_blocks = 8 (several tiles per block), into a NaN-filled output with a guard
tail; the same case with "gconvx" 0 (the generic kernel) must hold the same bound. The cases (tests/gconvx_ref.py) are the shapes of
RegNet's layers in small - every group width, group counts 2 .. 19, C % 64 != 0, the 112-wide window, a tail tile that crosses
image borders - and one case on each side of every boundary of the planner.
"""

import contextlib
import ctypes

import pytest
import torch

import util
from gconvx_ref import CASES, CLASS_DECLINED, DECLINED, DTYPES16, X, case_reference, gconvx_static, route
from test_gpu_conv_sweep import GRIDS, Launch, _lib, _p, _stream, case_id, check, make_desc, plan
from test_gpu_dw_se import CODE, NONE, TDT

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def gconvx(value):
    """pcv_set_tuning(ctx, "gconvx", value) for the block (the library's default is 1)"""
    lb, L, ctx = _lib()
    lb.check(L.pcv_set_tuning(ctx, b"gconvx", int(value)), ctx)
    try:
        yield
    finally:
        lb.check(L.pcv_set_tuning(ctx, b"gconvx", 1), ctx)


def supported(c, dtype):
    """(pcv_gconvx_supported's answer, its reason text)"""
    lb, L, ctx = _lib()
    d = make_desc(c, dtype)
    ok = L.pcv_gconvx_supported(ctypes.byref(d))
    return ok, (L.pcv_last_error(None) or b"").decode()


def _params(cases):
    return [pytest.param(c, dt, id=case_id(c) + "-" + dt) for c in cases for dt in DTYPES16]


def _sweep(c, dtype, dev, what, ref=None):
    ops, ref, bound = ref or case_reference(c, dtype)
    run = Launch(c, dtype, ops, dev)
    assert tuple(ref.shape) == run.oshape
    for g in GRIDS:
        name = "{} {} {} grid {}".format(what, case_id(c), dtype, g)
        with util.tuning(max_blocks=g):
            out, outside, tail = run.run()
        assert bool(torch.isnan(tail).all()), name + ": the guard tail behind y was written"
        if outside is not None:
            assert bool(torch.isnan(outside).all()), name + ": channels outside the slice of y were written"
        check(out, ref, bound, name, what, dtype)
    return ops, ref, bound


@pytest.mark.parametrize("c,dtype", _params(CASES))
def test_gconvx_kernel_and_generic_kernel_vs_float64(c, dtype, cuda_device):
    xp = route(c, dtype)
    ok, why = supported(c, dtype)
    assert xp is not None and ok == 1, (xp, why)
    assert not plan(c, dtype).gconv                                # not a shape of the ResNeXt kernels
    ref = _sweep(c, dtype, cuda_device, "gconvx")
    with gconvx(0):
        _sweep(c, dtype, cuda_device, "generic", ref)


@pytest.mark.parametrize("c,dtype", _params(DECLINED))
def test_declined_launches_run_on_the_generic_kernel(c, dtype, cuda_device):
    """a residual with post_act, a padded x_cpitch, a sliced y: statically the kernel's shape, routed to the generic kernel"""
    ok, why = supported(c, dtype)
    assert gconvx_static(c, dtype) and route(c, dtype) is None and ok == 0 and why.startswith("pcv_gconvx_supported: "), why
    assert "generic kernel" in why
    ops, _, _ = _sweep(c, dtype, cuda_device, "declined")
    run = Launch(c, dtype, ops, cuda_device)
    with gconvx(0):                                                # ... switch or no switch: the same kernel, the same bits
        a = run.run()[0]
    assert torch.equal(a, run.run()[0])


@pytest.mark.parametrize("c,dtype", _params(CLASS_DECLINED))
def test_classes_the_measurement_sent_back_run_on_the_generic_kernel(c, dtype, cuda_device):
    """shapes the kernel could run but measured slower on (gconvx_pays): the predicate says so, the generic kernel holds the bound"""
    ok, why = supported(c, dtype)
    assert gconvx_static(c, dtype) and route(c, dtype) is None and ok == 0 and "measured slower" in why, why
    _sweep(c, dtype, cuda_device, "class")


def test_fp16_guard_counts_exactly_the_outputs_beyond_range(cuda_device):
    """three outputs pushed past 65 520 by the scale, each in another group (= another unit, committed by its wave on its own): the context's
    overflow counter moves by exactly three. Every other output is exactly zero: the input holds three ones, the weights one centre
    tap per chosen output channel."""
    from pytorchcv_amd import engine
    from conv_ref import Operands
    c = X(3, 152, 8, 4, 6, 1, act=NONE)
    assert route(c, "fp16") is not None and supported(c, "fp16")[0] == 1
    hits = [(0, 1, 2, 5), (1, 0, 0, 83), (2, 3, 5, 150)]           # (n, h, w, output channel): groups 0, 10, 18
    x = torch.zeros((c.N, c.H, c.W, c.Cin))
    w = torch.zeros((c.Cout, 8, 3, 3))
    for n, h, wc, o in hits:
        x[n, h, wc, o // 8 * 8 + 3] = 1.0
        w[o, 3, 1, 1] = 1.0
    ops = Operands(x, w, torch.full((c.Cout,), 70000.0), torch.zeros(c.Cout), None, None)
    run = Launch(c, "fp16", ops, cuda_device)
    for g in GRIDS:
        before = engine.fp16_overflow_count(cuda_device)
        with util.tuning(max_blocks=g):
            out, _, tail = run.run()
        assert engine.fp16_overflow_count(cuda_device) - before == len(hits), g
        assert bool(torch.isnan(tail).all())
        out = out.float().cpu()
        assert int(torch.isinf(out).sum()) == len(hits) and all(bool(torch.isinf(out[n, h, wc, o])) for n, h, wc, o in hits)
        assert int((out != 0).sum()) == len(hits)


def test_predicate_follows_the_switches_of_the_descriptor_only(cuda_device):
    """pcv_gconvx_supported is host arithmetic on the descriptor: fp32, an odd map at stride 2 and a 113-wide map are refused with a text"""
    base = X(2, 56, 8, 6, 8, 2)
    assert supported(base, "bf16")[0] == 1
    for c, dt, word in ((base, "fp32", "16-bit"), (X(2, 56, 8, 7, 8, 2), "bf16", "odd"), (X(1, 56, 8, 2, 113, 1), "fp16", "112")):
        ok, why = supported(c, dt)
        assert ok == 0 and why.startswith("pcv_gconvx_supported: ") and word in why, (case_id(c), dt, why)
    assert CODE["bf16"] in (1, 2) and TDT["fp16"] is torch.float16 and NONE == 0
