"""
GPU sweep of the ghost-module launch (csrc/ghost.hpp behind pcv_ghost_dw_fused: cheap depthwise 3x3 + concatenation at channel
offset Cm + skip add; the clamp-only FAST build and the general-activation build; fp32 / bf16 / fp16 = 6 instances) against the
float64 reference and derived bound of tests/ghost_ref.py (checked on the CPU against bug models by tests/test_ghost_bounds.py), plus
its bit-for-bit invariances and the new activation code PCV_ACT_CLAMP01 in pcv_se_excite.

The operands are exactly what the kernel reads: m in the compute dtype with a large finite sentinel in its pad channels (a pad
channel that reached y would break the bound or the exact copy), the taps read back from the runner's packed blob at pitch
round8(Cm), the runner's folded fp32 scale / shift. y is NaN-filled before every launch: an element nobody writes stays NaN.
"""

import ctypes
import pytest
import torch
import torch.nn as nn
import util
import ghost_ref as gr
from ghost_ref import CLAMP01, SWEEP_SHAPES, round8
from test_gpu_dw_se import TDT, U32, NONE, RELU, RELU6, SIGMOID, SWISH, HSIGMOID, HSWISH, bn_fold64, fc_ref, se_mlp, _check, _lib, _p, _stream

pytestmark = pytest.mark.gpu

DTYPES = ["fp32", "bf16", "fp16"]
PCV_ERR_INVALID = -1


def _sid(s):
    return "n{}_c{}_{}x{}".format(*s)


class GhostLayer(object):
    """the cheap convolution of a ghost module - depthwise Conv2d(Cm) + BatchNorm2d - on the device, and its plain ConvRunner"""
    def __init__(self, w, bn, dev):
        from pytorchcv_amd import engine
        Cm = w.shape[0]
        self.conv = nn.Conv2d(Cm, Cm, 3, 1, 1, groups=Cm, bias=False)
        self.bn = nn.BatchNorm2d(Cm)
        with torch.no_grad():
            self.conv.weight.copy_(w)
            for dst, src in zip((self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var), bn):
                dst.copy_(src)
        self.conv.eval().to(dev)
        self.bn.eval().to(dev)
        self.runner = engine.ConvRunner(self.conv, self.bn)
        self.Cm, self.CP = Cm, round8(Cm)

    def desc(self, m, act, has_res, y_cpitch=None):
        """packs on first use (the runner's physical descriptor) and returns the launch's logical one"""
        from pytorchcv_amd import engine
        N, H, W, CP = m.shape
        assert CP == self.CP
        h = engine.NHWC(m, N, H, W, self.Cm, cpitch=CP)
        self.runner.prepare(h, self.runner.desc(h, act if act <= HSWISH else 0, 0, False))
        d = self.runner.desc(h, 0, 0, has_res)
        d.act = act
        d.Cin = d.Cout = d.groups = self.Cm
        d.y_cpitch = 2 * self.Cm if y_cpitch is None else y_cpitch
        return d

    def taps(self, dtype):
        es = torch.tensor([], dtype=TDT[dtype]).element_size()
        return self.runner.packed[:9 * self.CP * es].view(TDT[dtype]).view(9, self.CP)

    def launch(self, m, act, dtype, res=None, y=None, y_cpitch=None):
        lb, L, ctx = _lib()
        d = self.desc(m, act, res is not None, y_cpitch)
        assert L.pcv_ghost_supported(ctypes.byref(d)) == 1
        if y is None:
            y = torch.full((m.shape[0], m.shape[1], m.shape[2], 2 * self.Cm), float("nan"), dtype=TDT[dtype], device=m.device)
        lb.check(L.pcv_ghost_dw_fused(ctx, ctypes.byref(d), _p(m), _p(self.runner.packed), _p(self.runner.scale), _p(self.runner.shift),
                                      _p(res), _p(y), _stream()), ctx)
        return y


def _case(shape, dtype, dev, seed, with_res):
    N, Cm, H, W = shape
    m, w, bn, res = gr.ghost_operands(N, Cm, H, W, dtype, seed, with_res)
    layer = GhostLayer(w, bn, dev)
    return m, w, bn, layer, m.to(dev, TDT[dtype]), (res.to(dev, TDT[dtype]) if res is not None else None)


def _verify(layer, md, rd, y, act, dtype, what):
    Cm = layer.Cm
    ref, err = gr.ghost_ref(md, layer.taps(dtype).float(), layer.runner.scale, layer.runner.shift, Cm, act, rd)
    bound = gr.ghost_bound(ref, err, dtype, Cm, rd is not None)
    assert not bool(torch.isnan(y.float()).any()), what + ": NaN left in y"
    if rd is None:
        assert torch.equal(y[..., :Cm], md[..., :Cm]), what + ": main half is not a copy of m"
    _check(y[..., Cm:], ref[..., Cm:], bound[..., Cm:], what + " cheap half")
    _check(y[..., :Cm], ref[..., :Cm], bound[..., :Cm], what + " main half")


# ---- 1. vs float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=[_sid(s) for s in SWEEP_SHAPES])
def test_ghost_launch_vs_float64(shape, dtype, cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    quiet = engine.fp16_overflow_count(dev)
    N, Cm, H, W = shape
    acts = (NONE, RELU) + ((RELU6, SIGMOID, SWISH, HSIGMOID, HSWISH, CLAMP01) if shape == SWEEP_SHAPES[0] else ())
    for with_res in (False, True):
        m, w, bn, layer, md, rd = _case(shape, dtype, dev, seed=1000 + 7 * Cm + H, with_res=with_res)
        for i, act in enumerate(acts):
            what = "{} {} act{} res{}".format(_sid(shape), dtype, act, with_res)
            y = layer.launch(md, act, dtype, rd, y_cpitch=(0 if i % 2 else None))
            torch.cuda.synchronize()
            assert tuple(y.shape) == (N, H, W, 2 * Cm)
            if i == 0:
                # the operands the kernel read: taps = round_dtype(weight) exactly, zero in the pad channels; scale / shift = the
                # float64 fold to fp32 rounding
                assert torch.equal(layer.taps(dtype).float().cpu(), gr.padded_taps(w, dtype)), what
                s64, h64 = bn_fold64(bn)
                sc, sh = layer.runner.scale.cpu().double()[:Cm], layer.runner.shift.cpu().double()[:Cm]
                assert bool(((sc - s64).abs() <= 4 * U32 * s64.abs()).all()), what
                assert bool(((sh - h64).abs() <= 2 * U32 * h64.abs() + 6 * U32 * (bn[2].double() * s64).abs()).all()), what
                assert float(md[..., Cm:].float().abs().min()) == gr.SENTINEL if Cm % 8 else True
            _verify(layer, md, rd, y, act, dtype, what)
    assert engine.fp16_overflow_count(dev) == quiet          # in-range data is not counted


# ---- 2. the fp16 range guard ---------------------------------------------------------------------------------------------------
def test_fp16_overflow_of_a_main_half_sum_moves_the_counter(cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    shape = (2, 12, 9, 11)
    m, w, bn, layer, md, rd = _case(shape, "fp16", dev, seed=31, with_res=True)
    before = engine.fp16_overflow_count(dev)
    layer.launch(md, RELU, "fp16", rd)
    assert engine.fp16_overflow_count(dev) == before
    md2, big = md.clone(), rd.clone()
    md2[1, 4, 5, 3] = 600.0
    big[1, 4, 5, 3] = 64992.0                               # main half: 600 + 64992 >= 65520 rounds to infinity in fp16
    y = layer.launch(md2, RELU, "fp16", big)
    assert engine.fp16_overflow_count(dev) > before
    assert bool(torch.isinf(y[1, 4, 5, 3]))
    mid = engine.fp16_overflow_count(dev)
    layer16 = _case(shape, "bf16", dev, seed=31, with_res=True)[3]
    layer16.launch(md2.to(torch.bfloat16), RELU, "bf16", big.to(torch.bfloat16))
    assert engine.fp16_overflow_count(dev) == mid           # bf16 shares fp32's range: not counted


# ---- 3. invariances, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_batch_position_and_rerun_keep_their_bits(dtype, cuda_device):
    dev = cuda_device
    shape = (3, 36, 10, 3)
    m, w, bn, layer, md, rd = _case(shape, dtype, dev, seed=77, with_res=True)
    md[2], rd[2] = md[0], rd[0]
    for act, res in ((RELU, rd), (HSWISH, None)):
        y = layer.launch(md, act, dtype, res)
        again = layer.launch(md, act, dtype, res)
        alone = layer.launch(md[0:1].contiguous(), act, dtype, res[0:1].contiguous() if res is not None else None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.float()).all())
        assert torch.equal(y, again)
        assert torch.equal(y[0], y[2]) and torch.equal(y[0], alone[0]) and not torch.equal(y[0], y[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_strip_split_and_flags_keep_their_bits(dtype, cuda_device):
    """rows per thread dw_th in {1, 2, 3, H - 1, H} (strips shorter than the 3-row prefetch ring, strips that do not divide H, one
    strip) and dw_flags 1 .. 3 (non-temporal stores, dispatch-order blocks): the same bits as the automatic split"""
    dev = cuda_device
    for shape, act, with_res in (((2, 36, 40, 3), RELU, True), ((2, 12, 9, 11), SWISH, False)):
        N, Cm, H, W = shape
        m, w, bn, layer, md, rd = _case(shape, dtype, dev, seed=55 + H, with_res=with_res)
        y0 = layer.launch(md, act, dtype, rd)
        _verify(layer, md, rd, y0, act, dtype, "automatic split " + _sid(shape))
        for th in sorted({1, 2, 3, H - 1, H}):
            with util.tuning(dw_th=th):
                y = layer.launch(md, act, dtype, rd)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "dw_th={} on {}".format(th, _sid(shape))
        for flags in (1, 2, 3):
            with util.tuning(dw_flags=flags):
                y = layer.launch(md, act, dtype, rd)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "dw_flags={} on {}".format(flags, _sid(shape))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_graph_capture_equals_eager(dtype, cuda_device):
    """the launch neither allocates nor synchronises: captured into a graph and replayed it writes the eager bits"""
    dev = cuda_device
    shape = (2, 20, 9, 7)
    m, w, bn, layer, md, rd = _case(shape, dtype, dev, seed=91, with_res=True)
    eager = layer.launch(md, RELU, dtype, rd)
    torch.cuda.synchronize()
    static = torch.full_like(eager, float("nan"))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        layer.launch(md, RELU, dtype, rd, y=static)             # warm-up on a side stream, as torch's capture rules ask
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    static.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.launch(md, RELU, dtype, rd, y=static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)


# ---- 4. what only the launch can refuse (the descriptor's refusals: tests/test_ghostnet_host.py) --------------------------------
def test_launch_refuses_a_null_residual_and_misaligned_pointers(cuda_device):
    lb, L, ctx = _lib()
    dev = cuda_device
    m, w, bn, layer, md, rd = _case((2, 12, 5, 5), "bf16", dev, seed=3, with_res=True)
    y = torch.full((2, 5, 5, 24), float("nan"), dtype=torch.bfloat16, device=dev)
    r = layer.runner
    d = layer.desc(md, RELU, True)
    rc = L.pcv_ghost_dw_fused(ctx, ctypes.byref(d), _p(md), _p(r.packed), _p(r.scale), _p(r.shift), None, _p(y), _stream())
    assert rc == PCV_ERR_INVALID and b"residual is NULL" in L.pcv_last_error(ctx)
    off = md.reshape(-1)[4:]                                    # 8 bytes past a 16-byte boundary
    for args in ((_p(off), _p(r.packed), _p(r.scale), _p(r.shift), _p(rd), _p(y)),
                 (_p(md), _p(r.packed), _p(r.scale), _p(r.shift), _p(rd.reshape(-1)[4:]), _p(y)),
                 (_p(md), _p(r.packed), _p(r.scale), _p(r.shift), _p(rd), _p(y.reshape(-1)[4:]))):
        rc = L.pcv_ghost_dw_fused(ctx, ctypes.byref(d), *args, _stream())
        assert rc == PCV_ERR_INVALID and b"16-byte aligned" in L.pcv_last_error(ctx)
    d.act = 8
    rc = L.pcv_ghost_dw_fused(ctx, ctypes.byref(d), _p(md), _p(r.packed), _p(r.scale), _p(r.shift), _p(rd), _p(y), _stream())
    assert rc == PCV_ERR_INVALID and b"activation" in L.pcv_last_error(ctx)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all())                   # nothing was launched


# ---- 5. the clamp gate of GhostNet's SE blocks ---------------------------------------------------------------------------------
def test_se_excite_with_the_clamp01_gate_vs_float64(cuda_device):
    lb, L, ctx = _lib()
    dev = cuda_device
    N, C, M = 3, 72, 18
    g = torch.Generator().manual_seed(4242)
    mean = torch.randn(N, C, generator=g)
    w1, b1, w2, b2 = [t.to(dev).contiguous() for t in se_mlp(C, M, C + M)]
    md = mean.to(dev)
    mid = torch.full((N, M), float("nan"), device=dev)
    gate = torch.full((N, C), float("nan"), device=dev)
    lb.check(L.pcv_se_excite(ctx, _p(md), _p(w1), _p(b1), _p(w2), _p(b2), _p(mid), _p(gate), N, C, M, RELU, CLAMP01, _stream()), ctx)
    torch.cuda.synchronize()
    r_mid, _, e_mid = fc_ref(md, w1, b1, RELU)
    _check(mid, r_mid, e_mid, "mid (layer 1)")
    _, pre, e_pre = fc_ref(mid, w2, b2, NONE)                   # layer 2 on the kernel's own mid; clamp is 1-Lipschitz and exact
    _check(gate, pre.clamp(0, 1), e_pre, "gate = clamp(pre, 0, 1)")
    assert float(gate.min()) == 0.0 and float(gate.max()) == 1.0 and bool(((gate > 0) & (gate < 1)).any())
    # the hard sigmoid of the other families is another function: the code is not an alias
    hs = torch.full((N, C), float("nan"), device=dev)
    lb.check(L.pcv_se_excite(ctx, _p(md), _p(w1), _p(b1), _p(w2), _p(b2), _p(mid), _p(hs), N, C, M, RELU, HSIGMOID, _stream()), ctx)
    torch.cuda.synchronize()
    assert not torch.equal(hs, gate)
