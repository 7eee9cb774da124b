"""
GPU sweep of the depthwise MixConv launch (csrc/mixconv.hpp behind pcv_mixconv_packed_bytes / pcv_mixconv_pack /
pcv_mixconv2d_fused) through the C ABI against the float64 reference of tests/mixconv_ref.py, in fp32, bf16 and fp16.

The operands are exactly what the kernel reads: x in the compute dtype, the taps read back from the packed blob (and checked
against round_dtype(weight), with every embedded ring exactly zero), the runner's folded fp32 scale / shift (checked against a
float64 BN fold). The bound is the derived depthwise bound of tests/test_gpu_dw_se.py with KK = the channel's own k * k
(mixconv_ref.py); tests/test_mixconv_bounds.py shows on the CPU that plausible bugs violate it.

Shapes (N, C, kernels, stride, H, W):
  (2, 360, 4, 1, 9, 11)    group boundaries at 90 / 180 / 270 (no multiple of 4); map smaller than the 9x9 reach
  (2, 720, 5, 2, 9, 10)    11x11 window at stride 2
  (2, 720, 5, 2, 14, 14)   the 11x11 window on the net's own map
  (3, 144, 3, 2, 15, 16)   odd by even map at stride 2
  (2, 240, 2, 1, 12, 7)    120-wide groups at stride 1, non-square map
  (2, 16, 2, 1, 1, 1)      centre taps only
  (2, 48, 3, 1, 40, 3)     tall map: more than one row strip per column
  (2, 1200, 4, 1, 7, 7)    300-wide groups
  (2, 240, 4, 2, 5, 5)     60-wide groups at stride 2
  (2, 24, 5, 1, 7, 5)      five kernels at stride 1 on the narrowest list the plan takes (groups of 8, 4, 4, 4, 4): the 11x11 window
                           overhangs the whole map, the strips do not divide 7 rows
  (2, 8, 2, 2, 7, 5)       two kernels at stride 2 on 8 channels: ragged last row and column
"""

import ctypes
import pytest
import torch
import torch.nn as nn
import util

from test_gpu_dw_se import (TDT, U32, NONE, RELU, RELU6, SIGMOID, SWISH, HSIGMOID, HSWISH, bn_fold64, _check, _lib, _p, _stream)
from mixconv_ref import mix_operands, mix_ref, out_bound, taps_from_blob, taps_of_group

pytestmark = pytest.mark.gpu

SHAPES = [(2, 360, 4, 1, 9, 11), (2, 720, 5, 2, 9, 10), (2, 720, 5, 2, 14, 14), (3, 144, 3, 2, 15, 16), (2, 240, 2, 1, 12, 7),
          (2, 16, 2, 1, 1, 1), (2, 48, 3, 1, 40, 3), (2, 1200, 4, 1, 7, 7), (2, 240, 4, 2, 5, 5), (2, 24, 5, 1, 7, 5),
          (2, 8, 2, 2, 7, 5)]
DTYPES = ["fp32", "bf16", "fp16"]
OTHER_CODES = (NONE, RELU6, SIGMOID, HSIGMOID, HSWISH)         # every code besides the two the nets use


def _sid(s):
    return "N{}_C{}_k{}_s{}_{}x{}".format(*s)


class MixLayer(object):
    """G depthwise Conv2d + BatchNorm2d on the device and their MixConvRunner (the runner packs the blob and folds the BN)"""
    def __init__(self, ws, bn, s, dev):
        from pytorchcv_amd import engine
        self.G, self.C = len(ws), sum(w.shape[0] for w in ws)
        self.convs = []
        for g, w in enumerate(ws):
            k = 3 + 2 * g
            c = nn.Conv2d(w.shape[0], w.shape[0], k, s, k // 2, groups=w.shape[0], bias=False)
            with torch.no_grad():
                c.weight.copy_(w)
            self.convs.append(c.eval().to(dev))
        self.bn = nn.BatchNorm2d(self.C)
        with torch.no_grad():
            self.bn.weight.copy_(bn[0])
            self.bn.bias.copy_(bn[1])
            self.bn.running_mean.copy_(bn[2])
            self.bn.running_var.copy_(bn[3])
        self.bn.eval().to(dev)
        self.runner = engine.MixConvRunner(self.convs, self.bn)
        self.s = s

    def launch(self, x, act, y=None):
        """pcv_mixconv2d_fused through ctypes into a NaN-filled output: an element no thread writes stays NaN"""
        from pytorchcv_amd import engine
        lb, L, ctx = _lib()
        N, H, W, C = x.shape
        d = self.runner.desc(engine.NHWC(x, N, H, W, C), act)
        self.runner.prepare(engine.NHWC(x, N, H, W, C), d)
        Ho, Wo = (H - 1) // self.s + 1, (W - 1) // self.s + 1
        if y is None:
            y = torch.full((N, Ho, Wo, C), float("nan"), dtype=x.dtype, device=x.device)
        lb.check(L.pcv_mixconv2d_fused(ctx, ctypes.byref(d), self.runner.kernels, self.G, _p(x), _p(self.runner.packed),
                                       _p(self.runner.scale), _p(self.runner.shift), _p(y), _stream()), ctx)
        return y


_cache = {}


def _case(shape, dtype, dev):
    """operands, layer and device input of a (shape, dtype): built once, shared by the tests, never written"""
    key = (shape, dtype)
    if key not in _cache:
        N, C, G, s, H, W = shape
        x, ws, bn = mix_operands(N, H, W, C, G, dtype, seed=100 * C + 10 * G + s)
        layer = MixLayer(ws, bn, s, dev)
        _cache[key] = (x, ws, bn, layer, x.to(dev, TDT[dtype]))
    return _cache[key]


def _reference(shape, dtype, dev, act):
    N, C, G, s, H, W = shape
    x, ws, bn, layer, xd = _case(shape, dtype, dev)
    layer.launch(xd, act)                                   # (packs on first use)
    taps = taps_from_blob(layer.runner.packed, C, G, dtype)
    ref, err = mix_ref(xd.cpu().float(), taps, layer.runner.scale.cpu(), layer.runner.shift.cpu(), s, act)
    return taps, ref, out_bound(ref, err, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=[_sid(s) for s in SHAPES])
def test_mixconv_vs_float64(shape, dtype, cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    N, C, G, s, H, W = shape
    quiet = engine.fp16_overflow_count(dev)
    x, ws, bn, layer, xd = _case(shape, dtype, dev)
    for act in (RELU, SWISH):
        what = "{} {} act{}".format(_sid(shape), dtype, act)
        y = layer.launch(xd, act)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (N, (H - 1) // s + 1, (W - 1) // s + 1, C)
        taps, ref, bound = _reference(shape, dtype, dev, act)
        for g in range(G):                                   # the operands the kernel read: taps = round_dtype(weight) exactly
            assert torch.equal(taps[g], taps_of_group(ws[g], dtype)), what
        s64, h64 = bn_fold64(bn)
        sc, sh = layer.runner.scale.cpu().double(), layer.runner.shift.cpu().double()
        assert bool(((sc - s64).abs() <= 4 * U32 * s64.abs()).all()), what
        assert bool(((sh - h64).abs() <= 2 * U32 * h64.abs() + 6 * U32 * (bn[2].double() * s64).abs()).all()), what
        _check(y.cpu(), ref, bound, what)
    assert engine.fp16_overflow_count(dev) == quiet          # in-range data is not counted


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixconv_remaining_activation_codes(dtype, cuda_device):
    """the 90-wide case with every activation code the two above do not use (both builds of the kernel)"""
    dev = cuda_device
    shape = SHAPES[0]
    x, ws, bn, layer, xd = _case(shape, dtype, dev)
    for act in OTHER_CODES:
        y = layer.launch(xd, act)
        torch.cuda.synchronize()
        _, ref, bound = _reference(shape, dtype, dev, act)
        _check(y.cpu(), ref, bound, "{} {} act{}".format(_sid(shape), dtype, act))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[6]], ids=[_sid(s) for s in (SHAPES[0], SHAPES[2], SHAPES[6])])
def test_mixconv_batch_position_and_reruns_keep_their_bits(shape, dtype, cuda_device):
    """an image's result is bit-identical at batch positions 0 and 2, and from one run to the next"""
    dev = cuda_device
    x, ws, bn, layer, xd = _case(shape, dtype, dev)
    xb = torch.cat([xd[:1], xd[1:2], xd[:1]]).contiguous()
    for act in (RELU, SWISH):
        y = layer.launch(xb, act)
        y2 = layer.launch(xb, act)
        alone = layer.launch(xd[:1].contiguous(), act)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.float()).all())
        assert torch.equal(y[0], y[2]) and torch.equal(y[0], alone[0]), "batch position"
        assert torch.equal(y, y2), "run to run"


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixconv_strip_split_and_flags_keep_their_bits(dtype, cuda_device):
    """Rows per thread dw_th in {1, 2, 3, 5, Ho - 1, Ho} (strips shorter than a window, strips that do not divide Ho, one strip) and
    dw_flags 1 .. 3 (non-temporal stores, dispatch-order blocks) - the depthwise tuning switches this launch honours too: the same
    bits as the automatic split."""
    dev = cuda_device
    for shape in (SHAPES[6], SHAPES[2], SHAPES[0]):
        N, C, G, s, H, W = shape
        Ho = (H - 1) // s + 1
        x, ws, bn, layer, xd = _case(shape, dtype, dev)
        y0 = layer.launch(xd, SWISH)
        torch.cuda.synchronize()
        for th in sorted({1, 2, 3, 5, Ho - 1, Ho} - {0}):
            with util.tuning(dw_th=th):
                y = layer.launch(xd, SWISH)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "dw_th={} on {}".format(th, _sid(shape))
        for flags in (1, 2, 3):
            with util.tuning(dw_flags=flags):
                y = layer.launch(xd, SWISH)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "dw_flags={} on {}".format(flags, _sid(shape))


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixconv_graph_capture_equals_eager(dtype, cuda_device):
    """the launch neither allocates nor synchronises: captured into a graph and replayed it writes the eager bits"""
    dev = cuda_device
    for shape in (SHAPES[0], SHAPES[1]):
        x, ws, bn, layer, xd = _case(shape, dtype, dev)
        eager = layer.launch(xd, SWISH)
        torch.cuda.synchronize()
        static = torch.full_like(eager, float("nan"))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            layer.launch(xd, SWISH, y=static)               # warm-up on a side stream, as torch's capture rules ask
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        static.fill_(float("nan"))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            layer.launch(xd, SWISH, y=static)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager), _sid(shape)
