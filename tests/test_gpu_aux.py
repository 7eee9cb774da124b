"""
GPU sweep of the layout, pooling, channel-plumbing, interpolation and BatchNorm + activation kernels of csrc/aux_kernels.hpp
(nchw_to_nhwc_kernel, nhwc_to_nchw_kernel, maxpool_kernel, spatial_mean_kernel behind pcv_global_avgpool, channel_slice_kernel,
channel_interleave2_kernel, channel_concat_kernel, interpolate_kernel, bn_act_kernel), through the C ABI and through the engine
wrappers that choose the pitches, in fp32 / bf16 / fp16.

The operands are exactly what the kernels read: every input is rounded to the compute dtype first and the references see the
rounded values. Physical channels the kernel must not read (c >= C of an input) hold NaN. Outputs of the raw ABI calls live at
the front of a larger allocation filled with a sentinel bit pattern (a signalling-NaN pattern no kernel here produces): after the
launch every owned element must differ from the sentinel and everything behind the tensor must still hold it.

Kernels that copy or select values are compared bit for bit (the integer view of the tensors; max-pool by value and NaN mask, as
IEEE-754-2019 maximum may return +0 where v_max returned -0):
  nchw -> nhwc     y[n, h, w, c] = round_dtype(x[n, c, h, w]); pad channels and pad columns +0
  nhwc -> nchw     the inverse, fp32 out
  max-pool         F.max_pool2d of the rounded input in fp32 (max selects an input), the same NaN mask
  slice            y[.., i] = x[.., off + i], pads +0
  interleave2      channel_shuffle(cat(a[:, :Ch], b[:, :Ch]), 2) as torch computes it on NCHW, pads +0
  concat           buf[.., off:off + C] = x[.., :C], nothing else touched
  nearest          F.interpolate(mode="nearest") in fp32
  global avg-pool  fp32 out: the bits of pcv_se_squeeze (the same kernel)

Arithmetic kernels against float64 with derived bounds, first order in u = 2^-24; the output rounding U |ref| + (1 + U) e + F is
out_bound of tests/test_gpu_dw_se.py:
  global avg-pool, output in the compute dtype: mean_ref's (HW + 1) u mean|x|.
  bilinear : source coordinates f and lambda = f - floor(f) are computed in fp32 exactly as the kernel and ATen state them, the
             four-corner blend v = (1 - lh) ((1 - lw) a + lw b) + lh ((1 - lw) c + lw d) in float64 with w_i the exact products of
             (1 - l), l.
             (1) The kernel rounds 1 - lw and 1 - lh (one rounding each), the two inner products, the inner sum, the outer
                 product and the outer sum: the a-term passes six roundings (fewer when the compiler contracts to fma), the other
                 terms at most five: |e1| <= 6 u sum_i w_i |x_i|.
             (2) Without align_corners f = (dst + 0.5) scale - 0.5. hipcc may contract that into one fma, which skips the rounding
                 of the product p = (dst + 0.5) scale < in: with p rounded or not and the final rounding on either value,
                 |df| <= u p + 2 u |p - 0.5| <= 3 u in, per axis; f - floor(f) is exact in fp32. v is continuous and piecewise
                 linear in each f, with a slope of at most R = max corner - min corner of the cell it is in:
                 |e2| <= 3 u (H + W) R <= 6 u max(H, W) R. Only where the reference's f lies within 3 u in of an integer (in 5 ->
                 out 9 has such a coordinate) can the kernel's f land in the neighbouring cell; for those output rows / columns
                 R is taken over the corners and their neighbours (rows h0 - 1 .. h1 + 1, columns w0 - 1 .. w1 + 1, clipped).
                 With align_corners f = dst * ((in - 1) / (out - 1)) is a single rounded product in the kernel, the reference
                 and ATen alike: e2 = 0.
  bn_act   : y = act(x scale + shift) as one fma or a product and a sum: |e_pre| <= 2 u (|x scale| + |shift|), pushed through
             act_err of tests/test_gpu_dw_se.py.
The bounds are not fitted to observed errors; tests/test_aux_bounds.py checks on the CPU that every restatement here agrees with
torch, that plausible kernel bugs violate the assertions, and that the shape lists reach the branches they claim.
"""

import ctypes
import functools
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import util

from test_gpu_dw_se import (CODE, FLOOR, TDT, U32, ULP, _check, _lib, _p, _stream, act64, act_err, bn_fold64,  # noqa: F401
                            mean_ref, out_bound)

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16", "fp16")
NAN = float("nan")
INF = float("inf")
# a signalling-NaN pattern per element type: torch's NaN is 0x7FC0.. / 0x7E00, no arithmetic result carries these bits
SENTINEL = {torch.float32: 0x7FA5A5A5, torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5}
TAIL = 64                                   # sentinel elements behind every guarded output


def round8(c):
    return (c + 7) // 8 * 8


def rd(x, dtype):
    """x rounded to the compute dtype, as fp32"""
    return x.to(TDT[dtype]).float()


def bits(t):
    """the raw bit patterns of a floating tensor"""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def guarded(shape, tdt, dev):
    """(whole allocation, the tensor of `shape` at its front): every element holds the sentinel"""
    n = _numel(shape)
    flat = torch.full((n + TAIL,), SENTINEL[tdt], dtype=torch.int32 if tdt == torch.float32 else torch.int16, device=dev).view(tdt)
    return flat, flat[:n].view(shape)


def guard_violation(flat, n):
    """None when every owned element was written and nothing behind the tensor was"""
    b = bits(flat).cpu()
    s = SENTINEL[flat.dtype]
    if not bool((b[:n] != s).all()):
        return "{} owned elements were never written".format(int((b[:n] == s).sum()))
    if not bool((b[n:] == s).all()):
        return "written behind the tensor"
    return None


def assert_guard(flat, n, what):
    bad = guard_violation(flat, n)
    assert bad is None, "{}: {}".format(what, bad)


def assert_bits(out, ref, what):
    out = out.cpu()
    assert out.shape == ref.shape and out.dtype == ref.dtype, "{}: {} {} vs {} {}".format(what, out.shape, out.dtype, ref.shape, ref.dtype)
    bad = bits(out) != bits(ref)
    if bool(bad.any()):
        i = int(torch.where(bad.flatten())[0][0])
        pytest.fail("{}: {} of {} elements differ in their bits; first at flat index {}: got {!r}, want {!r}".format(
            what, int(bad.sum()), bad.numel(), i, float(out.flatten()[i]), float(ref.flatten()[i])))


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def with_pads(x, pitch, dtype, fill=NAN):
    """[..., C] fp32 -> [..., pitch] in the compute dtype, physical channels >= C hold `fill`"""
    C = x.shape[-1]
    y = torch.full(tuple(x.shape[:-1]) + (pitch,), fill, dtype=TDT[dtype])
    y[..., :C] = x.to(TDT[dtype])
    return y


def _handle(t, C):
    from pytorchcv_amd import engine
    N, H, W, P = t.shape
    return engine.NHWC(t, N, H, W, C, cpitch=P)


# the two row counts of the channel kernels as maps: 70 rows (one ragged block) and 527 (three blocks, the last ragged)
ROW_MAPS = ((2, 5, 7), (1, 17, 31))


# ---- 1 / 2. layout ----------------------------------------------------------------------------------------------------------------
_ALL = DTYPES
# (N, C, H, W, cpitch, wpitch, dtypes): the stem form (cpitch 4, even wpitch), ragged channel tails under full 8-channel stores,
# the fp32-only cpitch % 4 form, and N H wpitch = 527 (more than one block, the last one ragged)
NCHW_CASES = [(2, 3, 5, 7, 4, 8, _ALL), (1, 1, 3, 5, 4, 6, _ALL), (1, 4, 4, 6, 4, 6, _ALL), (1, 4, 4, 6, 4, 8, _ALL),
              (3, 58, 5, 9, 64, 9, _ALL), (2, 9, 4, 6, 16, 6, _ALL),
              (2, 9, 4, 6, 12, 6, ("fp32",)), (1, 12, 3, 3, 12, 3, ("fp32",)),
              (1, 8, 17, 31, 8, 31, _ALL)]
# (N, C, H, W, cpitch)
NHWC_CASES = [(2, 58, 5, 9, 64), (1, 3, 4, 5, 8), (1, 8, 17, 31, 8)]


def store_branches(cpitch):
    """the store branches of nchw_to_nhwc_kernel a launch reaches: one block row per 8 physical channels"""
    return {"vec8" if cpitch - c0 >= 8 else "vec4" if cpitch - c0 == 4 else "scalar" for c0 in range(0, cpitch, 8)}


def nhwc_ref(x, cpitch, wpitch, dtype):
    """NCHW fp32 -> [N, H, wpitch, cpitch] in the compute dtype, pads +0"""
    N, C, H, W = x.shape
    y = torch.zeros((N, H, wpitch, cpitch), dtype=TDT[dtype])
    y[:, :, :W, :C] = x.permute(0, 2, 3, 1).to(TDT[dtype])
    return y


def nchw_ref(x, C):
    """[N, H, W, cpitch] -> NCHW fp32 of the logical channels"""
    return x[..., :C].permute(0, 3, 1, 2).float().contiguous()


def engine_pitches(C, W, stem):
    return (4, (W + 1) // 2 * 2) if C <= 4 and stem else (round8(C), W)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nchw_to_nhwc_bits(dtype, cuda_device):
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    ran = set()
    for i, (N, C, H, W, cp, wp, dts) in enumerate(NCHW_CASES):
        if dtype not in dts:
            continue
        what = "nchw_to_nhwc {} {}x{}x{}x{} cpitch {} wpitch {}".format(dtype, N, C, H, W, cp, wp)
        x = randn((N, C, H, W), 100 + i)
        x[0, 0, 0, 0] = -0.0
        ref = nhwc_ref(x, cp, wp, dtype)
        xd = x.to(dev)
        flat, y = guarded((N, H, wp, cp), TDT[dtype], dev)
        lb.check(L.pcv_nchw_to_nhwc(ctx, _p(xd), _p(y), N, C, H, W, cp, wp, CODE[dtype], _stream()), ctx)
        torch.cuda.synchronize()
        assert_guard(flat, y.numel(), what)
        assert_bits(y, ref, what)
        ran |= store_branches(cp)
        for stem in (True, False):                               # the pitches the host wrapper chooses
            a = engine.from_nchw(xd, dtype, stem=stem)
            torch.cuda.synchronize()
            assert (a.cpitch, a.wpitch) == engine_pitches(C, W, stem) and (a.N, a.H, a.W, a.C) == (N, H, W, C), what
            assert_bits(a.t, nhwc_ref(x, a.cpitch, a.wpitch, dtype), what + " (engine.from_nchw stem={})".format(stem))
    assert ran == {"vec8", "vec4"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_nhwc_to_nchw_bits_and_round_trip(dtype, cuda_device):
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    for i, (N, C, H, W, cp) in enumerate(NHWC_CASES):
        what = "nhwc_to_nchw {} {}x{}x{}x{} cpitch {}".format(dtype, N, C, H, W, cp)
        x = with_pads(randn((N, H, W, C), 200 + i), cp, dtype)               # NaN in the pad channels
        x[0, 0, 0, 0] = -0.0
        ref = nchw_ref(x, C)
        assert not bool(torch.isnan(ref).any())
        xd = x.to(dev)
        flat, y = guarded((N, C, H, W), torch.float32, dev)
        lb.check(L.pcv_nhwc_to_nchw(ctx, _p(xd), _p(y), N, C, H, W, cp, CODE[dtype], _stream()), ctx)
        torch.cuda.synchronize()
        assert_guard(flat, y.numel(), what)
        assert_bits(y, ref, what)
        assert_bits(engine.to_nchw(_handle(xd, C)), ref, what + " (engine.to_nchw)")
    for i, (N, C, H, W, _, _, _) in enumerate(NCHW_CASES):                  # the round trip of the canonical layout
        x = randn((N, C, H, W), 300 + i)
        back = engine.to_nchw(engine.from_nchw(x.to(dev), dtype, stem=False))
        torch.cuda.synchronize()
        assert_bits(back, rd(x, dtype), "round trip {} {}x{}x{}x{}".format(dtype, N, C, H, W))


# ---- 3. max-pool ------------------------------------------------------------------------------------------------------------------
POOL_CONFIGS = [(3, 2, 1, 0), (2, 2, 0, 0), (3, 1, 1, 0), (3, 2, 0, 1), (3, 2, 1, 1), (2, 2, 0, 1), (5, 1, 2, 0), (1, 1, 0, 0),
                (3, 3, 1, 1)]                                                # (k, s, p, ceil_mode)
POOL_MAPS = [(2, 7, 9, 8), (3, 8, 5, 24), (1, 1, 1, 8), (1, 2, 2, 8), (2, 13, 3, 64), (1, 17, 31, 16)]   # (N, H, W, C)
POOL_KINDS = ("negative", "inf", "nan")


def pool_out(n, k, s, p, ceil_mode):
    """torch's pooled size (restated; tests/test_aux_bounds.py compares it with torch and with engine._pool_out)"""
    o = (n + 2 * p - k + (s - 1 if ceil_mode else 0)) // s + 1
    if ceil_mode and (o - 1) * s >= n + p:
        o -= 1                                  # the last window must start inside the map or its left padding
    return o


def pool_cases():
    """every (configuration, map) torch accepts: a non-empty pooled map"""
    return [(cfg, m) for cfg in POOL_CONFIGS for m in POOL_MAPS
            if pool_out(m[1], *cfg) >= 1 and pool_out(m[2], *cfg) >= 1]


def pool_coverage(n, k, s, p, ceil_mode):
    """how many windows cover each input index along one axis"""
    cover = [0] * n
    for o in range(pool_out(n, k, s, p, ceil_mode)):
        for i in range(max(0, o * s - p), min(n, o * s - p + k)):
            cover[i] += 1
    return cover


def nan_pixels(H, W, cfg):
    """where the NaN data plants its NaNs: an interior pixel, the bottom-right corner, and the pixel the fewest windows cover
    (exactly one wherever a configuration has such a pixel)"""
    ch, cw = pool_coverage(H, *cfg), pool_coverage(W, *cfg)
    lone_h = min(range(H), key=lambda i: (ch[i] if ch[i] else 99, i))
    lone_w = min(range(W), key=lambda i: (cw[i] if cw[i] else 99, i))
    return [(H // 2, W // 2), (H - 1, W - 1), (lone_h, lone_w)]


@functools.lru_cache(maxsize=None)
def pool_input(cfg, m, kind, dtype):
    """NHWC fp32 values representable in the compute dtype. -|synth_input - 3|: synth_input - 3 wherever that is negative (all but
    a few in ten thousand values), so a zero pad or a zero-initialised maximum shows in every window that touches the border."""
    N, H, W, C = m
    x = -(util.synth_input(N, C, H, W, seed=41 + H + W) - 3).abs()
    x = rd(x.permute(0, 2, 3, 1).contiguous(), dtype)
    if kind == "inf":
        r = torch.rand(x.shape, generator=torch.Generator().manual_seed(7 + H * W + C))
        x[r < 0.08] = -INF
        x[r > 0.94] = INF
    if kind == "nan":
        for (h, w) in nan_pixels(H, W, cfg):
            x[0, h, w, 1] = NAN
            x[N - 1, h, w, C - 2] = NAN
    return x


@functools.lru_cache(maxsize=None)
def pool_ref(cfg, m, kind, dtype):
    k, s, p, ceil = cfg
    x = pool_input(cfg, m, kind, dtype)
    return F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p, ceil_mode=bool(ceil)).permute(0, 2, 3, 1).contiguous()


def pool_mismatch(out, ref):
    """None when `out` has the reference's shape, its NaN mask and, outside the mask, its values (zeros compare by value)"""
    if out.shape != ref.shape:
        return "shape {} instead of {}".format(tuple(out.shape), tuple(ref.shape))
    no, nr = torch.isnan(out), torch.isnan(ref)
    if not torch.equal(no, nr):
        return "NaN mask: {} NaN outputs, torch has {}; {} positions differ".format(int(no.sum()), int(nr.sum()), int((no != nr).sum()))
    if not torch.equal(out.masked_fill(no, 0.0), ref.masked_fill(nr, 0.0)):
        bad = out.masked_fill(no, 0.0) != ref.masked_fill(nr, 0.0)
        i = int(torch.where(bad.flatten())[0][0])
        return "{} values differ; first at flat index {}: got {!r}, want {!r}".format(int(bad.sum()), i, float(out.flatten()[i]),
                                                                                      float(ref.flatten()[i]))
    return None


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_equals_torch(dtype, kind, cuda_device):
    """All physical channels are pooled (the pad channels are ordinary channels to this kernel); the engine handle below declares
    the last three of them pads and must return the same tensor."""
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    cases = pool_cases()
    for (cfg, m) in cases:
        k, s, p, ceil = cfg
        N, H, W, C = m
        what = "maxpool {} {} k{} s{} p{} ceil{} on {}x{}x{}x{}".format(dtype, kind, k, s, p, ceil, N, H, W, C)
        ref = pool_ref(cfg, m, kind, dtype)
        Ho, Wo = pool_out(H, *cfg), pool_out(W, *cfg)
        assert (Ho, Wo) == (engine._pool_out(H, k, s, p, bool(ceil)), engine._pool_out(W, k, s, p, bool(ceil))) == tuple(ref.shape[1:3])
        xd = pool_input(cfg, m, kind, dtype).to(dev, TDT[dtype])
        flat, y = guarded((N, Ho, Wo, C), TDT[dtype], dev)
        lb.check(L.pcv_maxpool2d(ctx, _p(xd), _p(y), N, H, W, C, k, s, p, ceil, CODE[dtype], _stream()), ctx)
        torch.cuda.synchronize()
        assert_guard(flat, y.numel(), what)
        bad = pool_mismatch(y.float().cpu(), ref)
        assert bad is None, "{}: {}".format(what, bad)
        e = engine.maxpool2d(_handle(xd, C - 3), k, s, p, bool(ceil))
        torch.cuda.synchronize()
        assert (e.H, e.W, e.C, e.cpitch) == (Ho, Wo, C - 3, C), what
        bad = pool_mismatch(e.t.float().cpu(), ref)
        assert bad is None, "{} (engine.maxpool2d): {}".format(what, bad)
    assert len(cases) >= 45


@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_maxpool_nan_fused_equals_two_launches(dtype, cuda_device):
    """The ResNet init block at (2, 33, 35) with one NaN input pixel: the stem convolution followed by the stand-alone pool gives
    NaN exactly where torch's max_pool2d of the stem's output does, and (16-bit, where the fused kernel exists) the one-launch
    stem + pool has the same NaN mask and the same bits outside it. fp32 has no fused form: run_maxpool must say so, and the block's
    own forward is held to the same comparison."""
    import pytorchcv_amd
    from pytorchcv_amd import engine
    from pytorchcv_amd.models.resnet import ResInitBlock
    N, H, W = 2, 33, 35
    blk = ResInitBlock(in_channels=3, out_channels=64).eval()
    blk.load_state_dict(util.synth_state_dict(blk.state_dict(), seed=77))
    blk = pytorchcv_amd.set_compute_dtype(blk.to(cuda_device), dtype)
    x = util.synth_input(N, 3, H, W, seed=78)
    x[1, 1, 16, 18] = NAN
    x = x.to(cuda_device)
    with torch.no_grad():
        a = engine.from_nchw(x, dtype, stem=True)
        whole = blk(x)                                  # builds the runner; NCHW fp32 out
        fused = blk.conv._pcv_runner.run_maxpool(a, 1, 3, 2, 1)
        conv = blk.conv(a)
        two = blk.pool(conv)
    torch.cuda.synchronize()
    want = F.max_pool2d(conv.t.float().cpu().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    mask = torch.isnan(want)
    assert 0 < int(mask.sum()) < mask.numel() // 4 and not bool(mask[0].any())
    bad = pool_mismatch(two.t.float().cpu(), want)
    assert bad is None, "stem + stand-alone pool against torch's max_pool2d of the stem output: {}".format(bad)
    if dtype == "fp32":
        assert fused is None
    else:
        assert fused is not None, "the 7x7/2 stem + MaxPool2d(3, 2, 1) must be covered by the fused kernel"
        assert (fused.H, fused.W) == (two.H, two.W)
        bad = pool_mismatch(fused.t.float().cpu(), two.t.float().cpu())
        assert bad is None, "fused stem + pool against the two launches: {}".format(bad)
    bad = pool_mismatch(whole.cpu().permute(0, 2, 3, 1), two.t.float().cpu())
    assert bad is None, "the block's forward against the two launches: {}".format(bad)


# ---- 4 - 6. channel plumbing --------------------------------------------------------------------------------------------------------
SLICE_CASES = [(116, 120, 58, 58), (116, 120, 0, 58), (24, 24, 12, 12), (48, 48, 8, 40), (8, 8, 7, 1), (8, 8, 2, 3),
               (64, 64, 0, 64)]                                             # (C_x, xpitch, offset, count)
# Ch -> (a's pitch: a tensor of its own; b's pitch: the leading channels of a wider tensor)
INTERLEAVE_CASES = {1: (8, 16), 4: (8, 16), 12: (16, 32), 58: (64, 120), 116: (120, 240)}
CONCAT_CASES = [(8, 8, 24, 0), (8, 8, 24, 16), (40, 40, 96, 8), (40, 64, 96, 56), (32, 32, 32, 0)]   # (C, xpitch, ypitch, offset)


def slice_ref(x, off, count, ypitch):
    y = torch.zeros(tuple(x.shape[:-1]) + (ypitch,), dtype=x.dtype)
    y[..., :count] = x[..., off:off + count]
    return y


def channel_shuffle2_nchw(x):
    """channel_shuffle(x, groups=2) of the reference (common/tutti.py): view (N, 2, C / 2, H, W), transpose, flatten"""
    N, C, H, W = x.shape
    return x.view(N, 2, C // 2, H, W).transpose(1, 2).contiguous().view(N, C, H, W)


def interleave_ref(a, b, Ch, ypitch):
    """NHWC a, b -> channel_shuffle(cat(a[:, :Ch], b[:, :Ch]), 2) on NCHW, back to NHWC with zero pads"""
    cat = torch.cat((a[..., :Ch].permute(0, 3, 1, 2), b[..., :Ch].permute(0, 3, 1, 2)), dim=1).contiguous()
    y = torch.zeros(tuple(a.shape[:-1]) + (ypitch,), dtype=a.dtype)
    y[..., :2 * Ch] = channel_shuffle2_nchw(cat).permute(0, 2, 3, 1)
    return y


def concat_ref(buf, x, C, off):
    y = buf.clone()
    y[..., off:off + C] = x[..., :C]
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_slice_bits(dtype, cuda_device):
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    for i, (Cx, xp, off, count) in enumerate(SLICE_CASES):
        for (N, H, W) in ROW_MAPS:
            rows = N * H * W
            x = with_pads(randn((N, H, W, Cx), 400 + i), xp, dtype)
            xd = x.to(dev)
            for yp in (round8(count), round8(count) + 8):
                what = "slice {} C_x {} xpitch {} off {} count {} ypitch {} rows {}".format(dtype, Cx, xp, off, count, yp, rows)
                ref = slice_ref(x, off, count, yp)
                assert not bool(torch.isnan(ref).any())
                flat, y = guarded((N, H, W, yp), TDT[dtype], dev)
                lb.check(L.pcv_channel_slice(ctx, _p(xd), _p(y), rows, count, off, xp, yp, CODE[dtype], _stream()), ctx)
                torch.cuda.synchronize()
                assert_guard(flat, y.numel(), what)
                assert_bits(y, ref, what)
            e = engine.channel_slice(_handle(xd, Cx), off, count)
            torch.cuda.synchronize()
            assert (e.C, e.cpitch) == (count, round8(count))
            assert_bits(e.t, slice_ref(x, off, count, round8(count)), what + " (engine.channel_slice)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_interleave2_bits(dtype, cuda_device):
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    for Ch, (ap, bp) in INTERLEAVE_CASES.items():
        for (N, H, W) in ROW_MAPS:
            rows = N * H * W
            yp = round8(2 * Ch)
            what = "interleave2 {} Ch {} pitches {} / {} -> {} rows {}".format(dtype, Ch, ap, bp, yp, rows)
            a = with_pads(randn((N, H, W, Ch), 500 + Ch), ap, dtype)         # different seeds: a swapped pair cannot pass
            b = with_pads(randn((N, H, W, Ch), 600 + Ch), bp, dtype)
            ref = interleave_ref(a, b, Ch, yp)
            assert not bool(torch.isnan(ref).any())
            ad, bd = a.to(dev), b.to(dev)
            flat, y = guarded((N, H, W, yp), TDT[dtype], dev)
            lb.check(L.pcv_channel_interleave2(ctx, _p(ad), _p(bd), _p(y), rows, Ch, ap, bp, yp, CODE[dtype], _stream()), ctx)
            torch.cuda.synchronize()
            assert_guard(flat, y.numel(), what)
            assert_bits(y, ref, what)
            e = engine.cat_shuffle2(_handle(ad, Ch), _handle(bd, min(bp, 2 * Ch)), Ch)
            torch.cuda.synchronize()
            assert (e.C, e.cpitch) == (2 * Ch, yp)
            assert_bits(e.t, ref, what + " (engine.cat_shuffle2)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_concat_bits(dtype, cuda_device):
    """fp32 copies two 16-byte vectors per thread, the 16-bit types one. The destination starts as the sentinel everywhere: after
    the launch the slice holds x's bits and every other element of the buffer, and everything behind it, still the sentinel."""
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    for i, (C, xp, yp, off) in enumerate(CONCAT_CASES):
        for (N, H, W) in ROW_MAPS:
            rows = N * H * W
            what = "concat {} C {} xpitch {} ypitch {} off {} rows {}".format(dtype, C, xp, yp, off, rows)
            x = with_pads(randn((N, H, W, C), 700 + i), xp, dtype)
            xd = x.to(dev)
            for via_engine in (False, True):
                flat, buf = guarded((N, H, W, yp), TDT[dtype], dev)
                ref = flat.cpu().clone()
                ref[:buf.numel()] = concat_ref(buf.cpu(), x, C, off).flatten()
                if via_engine:
                    engine.channel_concat_into(_handle(xd, C), buf, off)
                else:
                    lb.check(L.pcv_channel_concat(ctx, _p(xd), _p(buf), rows, C, xp, yp, off, CODE[dtype], _stream()), ctx)
                torch.cuda.synchronize()
                assert_bits(flat, ref, what + (" (engine.channel_concat_into)" if via_engine else ""))
                written = bits(buf).cpu() != SENTINEL[TDT[dtype]]
                want = torch.zeros_like(written)
                want[..., off:off + C] = True
                assert torch.equal(written, want), what


# ---- 7 / 9. interpolation ----------------------------------------------------------------------------------------------------------
NEAREST_SIZES = [((5, 6), (10, 12)), ((7, 5), (10, 9)), ((12, 10), (6, 5)), ((9, 7), (4, 3)), ((1, 1), (3, 4)), ((6, 7), (1, 1)),
                 ((4, 5), (4, 5))]
BILINEAR_SIZES = NEAREST_SIZES + [((7, 9), (14, 18)), ((6, 7), (1, 5))]
INTERP_C = (8, 24)
INTERP_N = 2


def nearest_index(inn, out):
    """min(floor(dst * (float) in / (float) out), in - 1) in fp32, as the kernel and ATen state it"""
    scale = torch.tensor(float(inn), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    return torch.floor(torch.arange(out, dtype=torch.float32) * scale).to(torch.int64).clamp(max=inn - 1)


def nearest_ref(x, Ho, Wo):
    return F.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode="nearest").permute(0, 2, 3, 1).contiguous()


def bilinear_source(inn, out, align):
    """the fp32 source coordinate of every destination index: align_corners dst * ((in - 1) / (out - 1)) (0 for out == 1), otherwise
    max(0, (dst + 0.5) * (in / out) - 0.5) - every operation rounded to fp32, nothing fused"""
    d = torch.arange(out, dtype=torch.float32)
    if align:
        if out == 1:
            return torch.zeros(1, dtype=torch.float32)
        return d * (torch.tensor(float(inn - 1), dtype=torch.float32) / torch.tensor(float(out - 1), dtype=torch.float32))
    scale = torch.tensor(float(inn), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    return ((d + 0.5) * scale - 0.5).clamp(min=0)


def bilinear_coords(inn, out, align):
    """(index 0, index 1, lambda) per destination index; lambda = f - floor(f) is exact in fp32"""
    f = bilinear_source(inn, out, align)
    i0 = f.to(torch.int64).clamp(max=inn - 1)
    i1 = (i0 + 1).clamp(max=inn - 1)
    return i0, i1, f - i0.float()


def near_knot(inn, out, align):
    """per destination index: the reference's source coordinate lies within its rounding error 3 u in of an integer, so the
    kernel's may fall into the neighbouring cell"""
    f = bilinear_source(inn, out, align).double()
    return (f - f.round()).abs() <= 3 * U32 * inn


def bilinear_blend(x, hc, wc, in_hw=None, near=None):
    """float64 four-corner blend of NHWC x with the given (index 0, index 1, lambda) per axis. Returns (reference, part 1 of the
    bound 6 u sum w |x|, part 2: 6 u max(H, W) (max corner - min corner); for the rows / columns flagged by `near` = (per-row mask,
    per-column mask) the range is taken over the corners and their neighbours)."""
    x = x.double()
    H, W = x.shape[1:3] if in_hw is None else in_hw
    (h0, h1, lh), (w0, w1, lw) = hc, wc
    lh = lh.double().reshape(1, -1, 1, 1)
    lw = lw.double().reshape(1, 1, -1, 1)
    a, b = x[:, h0][:, :, w0], x[:, h0][:, :, w1]
    c, d = x[:, h1][:, :, w0], x[:, h1][:, :, w1]
    wa, wb, wc_, wd = (1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw
    ref = wa * a + wb * b + wc_ * c + wd * d
    e1 = 6 * U32 * (wa * a.abs() + wb * b.abs() + wc_ * c.abs() + wd * d.abs())
    hs = ((h0 - 1).clamp(min=0), h0, h1, (h1 + 1).clamp(max=x.shape[1] - 1))
    ws = ((w0 - 1).clamp(min=0), w0, w1, (w1 + 1).clamp(max=x.shape[2] - 1))
    corners = torch.stack((a, b, c, d))
    rng = corners.max(0).values - corners.min(0).values
    if near is not None:
        around = torch.stack([x[:, i][:, :, j] for i in hs for j in ws])
        flagged = (near[0].reshape(1, -1, 1, 1) | near[1].reshape(1, 1, -1, 1)).expand_as(rng)
        rng = torch.where(flagged, around.max(0).values - around.min(0).values, rng)
    e2 = 6 * U32 * max(H, W) * rng
    return ref, e1, e2


def bilinear_ref(x, Ho, Wo, align):
    """(float64 reference, bound of the kernel's fp32 error before the output rounding) - see the module docstring"""
    H, W = x.shape[1:3]
    ref, e1, e2 = bilinear_blend(x, bilinear_coords(H, Ho, align), bilinear_coords(W, Wo, align),
                                 near=(near_knot(H, Ho, align), near_knot(W, Wo, align)))
    return ref, e1 if align else e1 + e2


def interp_input(hw, C, dtype):
    H, W = hw
    return rd(randn((INTERP_N, H, W, C), 800 + 10 * H + W + C), dtype)


def _launch_interp(xd, Ho, Wo, bilinear, align, dtype, what):
    lb, L, ctx = _lib()
    N, H, W, C = xd.shape
    flat, y = guarded((N, Ho, Wo, C), TDT[dtype], xd.device)
    lb.check(L.pcv_interpolate(ctx, _p(xd), _p(y), N, H, W, C, Ho, Wo, bilinear, align, CODE[dtype], _stream()), ctx)
    torch.cuda.synchronize()
    assert_guard(flat, y.numel(), what)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolate_nearest_equals_torch(dtype, cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    for (hw, (Ho, Wo)) in NEAREST_SIZES:
        for C in INTERP_C:
            what = "nearest {} {}x{} -> {}x{} C {}".format(dtype, hw[0], hw[1], Ho, Wo, C)
            x = interp_input(hw, C, dtype)
            ref = nearest_ref(x, Ho, Wo).to(TDT[dtype])
            xd = x.to(dev, TDT[dtype])
            assert_bits(_launch_interp(xd, Ho, Wo, 0, 0, dtype, what), ref, what)
            e = engine.interpolate(_handle(xd, C - 2), (Ho, Wo), False, False)
            torch.cuda.synchronize()
            assert (e.H, e.W, e.C, e.cpitch) == (Ho, Wo, C - 2, C)
            assert_bits(e.t, ref, what + " (engine.interpolate)")


@pytest.mark.parametrize("align", [0, 1], ids=["half_pixel", "align_corners"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolate_bilinear_vs_float64(dtype, align, cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    for (hw, (Ho, Wo)) in BILINEAR_SIZES:
        for C in INTERP_C:
            what = "bilinear {} align {} {}x{} -> {}x{} C {}".format(dtype, align, hw[0], hw[1], Ho, Wo, C)
            x = interp_input(hw, C, dtype)
            ref, err = bilinear_ref(x, Ho, Wo, align)
            xd = x.to(dev, TDT[dtype])
            y = _launch_interp(xd, Ho, Wo, 1, align, dtype, what)
            _check(y.cpu(), ref, out_bound(ref, err, dtype), what)
            e = engine.interpolate(_handle(xd, C - 2), (Ho, Wo), True, bool(align))
            torch.cuda.synchronize()
            assert_bits(e.t, y.cpu(), what + " (engine.interpolate)")


# ---- 8. global average pool ----------------------------------------------------------------------------------------------------------
GAP_HW = (1, 49, 50)
GAP_C = (8, 72, 4104)
GAP_N = 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_global_avgpool_bits_and_bound(dtype, cuda_device):
    """fp32 out: pcv_se_squeeze's bits (spatial_mean_kernel both times); compute-dtype out: float64 mean within the summation bound
    and one output rounding. C = 72 leaves rows of the block idle, C = 4104 needs a second channel group."""
    from pytorchcv_amd import engine
    lb, L, ctx = _lib()
    dev = cuda_device
    code = CODE[dtype]
    for HW in GAP_HW:
        for C in GAP_C:
            N = GAP_N
            what = "global_avgpool {} N{} HW{} C{}".format(dtype, N, HW, C)
            x = rd(randn((N, HW, 1, C), 900 + HW + C) + 0.5, dtype)
            xd = x.to(dev, TDT[dtype])
            sq = torch.full((N, C), NAN, dtype=torch.float32, device=dev)
            lb.check(L.pcv_se_squeeze(ctx, _p(xd), _p(sq), N, HW, C, code, _stream()), ctx)
            flat32, y32 = guarded((N, 1, 1, C), torch.float32, dev)
            lb.check(L.pcv_global_avgpool(ctx, _p(xd), _p(y32), N, HW, C, code, 0, _stream()), ctx)
            flat, y = guarded((N, 1, 1, C), TDT[dtype], dev)
            lb.check(L.pcv_global_avgpool(ctx, _p(xd), _p(y), N, HW, C, code, code, _stream()), ctx)
            torch.cuda.synchronize()
            assert_guard(flat32, y32.numel(), what + " fp32 out")
            assert_guard(flat, y.numel(), what)
            assert_bits(y32.view(N, C), sq.cpu(), what + " against pcv_se_squeeze")
            ref, err = mean_ref(x)
            _check(y32.view(N, C).cpu(), ref, err, what + " fp32 out")
            _check(y.view(N, C).cpu(), ref, out_bound(ref, err, dtype), what)
            h = _handle(xd.view(N, HW, 1, C), C - 5)
            assert_bits(engine.global_avgpool(h, out_fp32=True).t, y32.cpu(), what + " (engine, fp32 out)")
            assert_bits(engine.global_avgpool(h, out_fp32=False).t, y.cpu(), what + " (engine)")


# ---- 10. BatchNorm + activation -----------------------------------------------------------------------------------------------------
BN_ACT_CASES = [(70, 8, 8), (527, 64, 64), (70, 32, 96)]                     # (rows, C, x_cpitch)
BN_RUNNER_C = 58


def bn_act_ref(x, scale, shift, act):
    """float64 act(x * scale[c] + shift[c]) and the bound of the kernel's fp32 error before the output rounding"""
    x, s, h = x.double(), scale.double(), shift.double()
    pre = x * s + h
    return act64(pre, act), act_err(pre, 2 * U32 * ((x * s).abs() + h.abs()), act)


def bn_act_operands(rows, C, xp, dtype, seed):
    """x [rows, xp] in the compute dtype whose channels >= C hold NaN (another tensor's channels in a concat buffer), scale, shift"""
    g = torch.Generator().manual_seed(seed)
    x = with_pads(torch.randn((rows, C), generator=g) * 2, xp, dtype)
    scale = torch.rand(C, generator=g) * 1.5 + 0.25
    scale[::3] *= -1
    shift = torch.randn(C, generator=g)
    return x, scale, shift


def _launch_bn_act(xd, sd, hd, rows, C, xp, act, dtype, what):
    lb, L, ctx = _lib()
    flat, y = guarded((rows, C), TDT[dtype], xd.device)
    lb.check(L.pcv_bn_act(ctx, _p(xd), _p(sd), _p(hd), _p(y), rows, C, xp, act, CODE[dtype], _stream()), ctx)
    torch.cuda.synchronize()
    assert_guard(flat, y.numel(), what)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_act_vs_float64_and_capped_grid(dtype, cuda_device):
    dev = cuda_device
    for i, (rows, C, xp) in enumerate(BN_ACT_CASES):
        x, scale, shift = bn_act_operands(rows, C, xp, dtype, 1000 + i)
        xd, sd, hd = x.to(dev), scale.to(dev), shift.to(dev)
        for act in range(7):
            what = "bn_act {} rows {} C {} x_cpitch {} act {}".format(dtype, rows, C, xp, act)
            y = _launch_bn_act(xd, sd, hd, rows, C, xp, act, dtype, what)
            ref, err = bn_act_ref(x[:, :C], scale, shift, act)
            _check(y.cpu(), ref, out_bound(ref, err, dtype), what)         # a NaN leaked from the other channels fails here
            for cap in (8, 1):                # 527 x 64 is 17 blocks of work: rounds on 8; one block walks every case in rounds
                with util.tuning(max_blocks=cap):
                    yc = _launch_bn_act(xd, sd, hd, rows, C, xp, act, dtype, what + " max_blocks={}".format(cap))
                assert_bits(yc, y.cpu(), what + " max_blocks={}".format(cap))


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_act_runner_pads_and_fold(dtype, cuda_device):
    """engine.BnActRunner.run with C = 58 on a cpitch-64 handle. The runner folds the BatchNorm with scale = shift = 0 in the six pad
    channels, so whatever finite values the input pads hold, the output pads are act(0) EXACTLY: 0 for none / relu / relu6 / swish /
    hswish and 0.5 for sigmoid / hsigmoid. That is intended (a consumer's packed weights are zero there); the test pins it."""
    from pytorchcv_amd import engine
    dev = cuda_device
    C, CP = BN_RUNNER_C, round8(BN_RUNNER_C)
    N, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(58)
    bn = nn.BatchNorm2d(C).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.5)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    stats = (bn.weight.detach().clone(), bn.bias.detach().clone(), bn.running_mean.clone(), bn.running_var.clone())
    bn = bn.to(dev)
    runner = engine.BnActRunner(bn)
    x = with_pads(torch.randn((N, H, W, C), generator=g) * 2, CP, dtype, fill=3.5)
    x[..., C + 1] = -2.0
    xd = x.to(dev)
    for act in range(7):
        what = "BnActRunner {} act {}".format(dtype, act)
        y = runner.run(_handle(xd, C), act)
        with util.tuning(max_blocks=8):
            y8 = runner.run(_handle(xd, C), act)
        with util.tuning(max_blocks=1):                                        # 560 chunks on one block: three rounds
            y1 = runner.run(_handle(xd, C), act)
        torch.cuda.synchronize()
        assert (y.C, y.cpitch) == (C, CP) and tuple(y.t.shape) == (N, H, W, CP) and y.dtype == TDT[dtype]
        assert_bits(y8.t, y.t.cpu(), what + " max_blocks=8")
        assert_bits(y1.t, y.t.cpu(), what + " max_blocks=1")
        # the operands the kernel read: the float64 fold to fp32 rounding in the logical channels, zero in the pads
        sc, sh = runner.scale.cpu(), runner.shift.cpu()
        s64, h64 = bn_fold64(stats, eps=bn.eps)
        assert bool(((sc[:C].double() - s64).abs() <= 4 * U32 * s64.abs()).all()), what
        assert bool(((sh[:C].double() - h64).abs() <= 2 * U32 * h64.abs() + 6 * U32 * (stats[2].double() * s64).abs()).all()), what
        assert bool((sc[C:] == 0).all()) and bool((sh[C:] == 0).all()), what
        ref, err = bn_act_ref(x[..., :C], sc[:C], sh[:C], act)
        out = y.t.cpu()
        _check(out[..., :C], ref, out_bound(ref, err, dtype), what)
        pad0 = 0.5 if act in (3, 5) else 0.0                                   # sigmoid (3) and hsigmoid (5): act(0) = 1 / 2
        assert pad0 == float(act64(torch.zeros((), dtype=torch.float64), act))
        assert bool((out[..., C:].double() == pad0).all()), "{}: pad channels are not act(0) = {}".format(what, pad0)


# ---- argument refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(dtype, cuda_device):
    """every entry point answers PCV_ERR_INVALID, with its name in the context's error text, and launches nothing"""
    lb, L, ctx = _lib()
    st = _stream()
    code = CODE[dtype]
    x = torch.zeros(1 << 14, dtype=TDT[dtype], device=cuda_device)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=cuda_device)
    flat, y = guarded((1 << 14,), TDT[dtype], cuda_device)
    flat32, y32 = guarded((1 << 14,), torch.float32, cuda_device)
    X, Y, Fp, Y32 = _p(x), _p(y), _p(f), _p(y32)

    def invalid(name, rc):
        with pytest.raises(lb.PcvError) as e:
            lb.check(rc, ctx)
        assert e.value.code == -1 and name in str(e.value), (name, str(e.value))

    n = "pcv_nchw_to_nhwc"
    invalid(n, L.pcv_nchw_to_nhwc(ctx, None, Y, 2, 3, 4, 5, 8, 5, code, st))
    invalid(n, L.pcv_nchw_to_nhwc(ctx, Fp, None, 2, 3, 4, 5, 8, 5, code, st))
    invalid(n, L.pcv_nchw_to_nhwc(ctx, Fp, Y, 2, 9, 4, 5, 8, 5, code, st))            # cpitch < C
    invalid(n, L.pcv_nchw_to_nhwc(ctx, Fp, Y, 2, 3, 4, 5, 8, 4, code, st))            # wpitch < W
    invalid(n, L.pcv_nchw_to_nhwc(ctx, Fp, Y, 2, 3, 4, 5, 6, 5, code, st))            # cpitch neither 4 nor a multiple of 8 (or of 4)
    if dtype != "fp32":
        invalid(n, L.pcv_nchw_to_nhwc(ctx, Fp, Y, 2, 9, 4, 5, 12, 5, code, st))       # cpitch % 4 is the fp32-only form
    n = "pcv_nhwc_to_nchw"
    invalid(n, L.pcv_nhwc_to_nchw(ctx, None, Y32, 2, 3, 4, 5, 8, code, st))
    invalid(n, L.pcv_nhwc_to_nchw(ctx, X, None, 2, 3, 4, 5, 8, code, st))
    invalid(n, L.pcv_nhwc_to_nchw(ctx, X, Y32, 2, 9, 4, 5, 8, code, st))              # cpitch < C
    n = "pcv_maxpool2d"
    invalid(n, L.pcv_maxpool2d(ctx, X, Y, 2, 8, 8, 12, 3, 2, 1, 0, code, st))         # C % 8
    invalid(n, L.pcv_maxpool2d(ctx, X, Y, 2, 8, 8, 16, 3, 2, 2, 0, code, st))         # 2 p > k
    invalid(n, L.pcv_maxpool2d(ctx, X, Y, 2, 8, 8, 16, 2, 2, 2, 1, code, st))
    invalid(n, L.pcv_maxpool2d(ctx, X, Y, 2, 2, 8, 16, 3, 2, 0, 0, code, st))         # empty pooled map: H = 2 under a 3-row window
    invalid(n, L.pcv_maxpool2d(ctx, X, Y, 2, 8, 4, 16, 5, 1, 0, 1, code, st))
    invalid(n, L.pcv_maxpool2d(ctx, None, Y, 2, 8, 8, 16, 3, 2, 1, 0, code, st))
    invalid(n, L.pcv_maxpool2d(ctx, X, None, 2, 8, 8, 16, 3, 2, 1, 0, code, st))
    n = "pcv_global_avgpool"
    invalid(n, L.pcv_global_avgpool(ctx, X, Y, 2, 49, 12, code, code, st))            # C % 8
    invalid(n, L.pcv_global_avgpool(ctx, None, Y, 2, 49, 16, code, code, st))
    invalid(n, L.pcv_global_avgpool(ctx, X, None, 2, 49, 16, code, code, st))
    invalid(n, L.pcv_global_avgpool(ctx, X, Y, 2, 49, 16, code, 2 if code == 1 else 1, st))   # neither the input's type nor fp32
    n = "pcv_channel_slice"
    invalid(n, L.pcv_channel_slice(ctx, X, Y, 70, 58, 58, 112, 64, code, st))         # x_cpitch < offset + C
    invalid(n, L.pcv_channel_slice(ctx, X, Y, 70, 58, 0, 64, 56, code, st))           # y_cpitch < C
    invalid(n, L.pcv_channel_slice(ctx, X, Y, 70, 58, 0, 64, 60, code, st))           # y_cpitch % 8
    invalid(n, L.pcv_channel_slice(ctx, X, Y, 70, 58, -8, 64, 64, code, st))
    invalid(n, L.pcv_channel_slice(ctx, None, Y, 70, 58, 0, 64, 64, code, st))
    invalid(n, L.pcv_channel_slice(ctx, X, None, 70, 58, 0, 64, 64, code, st))
    n = "pcv_channel_interleave2"
    invalid(n, L.pcv_channel_interleave2(ctx, X, X, Y, 70, 58, 64, 64, 112, code, st))    # y_cpitch < 2 Ch
    invalid(n, L.pcv_channel_interleave2(ctx, X, X, Y, 70, 58, 64, 64, 116, code, st))    # y_cpitch % 8
    invalid(n, L.pcv_channel_interleave2(ctx, X, X, Y, 70, 58, 56, 64, 120, code, st))    # a_cpitch < Ch
    invalid(n, L.pcv_channel_interleave2(ctx, X, X, Y, 70, 58, 64, 56, 120, code, st))    # b_cpitch < Ch
    invalid(n, L.pcv_channel_interleave2(ctx, None, X, Y, 70, 58, 64, 64, 120, code, st))
    invalid(n, L.pcv_channel_interleave2(ctx, X, None, Y, 70, 58, 64, 64, 120, code, st))
    invalid(n, L.pcv_channel_interleave2(ctx, X, X, None, 70, 58, 64, 64, 120, code, st))
    n = "pcv_channel_concat"
    invalid(n, L.pcv_channel_concat(ctx, X, Y, 70, 40, 40, 96, 12, code, st))         # offset % 8
    invalid(n, L.pcv_channel_concat(ctx, X, Y, 70, 36, 40, 96, 8, code, st))          # C % 8
    invalid(n, L.pcv_channel_concat(ctx, X, Y, 70, 40, 40, 96, 64, code, st))         # y_cpitch < offset + C
    invalid(n, L.pcv_channel_concat(ctx, X, Y, 70, 40, 32, 96, 8, code, st))          # x_cpitch < C
    invalid(n, L.pcv_channel_concat(ctx, None, Y, 70, 40, 40, 96, 8, code, st))
    invalid(n, L.pcv_channel_concat(ctx, X, None, 70, 40, 40, 96, 8, code, st))
    n = "pcv_interpolate"
    invalid(n, L.pcv_interpolate(ctx, X, Y, 2, 5, 6, 12, 10, 12, 1, 0, code, st))     # C % 8
    invalid(n, L.pcv_interpolate(ctx, X, Y, 2, 5, 6, 8, 0, 12, 1, 0, code, st))       # empty output
    invalid(n, L.pcv_interpolate(ctx, None, Y, 2, 5, 6, 8, 10, 12, 1, 0, code, st))
    invalid(n, L.pcv_interpolate(ctx, X, None, 2, 5, 6, 8, 10, 12, 0, 0, code, st))
    n = "pcv_bn_act"
    invalid(n, L.pcv_bn_act(ctx, X, Fp, Fp, Y, 70, 12, 16, 1, code, st))              # C % 8
    invalid(n, L.pcv_bn_act(ctx, X, Fp, Fp, Y, 70, 32, 24, 1, code, st))              # x_cpitch < C
    invalid(n, L.pcv_bn_act(ctx, X, Fp, Fp, Y, 70, 32, 36, 1, code, st))              # x_cpitch % 8
    invalid(n, L.pcv_bn_act(ctx, X, Fp, Fp, Y, 70, 32, 32, 7, code, st))              # no such activation
    invalid(n, L.pcv_bn_act(ctx, None, Fp, Fp, Y, 70, 32, 32, 1, code, st))
    invalid(n, L.pcv_bn_act(ctx, X, None, Fp, Y, 70, 32, 32, 1, code, st))
    invalid(n, L.pcv_bn_act(ctx, X, Fp, None, Y, 70, 32, 32, 1, code, st))
    invalid(n, L.pcv_bn_act(ctx, X, Fp, Fp, None, 70, 32, 32, 1, code, st))
    from pytorchcv_amd import engine
    with pytest.raises(RuntimeError, match="would be empty"):                           # the wrapper: H = 2 under a 3-row window
        engine.maxpool2d(_handle(x[:2 * 2 * 8 * 16].view(2, 2, 8, 16), 16), 3, 2, 0)
    torch.cuda.synchronize()
    for fl in (flat, flat32):                                                           # a refused call wrote nothing
        assert bool((bits(fl).cpu() == SENTINEL[fl.dtype]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_squeeze_excite_pool_fold_preprocess(dtype, cuda_device):
    """the same for the entry points test_refusals does not reach: pcv_se_squeeze / _excite / _scale, pcv_fc_f32, pcv_avgpool2d,
    pcv_global_avgpool's types, pcv_bn_fold and pcv_preprocess_u8"""
    lb, L, ctx = _lib()
    st = _stream()
    code = CODE[dtype]
    other = 2 if code == 1 else 1                      # a 16-bit type that is neither the input's nor fp32
    x = torch.zeros(1 << 14, dtype=TDT[dtype], device=cuda_device)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=cuda_device)
    u8 = torch.zeros(1 << 14, dtype=torch.uint8, device=cuda_device)
    flat, y = guarded((1 << 14,), TDT[dtype], cuda_device)
    flat32, y32 = guarded((1 << 14,), torch.float32, cuda_device)
    flat32b, z32 = guarded((1 << 14,), torch.float32, cuda_device)
    X, Y, Fp, Y32, Z32, U8 = _p(x), _p(y), _p(f), _p(y32), _p(z32), _p(u8)

    def invalid(name, rc):
        with pytest.raises(lb.PcvError) as e:
            lb.check(rc, ctx)
        assert e.value.code == -1 and name in str(e.value), (name, str(e.value))

    n = "pcv_se_squeeze"
    invalid(n, L.pcv_se_squeeze(ctx, None, Y32, 2, 49, 16, code, st))
    invalid(n, L.pcv_se_squeeze(ctx, X, None, 2, 49, 16, code, st))
    invalid(n, L.pcv_se_squeeze(ctx, X, Y32, 2, 49, 12, code, st))                    # C % 8
    invalid(n, L.pcv_se_squeeze(ctx, X, Y32, 2, 49, 16, 3, st))                       # no such dtype
    n = "pcv_se_excite"
    good = [Fp, Fp, Fp, Fp, Fp, Z32, Y32]                                             # mean, w1, b1, w2, b2, mid, gate
    for i in range(7):
        invalid(n, L.pcv_se_excite(ctx, *(good[:i] + [None] + good[i + 1:]), 2, 16, 4, 1, 3, st))
    invalid(n, L.pcv_se_excite(ctx, *good, 2, 16, 0, 1, 3, st))                       # M = 0
    n = "pcv_se_scale"
    invalid(n, L.pcv_se_scale(ctx, None, Fp, None, Y, 2, 49, 16, 0, code, st))
    invalid(n, L.pcv_se_scale(ctx, X, None, None, Y, 2, 49, 16, 0, code, st))
    invalid(n, L.pcv_se_scale(ctx, X, Fp, None, None, 2, 49, 16, 0, code, st))
    invalid(n, L.pcv_se_scale(ctx, X, Fp, None, Y, 2, 49, 12, 0, code, st))           # C % 8
    invalid(n, L.pcv_se_scale(ctx, X, Fp, None, Y, 2, 49, 16, 0, 3, st))              # no such dtype
    n = "pcv_fc_f32"
    good = [Fp, Fp, Fp, Y32]                                                          # in, w, b, out
    for i in range(4):
        invalid(n, L.pcv_fc_f32(ctx, *(good[:i] + [None] + good[i + 1:]), 2, 16, 4, 1, st))
    invalid(n, L.pcv_fc_f32(ctx, *good, 2, 0, 4, 1, st))                              # K = 0
    n = "pcv_avgpool2d"
    for Yo, oc in ((Y, code), (Y32, 0)):
        invalid(n, L.pcv_avgpool2d(ctx, None, Yo, 2, 8, 8, 16, 3, 2, code, oc, st))
        invalid(n, L.pcv_avgpool2d(ctx, X, None, 2, 8, 8, 16, 3, 2, code, oc, st))
        invalid(n, L.pcv_avgpool2d(ctx, X, Yo, 2, 8, 8, 12, 3, 2, code, oc, st))      # C % 8
        invalid(n, L.pcv_avgpool2d(ctx, X, Yo, 2, 2, 8, 16, 3, 1, code, oc, st))      # k > H
        invalid(n, L.pcv_avgpool2d(ctx, X, Yo, 2, 8, 2, 16, 3, 1, code, oc, st))      # k > W
    invalid(n, L.pcv_avgpool2d(ctx, X, Y, 2, 8, 8, 16, 3, 2, 3, 3, st))               # no such dtype
    invalid(n, L.pcv_avgpool2d(ctx, X, Y, 2, 8, 8, 16, 3, 2, code, other, st))        # neither the input's type nor fp32
    invalid(n, L.pcv_avgpool2d(ctx, X, Y, 2, 8, 8, 16, 8, 1, code, other, st))        # ... on the whole-map form as well
    n = "pcv_global_avgpool"
    invalid(n, L.pcv_global_avgpool(ctx, X, Y, 2, 49, 16, 3, 3, st))                  # no such dtype
    invalid(n, L.pcv_global_avgpool(ctx, X, Y, 2, 49, 16, code, 3, st))               # no such out_dtype
    invalid(n, L.pcv_global_avgpool(ctx, X, Y32, 2, 49, 12, code, 0, st))             # C % 8, fp32 out
    invalid(n, L.pcv_global_avgpool(ctx, None, Y32, 2, 49, 16, code, 0, st))
    invalid(n, L.pcv_global_avgpool(ctx, X, None, 2, 49, 16, code, 0, st))
    n = "pcv_bn_fold"
    invalid(n, L.pcv_bn_fold(ctx, 0, Fp, Fp, Fp, Fp, 1e-5, None, Y32, Z32, st))       # C <= 0
    invalid(n, L.pcv_bn_fold(ctx, -8, Fp, Fp, Fp, Fp, 1e-5, None, Y32, Z32, st))
    invalid(n, L.pcv_bn_fold(ctx, 16, Fp, Fp, Fp, Fp, 1e-5, None, None, Z32, st))
    invalid(n, L.pcv_bn_fold(ctx, 16, Fp, Fp, Fp, Fp, 1e-5, None, Y32, None, st))
    stats = [Fp, Fp, Fp, Fp]
    for i in range(4):                                                                # three of gamma / beta / mean / var
        invalid(n, L.pcv_bn_fold(ctx, 16, *(stats[:i] + [None] + stats[i + 1:]), 1e-5, Fp, Y32, Z32, st))
    n = "pcv_preprocess_u8"
    # (x, y, N, Hs, Ws, C, top, left, H, W, wpitch, mean, inv_std, dtype)
    invalid(n, L.pcv_preprocess_u8(ctx, None, Y, 2, 12, 14, 3, 1, 2, 8, 8, 8, Fp, Fp, code, st))
    invalid(n, L.pcv_preprocess_u8(ctx, U8, None, 2, 12, 14, 3, 1, 2, 8, 8, 8, Fp, Fp, code, st))
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, 1, 2, 8, 8, 8, None, Fp, code, st))
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, 1, 2, 8, 8, 8, Fp, None, code, st))
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, 5, 2, 8, 8, 8, Fp, Fp, code, st))     # top + H > Hs
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, 1, 7, 8, 8, 8, Fp, Fp, code, st))     # left + W > Ws
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, -1, 2, 8, 8, 8, Fp, Fp, code, st))    # top < 0
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 5, 1, 2, 8, 8, 8, Fp, Fp, code, st))     # C > 4
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, 1, 2, 8, 8, 6, Fp, Fp, code, st))     # wpitch < W
    invalid(n, L.pcv_preprocess_u8(ctx, U8, Y, 2, 12, 14, 3, 1, 2, 8, 8, 8, Fp, Fp, 3, st))        # no such dtype
    torch.cuda.synchronize()
    for fl in (flat, flat32, flat32b):                                                # a refused call wrote nothing
        assert bool((bits(fl).cpu() == SENTINEL[fl.dtype]).all())


def test_flat_grid_refusals(cuda_device):
    """a flat launch whose block count does not fit a 32-bit grid is refused with PCV_ERR_TOO_LARGE before anything is launched (such a
    call used to launch the count's low 32 bits: 2^32 blocks became a grid of 0). The pointers are never dereferenced."""
    lb, L, ctx = _lib()
    st = _stream()
    x = torch.zeros(1 << 10, dtype=torch.bfloat16, device=cuda_device)
    f = torch.zeros(1 << 10, dtype=torch.float32, device=cuda_device)
    flat, y = guarded((1 << 10,), torch.bfloat16, cuda_device)
    X, Y, Fp = _p(x), _p(y), _p(f)

    def too_large(name, rc):
        with pytest.raises(lb.PcvError) as e:
            lb.check(rc, ctx)
        assert e.value.code == lb.PCV_ERR_TOO_LARGE == -4 and name in str(e.value), (name, str(e.value))

    too_large("pcv_bn_act", L.pcv_bn_act(ctx, X, Fp, Fp, Y, 1 << 40, 8, 8, 1, 1, st))                   # 2^40 chunks: 2^32 blocks
    too_large("pcv_channel_slice", L.pcv_channel_slice(ctx, X, Y, 1 << 40, 8, 0, 8, 8, 1, st))
    too_large("pcv_maxpool2d", L.pcv_maxpool2d(ctx, X, Y, 2 ** 31 - 1, 4096, 4096, 8, 1, 1, 0, 0, 1, st))
    torch.cuda.synchronize()
    assert bool((bits(flat).cpu() == SENTINEL[flat.dtype]).all())
