"""
GPU sweep of the depthwise kernels (csrc/dwconv.hpp: 3x3 register window, 5x5 row streaming; stride 1 / 2; the clamp-only FAST
build and the general-activation build; fp32 / bf16 / fp16 = 24 instances behind pcv_dwconv2d_fused) and of the SE kernels
(csrc/aux_kernels.hpp: spatial_mean_kernel, se_fc_kernel, se_scale_kernel behind pcv_se_squeeze / pcv_se_excite / pcv_fc_f32 /
pcv_se_scale / engine.se_forward) against float64 restatements, plus the bit-for-bit invariances of both families.

The operands are exactly what the kernels read: x in the compute dtype, the taps from the runner's packed blob, the runner's folded
fp32 scale / shift (each checked on its own against round_dtype(weight) and a float64 BN fold). Only the kernel's fp32 arithmetic
and the output rounding can then separate it from the reference. u = 2^-24 (fp32 unit roundoff); U = 2^-8 (bf16) / 2^-11 (fp16) /
0 (fp32), the output rounding.

Bounds (derived, first order in u; written here on purpose):
  depthwise : pre = scale * sum_k x_k w_k + shift is one product and KK - 1 fused multiply-adds (KK = 9 / 25), then one fma with
              scale and shift: |e_pre| <= (KK + 1) u (|scale| sum_k |x_k||w_k| + |shift|).
              act: e_a = L_act e_pre + T_act(pre); residual add: e_r = e_a + u (|a| + |res|); post_act: e_y = L_post e_r + T_post(r).
              |y - ref| <= U |ref| + (1 + U) e_y + F
  activations: Lipschitz constants L = 1 (none / relu / relu6), 1/4 (sigmoid), 1.1 (swish), 1/6 (hsigmoid), 3/2 (hswish).
              T = 0 for the clamps; for sigmoid / swish / hsigmoid / hswish T(v) = 4 u (1 + |v|)^2: __expf evaluates 2^(v log2 e)
              (the rounded argument is off by |v| u relative, a few ulp in v_exp_f32 / v_rcp_f32), swish multiplies that by |v|,
              the hard forms round two products and the constant 1/6.
  F         : 2^-25 for fp16 (half the subnormal spacing: tiny results round absolutely), 0 otherwise.
  squeeze   : any order of summing HW terms, then the rounded 1/HW and the product: |e| <= (HW + 1) u mean|x|.
  fc layer  : act(b + sum_k W x_k) in any bracketing of K + 1 terms (fma chains per K partition, partials added to the bias):
              |e_pre| <= sum_k |W| e_x + (K + 1) u (|b| + sum_k |W||x|); then the activation as above (e_x = 0 on the kernel's
              own input; end to end e_x is the previous stage's bound).
  se scale  : y = post(x g + res): e = |x| e_g + 2 u (|x g| + |res|), post_act as above, output rounding as above.
The bounds are not fitted to observed errors; tests/test_dw_se_bounds.py checks on the CPU that plausible bugs (a dropped tap, a
window shifted by one row or column, rows duplicated across a strip boundary, another image's gate, the mid activation skipped)
violate them.
"""

import ctypes
import math
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import util

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
U32 = 2.0 ** -24
ULP = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
FLOOR = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}
NONE, RELU, RELU6, SIGMOID, SWISH, HSIGMOID, HSWISH = range(7)
LIP = {NONE: 1.0, RELU: 1.0, RELU6: 1.0, SIGMOID: 0.25, SWISH: 1.1, HSIGMOID: 1.0 / 6.0, HSWISH: 1.5}
FAST_CODES = (NONE, RELU, RELU6)
GENERAL_CODES = (SIGMOID, SWISH, HSIGMOID, HSWISH)


# ---- float64 references and bounds (shared with the CPU checks of tests/test_dw_se_bounds.py) ----------------------------------
def act64(v, code):
    if code == RELU:
        return v.clamp(min=0)
    if code == RELU6:
        return v.clamp(0, 6)
    if code == SIGMOID:
        return torch.sigmoid(v)
    if code == SWISH:
        return v * torch.sigmoid(v)
    if code == HSIGMOID:
        return (v + 3).clamp(0, 6) / 6
    if code == HSWISH:
        return v * (v + 3).clamp(0, 6) / 6
    return v


def act_err(v, e, code):
    """bound on |act(v') - act(v)| for |v' - v| <= e, with the activation evaluated in fp32"""
    out = LIP[code] * e
    if code >= SIGMOID:
        out = out + 4 * U32 * (1 + v.abs()) ** 2
    return out


def out_bound(ref, err, dtype):
    return ULP[dtype] * ref.abs() + (1 + ULP[dtype]) * err + FLOOR[dtype]


def dw_out_hw(H, W, ks, s, pad4):
    l, r, t, b = pad4
    return (H + t + b - ks) // s + 1, (W + l + r - ks) // s + 1


def dw_ref(x, taps, scale, shift, ks, s, pad4, act, res=None, post=NONE):
    """float64 post_act(act(scale * dwconv(x) + shift) + res) on NHWC x; taps [ks*ks][C]; pad4 = (left, right, top, bottom).
    Returns (reference, bound of the kernel's fp32 error before the output rounding)."""
    x = x.double()
    w = taps.double().view(ks, ks, -1)
    l, r, t, b = pad4
    xp = F.pad(x, (0, 0, l, r, t, b))
    Ho, Wo = (xp.shape[1] - ks) // s + 1, (xp.shape[2] - ks) // s + 1
    z = torch.zeros((x.shape[0], Ho, Wo, x.shape[3]), dtype=torch.float64, device=x.device)
    m = torch.zeros_like(z)
    for dy in range(ks):
        for dx in range(ks):
            win = xp[:, dy:dy + s * (Ho - 1) + 1:s, dx:dx + s * (Wo - 1) + 1:s, :]
            z = z + win * w[dy, dx]
            m = m + win.abs() * w[dy, dx].abs()
    sc, sh = scale.double(), shift.double()
    pre = sc * z + sh
    err = (ks * ks + 1) * U32 * (sc.abs() * m + sh.abs())
    a = act64(pre, act)
    err = act_err(pre, err, act)
    v = a
    if res is not None:
        v = a + res.double()
        err = err + U32 * (a.abs() + res.double().abs())
    y = act64(v, post)
    if post != NONE:
        err = act_err(v, err, post)
    return y, err


def fc_ref(x, w, b, act, e_x=None):
    """float64 act(b + x W^T) on x [N][K], W [J][K]; (reference, pre-activation, bound of the fp32 error)"""
    x, w, b = x.double(), w.double(), b.double()
    pre = x @ w.t() + b
    K = w.shape[1]
    err = (K + 1) * U32 * (x.abs() @ w.abs().t() + b.abs())
    if e_x is not None:
        err = err + e_x @ w.abs().t()
    return act64(pre, act), pre, act_err(pre, err, act)


def mean_ref(x):
    """float64 spatial mean of NHWC x, per (n, c), and the fp32-summation bound (HW + 1) u mean|x|"""
    x = x.double()
    HW = x.shape[1] * x.shape[2]
    return x.mean(dim=(1, 2)), (HW + 1) * U32 * x.abs().mean(dim=(1, 2))


def scale_ref(x, g, res, post, e_g=None):
    """float64 post(x * gate[n, c] + res) on NHWC x, gate [N][C]; (reference, fp32 error bound before the output rounding)"""
    x = x.double()
    g = g.double()[:, None, None, :]
    v = x * g
    cond = v.abs()
    if res is not None:
        v = v + res.double()
        cond = cond + res.double().abs()
    err = 2 * U32 * cond
    if e_g is not None:
        err = err + x.abs() * e_g.double()[:, None, None, :]
    y = act64(v, post)
    if post != NONE:
        err = act_err(v, err, post)
    return y, err


# ---- depthwise operands -----------------------------------------------------------------------------------------------------
def dw_operands(N, H, W, C, ks, dtype, seed, Ho=None, Wo=None, with_res=False):
    """x (rounded to the compute dtype), the fp32 conv weight [C, 1, ks, ks], BN (gamma, beta, mean, var) and the residual"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, C), generator=g).to(TDT[dtype]).float()
    w = torch.randn((C, 1, ks, ks), generator=g) * (1.5 / ks)
    gamma = torch.rand(C, generator=g) * 1.5 + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    mean = torch.randn(C, generator=g) * 0.3
    var = torch.rand(C, generator=g) * 1.5 + 0.5
    res = torch.randn((N, Ho, Wo, C), generator=g).to(TDT[dtype]).float() if with_res else None
    return x, w, (gamma, beta, mean, var), res


def bn_fold64(bn, eps=1e-5):
    gamma, beta, mean, var = [t.double() for t in bn]
    s = gamma / torch.sqrt(var + eps)
    return s, beta - mean * s


def taps_of(w, dtype):
    """[ks*ks][C] taps of a depthwise weight [C, 1, ks, ks], rounded to the storage type (what pcv_dwconv_pack writes)"""
    C = w.shape[0]
    return w.reshape(C, -1).t().contiguous().to(TDT[dtype]).float()


# ---- the depthwise table -------------------------------------------------------------------------------------------------------
# (N, H, W, C, pad4) per (kernel size, stride); pad4 = (left, right, top, bottom). Symmetric padding is ks // 2.
_DW_SHAPES = {
    (3, 1): [(1, 112, 112, 32, None), (3, 56, 56, 144, None), (5, 14, 14, 672, None), (3, 7, 7, 1024, None),
             (3, 57, 31, 40, None), (5, 15, 15, 8, None), (3, 1, 1, 16, None), (1, 2, 3, 24, None), (3, 16, 12, 48, (1, 2, 1, 2)),
             (2, 9, 10, 56, (2, 0, 0, 2))],
    (3, 2): [(1, 112, 112, 32, None), (3, 56, 56, 144, (0, 1, 0, 1)), (2, 113, 111, 24, None), (5, 15, 15, 8, None),
             (3, 14, 14, 672, (0, 1, 0, 1)), (3, 7, 7, 960, None), (1, 1, 1, 16, None), (3, 2, 3, 24, None),
             (2, 16, 12, 40, (1, 2, 1, 2))],
    (5, 1): [(1, 112, 112, 32, None), (3, 28, 28, 240, None), (2, 14, 14, 672, None), (3, 7, 7, 960, None),
             (3, 57, 31, 40, None), (5, 15, 15, 8, None), (3, 4, 3, 16, None), (1, 2, 3, 24, None), (1, 1, 1, 8, None),
             (2, 12, 10, 48, (1, 3, 3, 1))],
    (5, 2): [(2, 112, 112, 32, (1, 2, 1, 2)), (3, 56, 56, 144, None), (2, 113, 111, 24, None), (5, 15, 15, 8, None),
             (3, 14, 14, 672, (1, 2, 1, 2)), (3, 7, 7, 1024, None), (3, 4, 3, 16, None), (1, 2, 3, 24, None),
             (1, 1, 1, 8, None)],
}


def dw_cases(ks, s, fast):
    """(N, H, W, C, pad4, act, post_act, with_res) of one (kernel size, stride, FAST) class: every shape once with each act of
    the class in turn, stride-1 shapes once more with a residual and a post_act of the class (the general class also with a
    clamp act behind which a general post_act forces that instance)."""
    codes = FAST_CODES if fast else GENERAL_CODES
    out = []
    for i, (N, H, W, C, pad4) in enumerate(_DW_SHAPES[(ks, s)]):
        pad4 = pad4 if pad4 is not None else (ks // 2,) * 4
        out.append((N, H, W, C, pad4, codes[i % len(codes)], NONE, False))
        if s == 1:
            post = codes[(i + 1) % len(codes)]
            act = codes[(i + 2) % len(codes)] if fast or i % 2 == 0 else (RELU, RELU6)[i % 4 // 2]
            out.append((N, H, W, C, pad4, act, post, True))
    return out


def is_fast(act, post):
    """the FAST index of the kDw table (pcv_dwconv2d_fused, csrc/pcv_api.hip): both activations clamps -> the FAST build"""
    return act <= RELU6 and post <= RELU6


DW_INSTANCES = [(ks, s, fast, dt) for ks in (3, 5) for s in (1, 2) for fast in (True, False) for dt in ("fp32", "bf16", "fp16")]


def _iid(p):
    ks, s, fast, dt = p
    return "{}x{}_s{}_{}_{}".format(ks, ks, s, "fast" if fast else "general", dt)


# ---- launching ----------------------------------------------------------------------------------------------------------------
def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


class DwLayer(object):
    """a depthwise Conv2d + BatchNorm2d on the device and its ConvRunner (the runner packs the taps and folds the BN)"""
    def __init__(self, w, bn, ks, s, dev):
        from pytorchcv_amd import engine
        C = w.shape[0]
        self.conv = nn.Conv2d(C, C, ks, s, ks // 2, groups=C, bias=False)
        self.bn = nn.BatchNorm2d(C)
        with torch.no_grad():
            self.conv.weight.copy_(w)
            self.bn.weight.copy_(bn[0])
            self.bn.bias.copy_(bn[1])
            self.bn.running_mean.copy_(bn[2])
            self.bn.running_var.copy_(bn[3])
        self.conv.eval().to(dev)
        self.bn.eval().to(dev)
        self.runner = engine.ConvRunner(self.conv, self.bn)
        self.ks, self.C = ks, C

    def prepare(self, x, act, post, has_res, pad4, dtype):
        from pytorchcv_amd import engine
        N, H, W, C = x.shape
        xh = engine.NHWC(x, N, H, W, C)
        d = self.runner.desc(xh, act, post, has_res, pad4=pad4)
        self.runner.prepare(xh, d)
        return d

    def taps(self, dtype):
        n = self.ks * self.ks * self.C
        es = torch.tensor([], dtype=TDT[dtype]).element_size()
        return self.runner.packed[:n * es].view(TDT[dtype]).view(self.ks * self.ks, self.C)

    def launch(self, x, act, post, pad4, dtype, res=None):
        """pcv_dwconv2d_fused through ctypes into a NaN-filled output: an element no thread writes stays NaN"""
        lb, L, ctx = _lib()
        d = self.prepare(x, act, post, res is not None, pad4, dtype)
        Ho, Wo = dw_out_hw(x.shape[1], x.shape[2], self.ks, d.stride_h, pad4)
        y = torch.full((x.shape[0], Ho, Wo, self.C), float("nan"), dtype=TDT[dtype], device=x.device)
        lb.check(L.pcv_dwconv2d_fused(ctx, ctypes.byref(d), _p(x), _p(self.runner.packed), _p(self.runner.scale),
                                      _p(self.runner.shift), _p(res), _p(y), _stream()), ctx)
        return y


def _check(out, ref, bound, what):
    err = (out.double() - ref).abs()
    bad = ~(err <= bound)                      # NaN (an element nobody wrote) counts as a failure
    if bool(bad.any()):
        i = int(torch.where(bad.flatten())[0][0])
        pytest.fail("{}: {} of {} elements out of bound; first at flat index {}: got {:.6e}, ref {:.6e}, bound {:.3e}".format(
            what, int(bad.sum()), bad.numel(), i, float(out.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


# ---- 1. depthwise vs float64, per kernel instance ---------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", DW_INSTANCES, ids=[_iid(p) for p in DW_INSTANCES])
def test_depthwise_instance_vs_float64(inst, cuda_device):
    from pytorchcv_amd import engine
    ks, s, fast, dtype = inst
    dev = cuda_device
    quiet = engine.fp16_overflow_count(dev)
    ran = 0
    for i, (N, H, W, C, pad4, act, post, with_res) in enumerate(dw_cases(ks, s, fast)):
        assert is_fast(act, post) == fast
        what = "{}x{} s{} {} N{} {}x{}x{} pad{} act{} post{} res{}".format(ks, ks, s, dtype, N, H, W, C, pad4, act, post, with_res)
        Ho, Wo = dw_out_hw(H, W, ks, s, pad4)
        x, w, bn, res = dw_operands(N, H, W, C, ks, dtype, seed=1000 * ks + 100 * s + i, Ho=Ho, Wo=Wo, with_res=with_res)
        layer = DwLayer(w, bn, ks, s, dev)
        xd = x.to(dev, TDT[dtype])
        rd = res.to(dev, TDT[dtype]) if res is not None else None
        y = layer.launch(xd, act, post, pad4, dtype, rd)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (N, Ho, Wo, C)
        # the operands the kernel read: taps = round_dtype(weight) exactly; scale / shift = the float64 fold to fp32 rounding
        taps = layer.taps(dtype).float()
        assert torch.equal(taps.cpu(), taps_of(w, dtype)), what
        s64, h64 = bn_fold64(bn)
        sc, sh = layer.runner.scale.cpu().double(), layer.runner.shift.cpu().double()
        assert bool(((sc - s64).abs() <= 4 * U32 * s64.abs()).all()), what
        assert bool(((sh - h64).abs() <= 2 * U32 * h64.abs() + 6 * U32 * (bn[2].double() * s64).abs()).all()), what
        ref, err = dw_ref(xd, taps, layer.runner.scale, layer.runner.shift, ks, s, pad4, act, rd, post)
        _check(y, ref, out_bound(ref, err, dtype), what)
        ran += 1
    assert ran >= 9
    assert engine.fp16_overflow_count(dev) == quiet          # in-range data is not counted


# ---- 2. depthwise invariances, bit for bit --------------------------------------------------------------------------------------
_INV_SHAPES = {(3, 1): [(2, 15, 13, 40), (3, 10, 7, 16)], (3, 2): [(2, 29, 13, 40), (3, 19, 7, 16)],
               (5, 1): [(2, 15, 13, 40), (3, 10, 7, 16)], (5, 2): [(2, 29, 13, 40), (3, 19, 7, 16)]}


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("ks,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_strip_split_and_flags_keep_their_bits(ks, s, dtype, cuda_device):
    """Rows per thread dw_th in {1 .. 7, Ho - 1, Ho} (strips shorter than the 3-row prefetch ring, strips that do not divide Ho,
    one strip) and dw_flags 0 .. 3 (non-temporal stores, dispatch-order blocks): the same bits as the automatic split."""
    dev = cuda_device
    for i, (N, H, W, C) in enumerate(_INV_SHAPES[(ks, s)]):
        pad4 = (ks // 2,) * 4
        Ho, Wo = dw_out_hw(H, W, ks, s, pad4)
        act, post, with_res = ((RELU6, NONE, False), (SWISH, HSWISH, s == 1))[i]
        x, w, bn, res = dw_operands(N, H, W, C, ks, dtype, seed=7000 + 10 * ks + s + i, Ho=Ho, Wo=Wo, with_res=with_res)
        layer = DwLayer(w, bn, ks, s, dev)
        xd = x.to(dev, TDT[dtype])
        rd = res.to(dev, TDT[dtype]) if res is not None else None
        y0 = layer.launch(xd, act, post, pad4, dtype, rd)
        ref, err = dw_ref(xd, layer.taps(dtype).float(), layer.runner.scale, layer.runner.shift, ks, s, pad4, act, rd, post)
        _check(y0, ref, out_bound(ref, err, dtype), "default split")
        for th in sorted({1, 2, 3, 4, 5, 6, 7, Ho - 1, Ho} - {0}):
            with util.tuning(dw_th=th):
                y = layer.launch(xd, act, post, pad4, dtype, rd)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "dw_th={} on {}x{}x{} (Ho {})".format(th, H, W, C, Ho)
        for flags in (1, 2, 3):
            with util.tuning(dw_flags=flags):
                y = layer.launch(xd, act, post, pad4, dtype, rd)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "dw_flags={} on {}x{}x{}".format(flags, H, W, C)


def _auto_th(N, Ho, Wo, C8, num_cu):
    """rows per thread the host picks (pcv_dwconv2d_fused) - only to check that the shapes below do change it"""
    cols = N * Wo * C8
    nseg = max(1, (num_cu * 64 * 16 + cols - 1) // cols)
    th = (Ho + nseg - 1) // nseg
    return th if th >= 4 else min(Ho, 4)


_POS_SHAPES = {(3, 1): (112, 112, 96), (3, 2): (112, 112, 384), (5, 1): (56, 56, 192), (5, 2): (112, 112, 192)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("ks,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_batch_position_keeps_its_bits(ks, s, dtype, cuda_device):
    """One image alone and at positions 0, 4 and 8 of a batch of 9 (where the automatic strip height differs): same bits."""
    dev = cuda_device
    H, W, C = _POS_SHAPES[(ks, s)]
    pad4 = (ks // 2,) * 4
    Ho, Wo = dw_out_hw(H, W, ks, s, pad4)
    C8 = C // (4 if ks == 5 else 8)
    num_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert _auto_th(1, Ho, Wo, C8, num_cu) != _auto_th(9, Ho, Wo, C8, num_cu)
    x, w, bn, _ = dw_operands(9, H, W, C, ks, dtype, seed=9000 + 10 * ks + s)
    layer = DwLayer(w, bn, ks, s, dev)
    xd = x.to(dev, TDT[dtype])
    img = xd[3:4].clone()
    for p in (0, 4, 8):
        xd[p] = img[0]
    for act, post in ((RELU, NONE), (HSWISH, RELU)):
        alone = layer.launch(img, act, post, pad4, dtype)
        batch = layer.launch(xd, act, post, pad4, dtype)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(alone.float()).all())
        for p in (0, 4, 8):
            assert torch.equal(batch[p], alone[0]), "position {} act {} post {}".format(p, act, post)


# ---- 3. SE and fc vs float64 ----------------------------------------------------------------------------------------------------
_SQ_HW = (1, 49, 196, 3136, 12544)
_SQ_C = (8, 72, 120, 1280, 2048, 4104, 8192)


def test_se_squeeze_vs_float64(cuda_device):
    """spatial_mean_kernel: idle rows (512 % Gc != 0: C = 72, 120, 1280), Gc < 512, a second channel group (C = 4104, 8192)."""
    lb, L, ctx = _lib()
    dev = cuda_device
    dts = ("fp32", "bf16", "fp16")
    k = 0
    for HW in _SQ_HW:
        for C in _SQ_C:
            big = HW * C > (1 << 22)
            for dtype in (dts[k % 3],) if big else dts:
                k += 1
                N = 1 if HW * C > (1 << 24) else 2 if big else 3
                gen = torch.Generator(device=dev).manual_seed(HW + C + k)
                x = (torch.randn((N, HW, 1, C), generator=gen, device=dev) + 0.5).to(TDT[dtype])
                m = torch.full((N, C), float("nan"), dtype=torch.float32, device=dev)
                lb.check(L.pcv_se_squeeze(ctx, _p(x), _p(m), N, HW, C, CODE[dtype], _stream()), ctx)
                ref, err = mean_ref(x)
                _check(m, ref, err, "squeeze {} N{} HW{} C{}".format(dtype, N, HW, C))
                del x


# (N, C, M, mid_act, out_act): N covers 1, 7, 8, 9, 17 (empty image slots); C = 16, 72 (one K chunk), 1024 (exactly one),
# 1032 (one + a tail of 8), 2048 (two); M = 18 puts the second layer on the scalar K % 4 path, small M shrinks TJ;
# the acts cover all seven codes on both layers, with the nets' pairs relu / sigmoid, relu / hsigmoid, swish / sigmoid
_EXCITE = [(1, 16, 8, RELU, SIGMOID), (7, 72, 18, RELU, HSIGMOID), (8, 1024, 20, SWISH, SIGMOID), (9, 1032, 120, NONE, HSWISH),
           (17, 2048, 512, RELU6, SWISH), (17, 72, 8, SIGMOID, NONE), (9, 16, 18, HSIGMOID, RELU6), (8, 1032, 512, HSWISH, RELU),
           (7, 2048, 120, RELU, SIGMOID), (1, 1024, 18, SWISH, HSIGMOID), (17, 1032, 20, RELU, HSIGMOID), (8, 72, 120, SWISH, SIGMOID)]


def se_mlp(C, M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, C, generator=g) * (1.5 / math.sqrt(C)), torch.randn(M, generator=g) * 0.5,
            torch.randn(C, M, generator=g) * (1.5 / math.sqrt(M)), torch.randn(C, generator=g) * 0.5)


@pytest.mark.parametrize("case", _EXCITE, ids=["n{}_c{}_m{}_a{}{}".format(*c) for c in _EXCITE])
def test_se_excite_vs_float64(case, cuda_device):
    lb, L, ctx = _lib()
    dev = cuda_device
    N, C, M, ma, oa = case
    g = torch.Generator().manual_seed(N * 10000 + C + M)
    mean = torch.randn(N, C, generator=g)
    w1, b1, w2, b2 = [t.to(dev).contiguous() for t in se_mlp(C, M, C + M)]
    md = mean.to(dev)
    mid = torch.full((N, M), float("nan"), device=dev)
    gate = torch.full((N, C), float("nan"), device=dev)
    lb.check(L.pcv_se_excite(ctx, _p(md), _p(w1), _p(b1), _p(w2), _p(b2), _p(mid), _p(gate), N, C, M, ma, oa, _stream()), ctx)
    torch.cuda.synchronize()
    r_mid, _, e_mid = fc_ref(md, w1, b1, ma)
    _check(mid, r_mid, e_mid, "mid (layer 1)")
    r_gate, _, e_gate = fc_ref(mid, w2, b2, oa)                  # layer 2 on the kernel's own mid
    _check(gate, r_gate, e_gate, "gate (layer 2 on the kernel's mid)")
    r_end, _, e_end = fc_ref(r_mid, w2, b2, oa, e_x=e_mid)      # end to end
    _check(gate, r_end, e_end, "gate (end to end)")


_FC = [(K, J) for K in (1000, 1001, 2048, 2050) for J in (1, 8, 1000)]


def test_fc_f32_vs_float64(cuda_device):
    """pcv_fc_f32 (the SE layers of a folded squeezed-excite convolution, and the K-chunk / scalar / TJ paths of se_fc_kernel)."""
    lb, L, ctx = _lib()
    dev = cuda_device
    for i, (K, J) in enumerate(_FC):
        N = (1, 5, 8, 13, 17)[i % 5]
        act = i % 7
        g = torch.Generator().manual_seed(K * 7 + J)
        x = torch.randn(N, K, generator=g).to(dev)
        w = (torch.randn(J, K, generator=g) * (1.5 / math.sqrt(K))).to(dev)
        b = (torch.randn(J, generator=g) * 0.5).to(dev)
        y = torch.full((N, J), float("nan"), device=dev)
        lb.check(L.pcv_fc_f32(ctx, _p(x), _p(w), _p(b), _p(y), N, K, J, act, _stream()), ctx)
        torch.cuda.synchronize()
        ref, _, err = fc_ref(x, w, b, act)
        _check(y, ref, err, "fc N{} K{} J{} act{}".format(N, K, J, act))


def _launch_scale(x, gate, res, post, dtype):
    lb, L, ctx = _lib()
    N, H, W, C = x.shape
    y = torch.full_like(x, float("nan"))
    lb.check(L.pcv_se_scale(ctx, _p(x), _p(gate), _p(res), _p(y), N, H * W, C, post, CODE[dtype], _stream()), ctx)
    return y


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_se_scale_vs_float64_and_capped_grid(dtype, cuda_device):
    """every post_act, with and without a residual; under max_blocks=3 (grid-stride rounds) the same bits"""
    from pytorchcv_amd import engine
    dev = cuda_device
    quiet = engine.fp16_overflow_count(dev)
    for (N, H, W, C) in ((3, 7, 7, 72), (2, 14, 13, 1032), (5, 1, 1, 8)):
        g = torch.Generator().manual_seed(N + H + C)
        x = torch.randn((N, H, W, C), generator=g).to(dev, TDT[dtype])
        res = torch.randn((N, H, W, C), generator=g).to(dev, TDT[dtype])
        gate = torch.rand((N, C), generator=g).to(dev) * 2 - 0.5
        for post in range(7):
            for r in (None, res):
                y = _launch_scale(x, gate, r, post, dtype)
                torch.cuda.synchronize()
                ref, err = scale_ref(x, gate, r, post)
                _check(y, ref, out_bound(ref, err, dtype), "se_scale {}x{}x{}x{} post{} res{}".format(N, H, W, C, post, r is not None))
                with util.tuning(max_blocks=3):
                    y3 = _launch_scale(x, gate, r, post, dtype)
                torch.cuda.synchronize()
                assert torch.equal(y, y3), (N, H, W, C, post)
    assert engine.fp16_overflow_count(dev) == quiet


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_se_forward_end_to_end_vs_float64(dtype, cuda_device):
    """engine.se_forward (squeeze -> excite -> scale) with logical C not a multiple of 8: the pad channels come out post_act(0)"""
    from pytorchcv_amd import engine
    dev = cuda_device
    quiet = engine.fp16_overflow_count(dev)
    for i, (N, H, W, C, M, ma, oa) in enumerate([(3, 7, 7, 20, 8, RELU, SIGMOID), (2, 14, 14, 60, 16, RELU, HSIGMOID),
                                                 (5, 5, 6, 72, 18, SWISH, SIGMOID), (17, 3, 3, 44, 20, HSWISH, HSIGMOID)]):
        CP = (C + 7) // 8 * 8
        g = torch.Generator().manual_seed(500 + i)
        x = torch.zeros((N, H, W, CP))
        x[..., :C] = torch.randn((N, H, W, C), generator=g)
        res = torch.zeros((N, H, W, CP))
        res[..., :C] = torch.randn((N, H, W, C), generator=g)
        x = x.to(dev, TDT[dtype])
        res = res.to(dev, TDT[dtype])
        w1, b1, w2, b2 = [t.to(dev).contiguous() for t in se_mlp(C, M, 600 + i)]
        for post in range(7):
            r = res if post % 2 == 0 else None
            xh = engine.NHWC(x, N, H, W, C, cpitch=CP)
            rh = engine.NHWC(r, N, H, W, C, cpitch=CP) if r is not None else None
            y = engine.se_forward(xh, w1, b1, w2, b2, ma, oa, rh, post)
            with util.tuning(max_blocks=3):
                y3 = engine.se_forward(xh, w1, b1, w2, b2, ma, oa, rh, post)
            torch.cuda.synchronize()
            assert y.C == C and y.cpitch == CP and tuple(y.t.shape) == (N, H, W, CP)
            assert torch.equal(y.t, y3.t)
            m, e_m = mean_ref(x[..., :C])
            mid, _, e_mid = fc_ref(m, w1, b1, ma, e_x=e_m)
            gate, _, e_g = fc_ref(mid, w2, b2, oa, e_x=e_mid)
            ref, err = scale_ref(x[..., :C], gate, r[..., :C] if r is not None else None, post, e_g=e_g)
            _check(y.t[..., :C], ref, out_bound(ref, err, dtype), "se_forward C{} post{}".format(C, post))
            pad = y.t[..., C:].double()
            assert bool((pad == float(act64(torch.zeros((), dtype=torch.float64), post))).all()), "pad channels, post {}".format(post)
    assert engine.fp16_overflow_count(dev) == quiet


@pytest.mark.parametrize("C,M", [(1032, 18), (72, 20), (2048, 8)])
def test_se_excite_batch_position_keeps_its_bits(C, M, cuda_device):
    """Row i of mid and gate is the same bits alone and at positions 0, 6, 7, 8, 15, 16 of a batch of 17 (se_fc_kernel's 8-image
    slots once rounded slot pairs differently: a 1-ulp batch-position dependence)."""
    lb, L, ctx = _lib()
    dev = cuda_device
    g = torch.Generator().manual_seed(C * M)
    batch = torch.randn(17, C, generator=g)
    row = batch[3].clone()
    pos = (0, 6, 7, 8, 15, 16)
    for p in pos:
        batch[p] = row
    w1, b1, w2, b2 = [t.to(dev).contiguous() for t in se_mlp(C, M, C + 3 * M)]

    def excite(mean):
        n = mean.shape[0]
        mid = torch.empty((n, M), device=dev)
        gate = torch.empty((n, C), device=dev)
        md = mean.to(dev).contiguous()
        lb.check(L.pcv_se_excite(ctx, _p(md), _p(w1), _p(b1), _p(w2), _p(b2), _p(mid), _p(gate), n, C, M, RELU, SIGMOID,
                                 _stream()), ctx)
        f = torch.empty((n, M), device=dev)
        lb.check(L.pcv_fc_f32(ctx, _p(md), _p(w1), _p(b1), _p(f), n, C, M, SWISH, _stream()), ctx)
        torch.cuda.synchronize()
        return mid, gate, f
    m1, g1, f1 = excite(row[None])
    mb, gb, fb = excite(batch)
    for p in pos:
        assert torch.equal(mb[p], m1[0]) and torch.equal(gb[p], g1[0]) and torch.equal(fb[p], f1[0]), "position {}".format(p)
