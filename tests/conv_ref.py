"""
Float64 reference and first-order error bound of one fused convolution launch (plain module: CPU only, nothing of the GPU side is
imported), shared by tests/test_gpu_conv_sweep.py (the kernels) and tests/test_conv_ref_bounds.py (the CPU proof that the bound
is sound and tight enough to fail).

    y = post_act( act( scale * conv(x, w) + shift ) * gate + res )

conv_ref is an explicit loop over the (r, q) filter taps: a strided slice of the zero-padded NHWC input and one float64 matmul per
tap and group. It shares nothing with any library convolution (tests/test_conv_ref_bounds.py compares it with F.conv2d).

Bound (derived, first order; u = 2^-24 is fp32's unit roundoff, U the output type's, F fp16's subnormal floor - the definitions of
tests/test_gpu_dw_se.py, imported, not copied). K = kh kw Cin / groups terms per output, S = sum |x||w| over them:

    e_pre = (K + 3) 2^-23 (|scale| S + |shift|)

2^-23 = 2u per operation, not the u of the depthwise sweep: how the matrix units round inside one instruction is not documented,
and 2u per addition covers round-to-nearest and truncation in any summation order. The products of 16-bit operands are exact in
fp32; the + 3 covers an fp32 product rounding (fp32 storage), the scale multiply and the shift add. Then, as in the depthwise sweep:
    act       e_a = L_act e_pre + T_act(pre)
    gate g    e_g = |g| e_a + u |a g|
    residual  e_r = e_g + u (|a g| + |res|)
    post_act  e_y = L_post e_r + T_post(r)
    output    |y - ref| <= U |ref| + (1 + U) e_y + F
A residual the kernel computes itself (res_err, tests/pair_ref.py: the identity convolution recomputed inside the fused 1x1 pair): the
reference adds the exact float64 skip `res`, the kernel adds a value res' with |res' - res| <= res_err elementwise. The sum a g + res'
is off by e_g + res_err before the addition rounds, and the addition rounds a result of magnitude at most |a g| + |res| + res_err:
    residual  e_r = e_g + res_err + u (|a g| + |res| + res_err)
With res_err = None (a residual read from memory, exact) this is the line above.
Pooled stem (the MaxPool2d(3, 2, 1) fused behind the convolution): the reference is the pool, with -inf padding, of the reference
ROUNDED to the storage type. max is 1-Lipschitz in the maximum norm, so the pooled bound is the maximum over the window of the
per-element distance to that rounded reference: the per-element bound above plus the U |ref| by which the rounding moved the
reference itself (without that term a kernel value and a reference value on two sides of a rounding boundary are a whole ulp apart
while the bound allows half of one).

Operands come from pytorchcv_amd.synth (hash_normal / hash_uniform). Magnitudes below 2^-10 are replaced by +-2^-10: neither 16-bit
type then holds a subnormal, so nothing here makes a claim about subnormal flushing. Weights are scaled by K^-1/2, scale lies in
[0.5, 1.5], shift is of order 1; x, w and res are rounded to the storage type before either side sees them, so packing is lossless
and only the kernel's arithmetic separates the two sides.
"""

import collections
import math

import torch

from pytorchcv_amd.synth import hash_normal, hash_uniform
from test_gpu_dw_se import FLOOR, NONE, TDT, U32, ULP, act64, act_err, out_bound  # noqa: F401  (re-exported)

Geom = collections.namedtuple("Geom", "kh kw sh sw pt pl pb pr dh dw groups Cin")
U_MMA = 2.0 ** -23
TINY = 2.0 ** -10


def out_hw(H, W, g):
    """output size; 0 where the dilated filter does not fit into the padded input"""
    eh = H + g.pt + g.pb - g.dh * (g.kh - 1) - 1
    ew = W + g.pl + g.pr - g.dw * (g.kw - 1) - 1
    return (eh // g.sh + 1 if eh >= 0 else 0), (ew // g.sw + 1 if ew >= 0 else 0)


def conv_terms(x, w, g):
    """z = conv(x, w) and S = conv(|x|, |w|) in float64. x NHWC (channels beyond g.Cin are ignored: a view of a wider buffer),
    w OIHW [Cout][Cin / groups][kh][kw]."""
    x = x[..., :g.Cin].double()
    w = w.double()
    N, H, W, _ = x.shape
    Cout = w.shape[0]
    cgi, cgo = g.Cin // g.groups, Cout // g.groups
    assert w.shape[1] == cgi and w.shape[2] == g.kh and w.shape[3] == g.kw
    Ho, Wo = out_hw(H, W, g)
    assert Ho > 0 and Wo > 0
    xp = torch.zeros((N, H + g.pt + g.pb, W + g.pl + g.pr, g.Cin), dtype=torch.float64)
    xp[:, g.pt:g.pt + H, g.pl:g.pl + W] = x
    xa = xp.abs()
    z = torch.zeros((N, Ho, Wo, Cout), dtype=torch.float64)
    S = torch.zeros_like(z)
    for r in range(g.kh):
        for q in range(g.kw):
            rows = slice(r * g.dh, r * g.dh + g.sh * (Ho - 1) + 1, g.sh)
            cols = slice(q * g.dw, q * g.dw + g.sw * (Wo - 1) + 1, g.sw)
            for k in range(g.groups):
                ci, co = slice(k * cgi, (k + 1) * cgi), slice(k * cgo, (k + 1) * cgo)
                wt = w[co, :, r, q].t()
                z[..., co] += xp[:, rows, cols, ci] @ wt
                S[..., co] += xa[:, rows, cols, ci] @ wt.abs()
    return z, S


def conv_ref_err(x, w, scale, shift, geom, act, res=None, post=NONE, gate=None, res_err=None):
    """(reference, S, bound of the kernel's fp32 error before the output rounding), all float64 NHWC [N][Ho][Wo][Cout]; res_err: an
    elementwise bound on the error of a residual the kernel computes itself (module docstring), None for one it reads"""
    z, S = conv_terms(x, w, geom)
    K = geom.kh * geom.kw * (geom.Cin // geom.groups)
    sc = scale.double() if scale is not None else torch.ones(z.shape[-1], dtype=torch.float64)
    sh = shift.double() if shift is not None else torch.zeros(z.shape[-1], dtype=torch.float64)
    pre = sc * z + sh
    err = (K + 3) * U_MMA * (sc.abs() * S + sh.abs())
    a = act64(pre, act)
    err = act_err(pre, err, act)
    if gate is not None:
        gg = gate.double()[:, None, None, :]
        a = a * gg
        err = gg.abs() * err + U32 * a.abs()
    v = a
    if res is not None:
        v = a + res.double()
        if res_err is None:
            err = err + U32 * (a.abs() + res.double().abs())
        else:
            err = err + res_err + U32 * (a.abs() + res.double().abs() + res_err)
    y = act64(v, post)
    if post != NONE:
        err = act_err(v, err, post)
    return y, S, err


def conv_ref(x, w, scale, shift, geom, act, res=None, post=NONE, gate=None):
    """(reference, S = sum |x||w| computed the same way)"""
    y, S, _ = conv_ref_err(x, w, scale, shift, geom, act, res, post, gate)
    return y, S


def conv_ref_bound(x, w, scale, shift, geom, act, res=None, post=NONE, gate=None, out_dtype="fp32", res_err=None):
    """(reference, elementwise bound on |y - reference| for a y stored as out_dtype)"""
    y, _, err = conv_ref_err(x, w, scale, shift, geom, act, res, post, gate, res_err)
    return y, out_bound(y, err, out_dtype)


def round_to(v, dtype):
    """values rounded to the storage type, held in fp32 (exact)"""
    return v.float().to(TDT[dtype]).float()


def _pool_max(t, Hq, Wq):
    """3 x 3 / stride 2 / pad 1 window maximum of NHWC t, the padding taken as -inf"""
    N, Ho, Wo, C = t.shape
    tp = torch.full((N, 2 * Hq + 1, 2 * Wq + 1, C), float("-inf"), dtype=t.dtype)
    tp[:, 1:1 + Ho, 1:1 + Wo] = t[:, :2 * Hq, :2 * Wq]
    out = torch.full((N, Hq, Wq, C), float("-inf"), dtype=t.dtype)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, tp[:, dy:dy + 2 * Hq - 1:2, dx:dx + 2 * Wq - 1:2])
    return out


def pool_out_hw(Ho, Wo):
    return (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1


def pool_ref_bound(ref, bound, dtype):
    """MaxPool2d(3, 2, 1) of the rounded reference, and the pooled bound (module docstring)"""
    Hq, Wq = pool_out_hw(ref.shape[1], ref.shape[2])
    rr = round_to(ref, dtype).double()
    return _pool_max(rr, Hq, Wq), _pool_max(bound + ULP[dtype] * ref.abs(), Hq, Wq)


def pool_values(y):
    """the same pool of any NHWC tensor (the emulated kernel of the CPU checks)"""
    Hq, Wq = pool_out_hw(y.shape[1], y.shape[2])
    return _pool_max(y, Hq, Wq)


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _floor_mag(v):
    return torch.where(v.abs() < TINY, torch.where(v < 0, -TINY, TINY).to(v.dtype), v)


def normal(seed, stream, shape):
    n = int(math.prod(shape))
    return torch.from_numpy(hash_normal(seed, stream, n)).view(*shape)


def uniform(seed, stream, shape):
    n = int(math.prod(shape))
    return torch.from_numpy(hash_uniform(seed, stream, n)).view(*shape)


def storage_normal(seed, stream, shape, dtype, gain=1.0):
    """hash_normal * gain, no magnitude below 2^-10, rounded to the storage type (fp32 tensor of exactly representable values)"""
    return round_to(_floor_mag(normal(seed, stream, shape) * gain), dtype)


Operands = collections.namedtuple("Operands", "x w scale shift res gate")


def operands(N, H, W, Cout, geom, dtype, seed, with_res=False, with_gate=False):
    """x NHWC [N][H][W][Cin], w OIHW, fp32 scale / shift, res NHWC [N][Ho][Wo][Cout] (or None), gate fp32 [N][Cout] (or None)"""
    g = geom
    K = g.kh * g.kw * (g.Cin // g.groups)
    Ho, Wo = out_hw(H, W, g)
    x = storage_normal(seed, 1, (N, H, W, g.Cin), dtype)
    w = storage_normal(seed, 2, (Cout, g.Cin // g.groups, g.kh, g.kw), dtype, gain=K ** -0.5)
    scale = (0.5 + uniform(seed, 3, (Cout,))).float()
    shift = normal(seed, 4, (Cout,)).float()
    res = storage_normal(seed, 5, (N, Ho, Wo, Cout), dtype) if with_res else None
    gate = (uniform(seed, 6, (N, Cout)) * 2 - 0.5).float() if with_gate else None
    return Operands(x, w, scale, shift, res, gate)
