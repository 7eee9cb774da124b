"""
Float64 reference of the fused stage-1 bottleneck unit (pcv_bottleneck_fused: csrc/bnu.hpp), plain module: CPU only, nothing of the GPU
side is imported. Shared by tests/test_gpu_bnu_sweep.py (the kernel) and tests/test_bnu_ref_bounds.py (the CPU proofs).

    t1 = act1( scale1 * conv1x1(x, w1) + shift1 )                [N][H][56][64]
    t2 = act2( scale2 * conv3x3(t1, w2; pad 1) + shift2 )        [N][H][56][64]      (t1 is zero-padded)
    y  = post( act3( scale3 * conv1x1(t2, w3) + shift3 ) + skip ) [N][H][56][256]
    skip = x (plain form, Cin = 256)   or   scale_id * conv1x1(x, w_id) + shift_id (identity-convolution form, Cin = 64)

Every stage is conv_ref.conv_terms. The reference has the kernel's rounding points: t1, t2, the computed skip and y are each rounded to
the storage type, and a stage is computed on the ROUNDED result of the stage before it.

Exact family (exact_operands). Small integers and dyadic constants, chosen so that every fp32 value inside a correct kernel is exactly
representable whatever the summation order: x integers in [-2, 2], all weights in {-1, 0, 1}, scales powers of two, shifts multiples of
0.5. A correct kernel must equal the reference BIT FOR BIT. `certificate` is the proof obligation, computed from the operands alone:
per stage and output element sum |term| / g < 2^24, g the largest power of two that divides every term (all partial sums, in any order,
are then multiples of g below 2^24 g: fp32 holds them exactly), likewise for the BN step and the skip add.

Bounded family (bounded_operands). Operands as conv_ref.operands draws them (normal values of magnitude >= 2^-10 rounded to the storage
type, weights scaled by K^-1/2, scale in [0.5, 1.5], shift of order 1). Derived first-order bound, stage by stage as tests/mbconv_ref.py
derives its own; nothing is fitted. U the storage type's unit roundoff, F fp16's subnormal floor, U_MMA = 2^-23 per operation
(conv_ref.py). For stage k with K terms per output (K = Cin = 256 or 64, then 576, then 64):

    r     = round(ref_{k-1})               what the reference of stage k is computed on
    d     = out_bound(ref_{k-1}, e_{k-1}) + U |ref_{k-1}|
                                           the kernel's input satisfies |k_{k-1} - r| <= d: it is within out_bound of the unrounded
                                           reference, whose own rounding moved r by at most U |ref|
    S     = conv(|w|, |r| + d)             the magnitudes the kernel's arithmetic works on
    e_pre = (K + 3) U_MMA (|scale| S + |shift|) + |scale| conv(|w|, d)
    activation as conv_ref.py has it.
The skip of the identity-convolution form is one more such stage on x (d = 0), rounded: the kernel's skip is within
res_err = out_bound(skip, e_id) + U |skip| of the reference's rounded skip, and enters the residual add as conv_ref.py's res_err does:
    e_r = e_3 + res_err + u (|a| + |skip| + res_err).
In the plain form the skip is read (res_err = 0). Post-activation and output rounding as conv_ref.py.
"""

import collections

import torch

from conv_ref import Geom, U_MMA, conv_terms, round_to, storage_normal, normal, uniform
from mbconv_ref import granule
from test_gpu_dw_se import FLOOR, NONE, RELU, RELU6, TDT, U32, ULP, act64, act_err, out_bound  # noqa: F401  (re-exported)

W = 56
CM, CO = 64, 256
Unit = collections.namedtuple("Unit", "N H idconv act1 act2 act3 post")
Ops = collections.namedtuple("Ops", "x w1 scale1 shift1 w2 scale2 shift2 w3 scale3 shift3 wid scale_id shift_id")
RESNET = (RELU, RELU, NONE, RELU)


def cin_of(u):
    return 64 if u.idconv else 256


def _g1(C):
    return Geom(1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, C)


G3 = Geom(3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, CM)


def _stage(r, d, w, geom, scale, shift, act):
    """(float64 value behind the activation, the fp32 error bound behind it, sum |term| of the linear part)"""
    z = conv_terms(r, w, geom)[0]
    wa = w.double().abs()
    S = conv_terms(r.abs() + d, wa, geom)[0]
    sc, sh = scale.double(), shift.double()
    K = geom.kh * geom.kw * geom.Cin
    pre = sc * z + sh
    e_pre = (K + 3) * U_MMA * (sc.abs() * S + sh.abs()) + sc.abs() * conv_terms(d, wa, geom)[0]
    return act64(pre, act), act_err(pre, e_pre, act), S


def _between(a, e, dtype, rounded):
    """(what the next stage's reference reads, the distance d of the kernel's value from it)"""
    if not rounded:
        return a, torch.zeros_like(a)
    return round_to(a, dtype).double(), out_bound(a, e, dtype) + ULP[dtype] * a.abs()


def unit_ref(u, ops, dtype, rounded=True):
    """(y, bound on |kernel y - y| for a y stored as dtype, t1, t2, skip), float64 NHWC; t1, t2 and the skip as the next stage reads
    them (rounded). rounded=False: the plain float64 composition, no rounding point."""
    x = ops.x.double()
    zero = torch.zeros_like(x)
    a, e, _ = _stage(x, zero, ops.w1, _g1(cin_of(u)), ops.scale1, ops.shift1, u.act1)
    t1, d1 = _between(a, e, dtype, rounded)
    a, e, _ = _stage(t1, d1, ops.w2, G3, ops.scale2, ops.shift2, u.act2)
    t2, d2 = _between(a, e, dtype, rounded)
    a, e, _ = _stage(t2, d2, ops.w3, _g1(CM), ops.scale3, ops.shift3, u.act3)
    if u.idconv:
        sa, se, _ = _stage(x, zero, ops.wid, _g1(64), ops.scale_id, ops.shift_id, NONE)
        skip, res_err = _between(sa, se, dtype, rounded)
    else:
        skip, res_err = x, torch.zeros_like(x)
    v = a + skip
    e = e + res_err + U32 * (a.abs() + skip.abs() + res_err)
    y = act64(v, u.post)
    if u.post != NONE:
        e = act_err(v, e, u.post)
    return y, out_bound(y, e, dtype), t1, t2, skip


def exact_result(u, ops, dtype):
    """what a correct kernel stores for exact-family operands: the float64 result rounded to the storage type by torch's conversion"""
    return unit_ref(u, ops, dtype)[0].float().to(TDT[dtype])


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _ints(seed, stream, shape, lo, hi):
    return torch.floor(uniform(seed, stream, shape).double() * (hi - lo + 1)).clamp(max=hi - lo).float() + lo


def _pick(seed, stream, n, values):
    v = torch.tensor(values, dtype=torch.float32)
    return v[_ints(seed, stream, (n,), 0, len(values) - 1).long()]


def exact_operands(u, seed):
    """the exact family's operands (module docstring); every value is exact in bf16 and in fp16"""
    ci = cin_of(u)
    x = _ints(seed, 1, (u.N, u.H, W, ci), -2, 2)
    w1 = _ints(seed, 2, (CM, ci, 1, 1), -1, 1)
    scale1 = _pick(seed, 3, CM, [2.0 ** -4, 2.0 ** -3])
    shift1 = 0.5 * _ints(seed, 4, (CM,), -4, 4)
    w2 = _ints(seed, 5, (CM, CM, 3, 3), -1, 1)
    scale2 = _pick(seed, 6, CM, [2.0 ** -5, 2.0 ** -4])
    shift2 = 0.5 * _ints(seed, 7, (CM,), -4, 4)
    w3 = _ints(seed, 8, (CO, CM, 1, 1), -1, 1)
    scale3 = _pick(seed, 9, CO, [2.0 ** -4, 2.0 ** -3, 2.0 ** -2])
    shift3 = 0.5 * _ints(seed, 10, (CO,), -6, 6)
    wid = scale_id = shift_id = None
    if u.idconv:
        wid = _ints(seed, 11, (CO, ci, 1, 1), -1, 1)
        scale_id = _pick(seed, 12, CO, [2.0 ** -3, 2.0 ** -2, 2.0 ** -1])
        shift_id = 0.5 * _ints(seed, 13, (CO,), -6, 6)
    return Ops(x, w1, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3, wid, scale_id, shift_id)


def bounded_operands(u, dtype, seed):
    """operands as conv_ref.operands draws them, per stage"""
    ci = cin_of(u)
    x = storage_normal(seed, 1, (u.N, u.H, W, ci), dtype)
    w1 = storage_normal(seed, 2, (CM, ci, 1, 1), dtype, gain=ci ** -0.5)
    scale1 = (0.5 + uniform(seed, 3, (CM,))).float()
    shift1 = normal(seed, 4, (CM,)).float()
    w2 = storage_normal(seed, 5, (CM, CM, 3, 3), dtype, gain=(9 * CM) ** -0.5)
    scale2 = (0.5 + uniform(seed, 6, (CM,))).float()
    shift2 = normal(seed, 7, (CM,)).float()
    w3 = storage_normal(seed, 8, (CO, CM, 1, 1), dtype, gain=CM ** -0.5)
    scale3 = (0.5 + uniform(seed, 9, (CO,))).float()
    shift3 = normal(seed, 10, (CO,)).float()
    wid = scale_id = shift_id = None
    if u.idconv:
        wid = storage_normal(seed, 11, (CO, ci, 1, 1), dtype, gain=ci ** -0.5)
        scale_id = (0.5 + uniform(seed, 12, (CO,))).float()
        shift_id = normal(seed, 13, (CO,)).float()
    return Ops(x, w1, scale1, shift1, w2, scale2, shift2, w3, scale3, shift3, wid, scale_id, shift_id)


# ---- certificate -----------------------------------------------------------------------------------------------------------------------
def certificate(u, ops, dtype):
    """per stage the largest sum |term| / g over its output elements, for the linear part (the products w * input), the BN step (scale *
    z and shift) and, behind conv3, the skip add. Every value must be < 2^24."""
    y, _, t1, t2, skip = unit_ref(u, ops, dtype)
    out = {}

    def stage(name, r, w, geom, scale, shift):
        S = conv_terms(r.abs(), w.double().abs(), geom)[0]
        g = granule(r) * granule(w)
        out[name + ".sum"] = float(S.max()) / g
        sc, sh = scale.double(), shift.double()
        g2 = min(granule(sc) * g, granule(sh))
        out[name + ".bn"] = float((sc.abs() * S + sh.abs()).max()) / g2
        return g2

    x = ops.x.double()
    stage("t1", x, ops.w1, _g1(cin_of(u)), ops.scale1, ops.shift1)
    stage("t2", t1, ops.w2, G3, ops.scale2, ops.shift2)
    g = stage("y", t2, ops.w3, _g1(CM), ops.scale3, ops.shift3)
    if u.idconv:
        stage("skip", x, ops.wid, _g1(64), ops.scale_id, ops.shift_id)
    pre = ops.scale3.double() * conv_terms(t2, ops.w3, _g1(CM))[0] + ops.shift3.double()
    out["y.res"] = float((act64(pre, u.act3).abs() + skip.abs()).max()) / min(g, granule(skip))
    return out


def certified(u, ops, dtype):
    worst = max(certificate(u, ops, dtype).values())
    return worst < 2.0 ** 24, worst


__all__ = ["Unit", "Ops", "RESNET", "W", "CM", "CO", "cin_of", "unit_ref", "exact_result", "exact_operands", "bounded_operands",
           "certificate", "certified", "RELU", "RELU6", "NONE"]
