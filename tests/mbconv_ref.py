"""
Float64 reference of the fused inverted-residual unit (pcv_mbconv_fused: csrc/mbr.hpp, csrc/mbw.hpp, csrc/mbconv.hpp), plain module:
CPU only, nothing of the GPU side is imported. Shared by tests/test_gpu_mbconv_sweep.py (the kernels) and
tests/test_mbconv_ref_bounds.py (the CPU proofs).

    E = act_e( scale_e * conv1x1(x, w_exp) + shift_e )              [N][H][W][Cmid]     (absent without an expand stage: E = x)
    D = act_d( scale_d * dw3x3(E, w_dw; pad 1, stride s) + shift_d ) [N][Ho][Wo][Cmid]   (the EXPANDED map is zero-padded)
    y = post( act_p( scale_p * conv1x1(D, w_proj) + shift_p ) + res ) [N][Ho][Wo][Cout]

The two 1x1 stages are conv_ref.conv_terms (one float64 matmul), the depthwise stage is test_gpu_dw_se.dw_ref (an explicit loop over
the nine taps). The reference has the kernels' three rounding points: E, D and y are each rounded to the storage type, and stage k is
computed on the ROUNDED result of stage k - 1.

Exact family (exact_operands). Small integers and dyadic constants, chosen so that every fp32 value inside a correct kernel is exactly
representable whatever the summation order: x and the residual are integers in [-3, 3], the 1x1 weights lie in {-1, 0, 1}, the
depthwise taps are integers in [-2, 2], scale_e = 0.75 * 2^-k (k = 1, 2, 3), shift_e and shift_d are multiples of 0.75 in [-3, 6],
scale_d is 0.25 / 0.5 / 1, scale_p is 2^-4 / 2^-3 / 2^-2 and shift_p a multiple of 0.5. The multiples of 0.75 = 6 / 8 keep mbr.hpp's
fp16 + ReLU6 form exact too: it holds E / 6 and D / 6 (constants multiplied by float32(1 / 6), which for these values rounds back to
the exact quotient), and E / 6 is then a multiple of 1 / 8. A correct kernel must equal the reference BIT FOR BIT. `certificate`
is the proof obligation: per stage and per output element sum |term| / g < 2^24, g the largest power of two that divides every term
(all partial sums, in any order, are then multiples of g below 2^24 g: fp32 holds them exactly). It is a condition on the operands,
computed from them alone.

Bounded family (bounded_operands). Operands as conv_ref.operands draws them (normal values of magnitude >= 2^-10 rounded to the
storage type, weights scaled by K^-1/2, scale in [0.5, 1.5], shift of order 1). Derived first-order bound, not fitted to anything
observed. With U the storage type's unit roundoff, F fp16's subnormal floor, U_MMA = 2^-23 per operation (conv_ref.py: the matrix
pipe's internal rounding is undocumented; the depthwise stage runs on the matrix pipe here, so it takes U_MMA too and not the u of
the depthwise sweep), for stage k with K terms per output:

    r    = round(ref_{k-1})                     what the reference of stage k is computed on
    d    = out_bound(ref_{k-1}, e_{k-1}) + U |ref_{k-1}| + 5 F
                                                the kernel's input k_{k-1} satisfies |k_{k-1} - r| <= d: it is within out_bound of
                                                the unrounded reference, whose rounding moved r by at most U |ref| (pool_ref_bound's
                                                argument). 5 F more because the folded form rounds E / 6, whose subnormal floor is
                                                6 F in units of E
    S    = conv(|w|, |r| + d)                   the magnitudes the kernel's own arithmetic works on
    e_pre = (K + 3 + c) U_MMA (|scale| S + |shift|) + |scale| conv(|w|, d)
                                                c = folded constants of the stage, one more rounding each: 2 (scale_e / 6, shift_e / 6),
                                                1 (shift_d / 6), 1 (6 scale_p). Applied to every instance, folded or not
    activation, residual, post-activation and output rounding exactly as conv_ref.py has them.
In bf16 this worst-case chain is loose at large Cmid (about a tenth of a typical output at Cmid = 144), which is why the exact family
carries the geometry and the bounded cases that must tell bugs apart keep Cmid small.
"""

import collections

import torch

from conv_ref import Geom, U_MMA, conv_terms, round_to, storage_normal, normal, uniform
from test_gpu_dw_se import FLOOR, NONE, RELU, RELU6, U32, ULP, act64, act_err, dw_ref, out_bound

Unit = collections.namedtuple("Unit", "N H W Cin Cmid Cout stride expand act_e act_d act_p post res")
# res: None, "own" (a tensor of its own) or "x" (the unit's input, as the engine passes it)
Ops = collections.namedtuple("Ops", "x w_exp scale_e shift_e w_dw scale_d shift_d w_proj scale_p shift_p res")
FOLDED_EXTRA = (2, 1, 1)


def out_hw(u):
    return (u.H - 1) // u.stride + 1, (u.W - 1) // u.stride + 1


def _g1(C):
    return Geom(1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, C)


def taps_of(w_dw):
    """[9][C] taps of a depthwise weight [C][1][3][3]"""
    return w_dw.reshape(w_dw.shape[0], 9).t().contiguous()


def _dw_lin(t, taps, s):
    """depthwise 3x3 / pad 1 / stride s of NHWC t as a float64 linear map (dw_ref with scale 1, shift 0 and no activation)"""
    C = t.shape[3]
    return dw_ref(t, taps, torch.ones(C), torch.zeros(C), 3, s, (1, 1, 1, 1), NONE)[0]


def _pw_lin(t, w):
    return conv_terms(t, w, _g1(w.shape[1]))[0]


def _stage(lin, absw_lin, r, d, scale, shift, K, extra, act):
    """(float64 value before the activation, after it, the fp32 error bound behind the activation, sum |term| of the linear part)"""
    z = lin(r)
    sc, sh = scale.double(), shift.double()
    S = absw_lin(r.abs() + d)
    pre = sc * z + sh
    e_pre = (K + 3 + extra) * U_MMA * (sc.abs() * S + sh.abs()) + sc.abs() * absw_lin(d)
    return pre, act64(pre, act), act_err(pre, e_pre, act), S


def _between(a, e, dtype, rounded):
    """(what the next stage's reference reads, the distance d of the kernel's value from it)"""
    if not rounded:
        return a, torch.zeros_like(a)
    d = out_bound(a, e, dtype) + ULP[dtype] * a.abs() + 5 * FLOOR[dtype]
    return round_to(a, dtype).double(), d


def residual_of(u, ops):
    return ops.x if u.res == "x" else ops.res


def unit_ref(u, ops, dtype, rounded=True, drop_tap=None):
    """(y, bound on |kernel y - y| for a y stored as dtype, E, D), float64 NHWC; E and D as the next stage reads them (rounded).
    rounded=False: the plain float64 composition, no rounding point. drop_tap=(tap, channel): that tap is left out (used once by the
    CPU checks to show that a broken reference fails them)."""
    x = ops.x.double()
    zero = torch.zeros_like(x)
    if u.expand:
        we = ops.w_exp.double()
        _, a, e, _ = _stage(lambda t: _pw_lin(t, we), lambda t: _pw_lin(t, we.abs()), x, zero, ops.scale_e, ops.shift_e,
                            u.Cin, FOLDED_EXTRA[0], u.act_e)
        E, dE = _between(a, e, dtype, rounded)
    else:
        E, dE = x, zero
    taps = taps_of(ops.w_dw.double())
    if drop_tap is not None:
        taps = taps.clone()
        taps[drop_tap[0], drop_tap[1]] = 0
    _, a, e, _ = _stage(lambda t: _dw_lin(t, taps, u.stride), lambda t: _dw_lin(t, taps.abs(), u.stride), E, dE, ops.scale_d,
                        ops.shift_d, 9, FOLDED_EXTRA[1], u.act_d)
    D, dD = _between(a, e, dtype, rounded)
    wp = ops.w_proj.double()
    _, a, e, _ = _stage(lambda t: _pw_lin(t, wp), lambda t: _pw_lin(t, wp.abs()), D, dD, ops.scale_p, ops.shift_p, u.Cmid,
                        FOLDED_EXTRA[2], u.act_p)
    v = a
    res = residual_of(u, ops)
    if res is not None:
        v = a + res.double()
        e = e + U32 * (a.abs() + res.double().abs())
    y = act64(v, u.post)
    if u.post != NONE:
        e = act_err(v, e, u.post)
    return y, out_bound(y, e, dtype), E, D


def exact_result(u, ops, dtype):
    """what a correct kernel stores for exact-family operands: the float64 result rounded to the storage type by torch's conversion"""
    from test_gpu_dw_se import TDT
    return unit_ref(u, ops, dtype)[0].float().to(TDT[dtype])


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _ints(seed, stream, shape, lo, hi):
    return torch.floor(uniform(seed, stream, shape).double() * (hi - lo + 1)).clamp(max=hi - lo).float() + lo


def _pick(seed, stream, n, values):
    v = torch.tensor(values, dtype=torch.float32)
    return v[_ints(seed, stream, (n,), 0, len(values) - 1).long()]


def exact_operands(u, seed):
    """the exact family's operands (module docstring); every value is exact in bf16 and in fp16"""
    Ho, Wo = out_hw(u)
    x = _ints(seed, 1, (u.N, u.H, u.W, u.Cin), -3, 3)
    w_exp = scale_e = shift_e = None
    if u.expand:
        w_exp = _ints(seed, 2, (u.Cmid, u.Cin, 1, 1), -1, 1)
        scale_e = _pick(seed, 3, u.Cmid, [0.75 * 2.0 ** -k for k in (1, 2, 3)])
        shift_e = 0.75 * _ints(seed, 4, (u.Cmid,), -4, 8)
    w_dw = _ints(seed, 5, (u.Cmid, 1, 3, 3), -2, 2)
    scale_d = _pick(seed, 6, u.Cmid, [0.25, 0.5, 1.0])
    shift_d = 0.75 * _ints(seed, 7, (u.Cmid,), -4, 8)
    w_proj = _ints(seed, 8, (u.Cout, u.Cmid, 1, 1), -1, 1)
    scale_p = _pick(seed, 9, u.Cout, [2.0 ** -4, 2.0 ** -3, 2.0 ** -2])
    shift_p = 0.5 * _ints(seed, 10, (u.Cout,), -6, 6)
    res = _ints(seed, 11, (u.N, Ho, Wo, u.Cout), -3, 3) if u.res == "own" else None
    return Ops(x, w_exp, scale_e, shift_e, w_dw, scale_d, shift_d, w_proj, scale_p, shift_p, res)


def bounded_operands(u, dtype, seed):
    """operands as conv_ref.operands draws them, per stage"""
    Ho, Wo = out_hw(u)
    x = storage_normal(seed, 1, (u.N, u.H, u.W, u.Cin), dtype)
    w_exp = scale_e = shift_e = None
    if u.expand:
        w_exp = storage_normal(seed, 2, (u.Cmid, u.Cin, 1, 1), dtype, gain=u.Cin ** -0.5)
        scale_e = (0.5 + uniform(seed, 3, (u.Cmid,))).float()
        shift_e = normal(seed, 4, (u.Cmid,)).float()
    w_dw = storage_normal(seed, 5, (u.Cmid, 1, 3, 3), dtype, gain=1.0 / 3.0)
    scale_d = (0.5 + uniform(seed, 6, (u.Cmid,))).float()
    shift_d = normal(seed, 7, (u.Cmid,)).float()
    w_proj = storage_normal(seed, 8, (u.Cout, u.Cmid, 1, 1), dtype, gain=u.Cmid ** -0.5)
    scale_p = (0.5 + uniform(seed, 9, (u.Cout,))).float()
    shift_p = normal(seed, 10, (u.Cout,)).float()
    res = storage_normal(seed, 11, (u.N, Ho, Wo, u.Cout), dtype) if u.res == "own" else None
    return Ops(x, w_exp, scale_e, shift_e, w_dw, scale_d, shift_d, w_proj, scale_p, shift_p, res)


# ---- certificate -----------------------------------------------------------------------------------------------------------------------
_Q = 2.0 ** 40


def granule(*tensors):
    """the largest power of two that divides every value of the tensors (all of them multiples of 2^-40: asserted)"""
    bits = 0
    for t in tensors:
        q = t.double() * _Q
        assert bool((q == q.round()).all()) and float(q.abs().max()) < 2.0 ** 62
        for v in torch.unique(q.abs().long()).tolist():
            bits |= v
    assert bits != 0
    return (bits & -bits) / _Q


def certificate(u, ops, dtype, folded=False):
    """per stage the largest sum |term| / g over its output elements, for the linear part (the products w * input), the BN step (scale *
    z and shift) and, behind the projection, the residual add. Every value must be < 2^24. folded: with mbr.hpp's constants (scale_e / 6,
    shift_e / 6, shift_d / 6, 6 scale_p; E / 6 and D / 6 between the stages)."""
    six = 6.0 if folded else 1.0
    y, _, E, D = unit_ref(u, ops, dtype)
    out = {}

    def stage(name, r, absw_lin, w, scale, shift):
        S = absw_lin(r.abs())
        g = granule(r) * granule(w)
        out[name + ".sum"] = float(S.max()) / g
        sc, sh = scale.double(), shift.double()
        g2 = min(granule(sc) * g, granule(sh))
        out[name + ".bn"] = float((sc.abs() * S + sh.abs()).max()) / g2
        return g2

    x = ops.x.double()
    if u.expand:
        we = ops.w_exp.double()
        stage("E", x, lambda t: _pw_lin(t, we.abs()), we, ops.scale_e.double() / six, ops.shift_e.double() / six)
    else:
        E = x
    taps = taps_of(ops.w_dw.double())
    Ein = E / six if u.expand else E
    stage("D", Ein, lambda t: _dw_lin(t, taps.abs(), u.stride), taps, ops.scale_d, ops.shift_d.double() / six)
    wp = ops.w_proj.double()
    g = stage("y", D / six, lambda t: _pw_lin(t, wp.abs()), wp, ops.scale_p.double() * six, ops.shift_p)
    res = residual_of(u, ops)
    if res is not None:
        pre = ops.scale_p.double() * _pw_lin(D, wp) + ops.shift_p.double()
        out["y.res"] = float((act64(pre, u.act_p).abs() + res.double().abs()).max()) / min(g, granule(res))
    return out


def certified(u, ops, dtype):
    """the certificate holds, for the plain form and - where mbr.hpp's folded form can run (fp16, both inner stages ReLU6) - for that"""
    forms = [False] + ([True] if dtype == "fp16" and u.expand and u.act_e == RELU6 and u.act_d == RELU6 else [])
    worst = max(v for f in forms for v in certificate(u, ops, dtype, f).values())
    return worst < 2.0 ** 24, worst


__all__ = ["Unit", "Ops", "unit_ref", "exact_result", "exact_operands", "bounded_operands", "certificate", "certified", "out_hw",
           "taps_of", "residual_of", "RELU", "RELU6", "NONE"]
