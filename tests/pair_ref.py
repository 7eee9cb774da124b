"""
Float64 reference and elementwise bound of the fused 1x1 pair (csrc/pair1x1.hpp, csrc/wpair1x1.hpp; plain module: CPU only), shared by
tests/test_gpu_pair_sweep.py (the kernels) and tests/test_pair_ref_bounds.py (the CPU proof). Built on tests/conv_ref.py: every
convolution here is that module's conv_ref_err with a 1x1 geometry, nothing of it is restated.

    y1 = post1( act1( scale1 * (W1 . x) + shift1 ) * gate + res )          stored in the 16-bit type
    y2 = act2( scale2 * (W2 . y1) + shift2 )                                stored in the 16-bit type

y1   is one fused convolution: conv_ref_bound(x, w1, scale1, shift1, 1x1, act1, res, post1, gate, out_dtype=dtype), the derivation of
     tests/conv_ref.py as it stands.
y2   takes as its input the y1 THE KERNEL STORED. Both kernel headers say that the rounded y1 packs are GEMM2's B fragments, so whatever
     y1 holds, y2 must satisfy the single-convolution bound conv_ref_bound(y1_stored, w2, scale2, shift2, 1x1, act2, out_dtype=dtype).
     With the y1 check this pins the whole pair elementwise (a wrong value in a small-magnitude output fails), and no error of the first
     convolution has to be carried through the second.
     One more term, derived: how the matrix units treat 16-bit SUBNORMAL inputs is not documented here (conv_ref's operands hold none,
     but the kernel's own y1 can hold a few in fp16: outputs just above zero). Such an element may be read as anything between itself
     and zero, which moves the sum by at most |y1_k| |w2_k|, so
         e_pre(y2) += |scale2| sum_k [0 < |y1_k| < smallest normal] |y1_k| |w2_k|
     before the activation (times L_act2 behind it; the activations' own T terms do not depend on it to first order).
identity-convolution form (pair1x1.hpp, IDC): res is not read but computed, skip' = round(BN_id(W_id . x0)), which no test can
     observe. The reference adds the unrounded float64 skip = BN_id(W_id . x0); res_err is the full output bound of that convolution
     stored in the 16-bit type (out_bound of its conv_ref_err), and conv_ref_err's residual stage becomes
         e_r = e_g + res_err + u (|a g| + |res| + res_err)
     (tests/conv_ref.py, module docstring).

Operands: conv_ref.operands (hash generator, storage-rounded, no magnitude below 2^-10) for each of the two or three convolutions, the
seeds derived from the case by the caller.

The LDS arithmetic of WPairCfg (csrc/wpair1x1.hpp) is restated in wpair_layout: the tile size and whether the gated form keeps the gate
rows in LDS (GATE_LDS) decide which shapes the host accepts; tests/test_pair_ref_bounds.py checks the values, the GPU file routes by them.
"""

import collections

import torch

from conv_ref import Geom, conv_ref_bound, conv_ref_err, operands, out_bound
from test_gpu_dw_se import LIP, NONE

SMALLEST_NORMAL = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14}

PairOps = collections.namedtuple("PairOps", "x w1 scale1 shift1 res gate w2 scale2 shift2 x0 wid scale_id shift_id")


def g1x1(cin):
    return Geom(1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, cin)


def pair_operands(N, H, W, CM, C1, dtype, seed, gated=False, idconv=False):
    """the operands of a pair: conv 1 (with its residual, and its gate where gated) from seed, conv 2 from seed + 1, the identity
    convolution (its own input x0; then there is no residual tensor) from seed + 2"""
    a = operands(N, H, W, C1, g1x1(CM), dtype, seed, with_res=not idconv, with_gate=gated)
    b = operands(1, 1, 1, CM, g1x1(C1), dtype, seed + 1)                  # its x is not used: conv 2 reads y1
    i = operands(N, H, W, C1, g1x1(CM), dtype, seed + 2) if idconv else None
    return PairOps(a.x, a.w, a.scale, a.shift, a.res, a.gate, b.w, b.scale, b.shift, *((i.x, i.w, i.scale, i.shift) if idconv else (None,) * 4))


def skip_ref_err(ops, dtype):
    """(float64 skip of the identity-convolution form, elementwise bound on |the kernel's rounded skip - it|)"""
    skip, _, err = conv_ref_err(ops.x0, ops.wid, ops.scale_id, ops.shift_id, g1x1(ops.x0.shape[-1]), NONE)
    return skip, out_bound(skip, err, dtype)


def y1_ref_bound(ops, act1, post1, dtype):
    """(reference, bound) of y1, NHWC float64"""
    CM = ops.x.shape[-1]
    if ops.x0 is not None:
        skip, skip_err = skip_ref_err(ops, dtype)
        return conv_ref_bound(ops.x, ops.w1, ops.scale1, ops.shift1, g1x1(CM), act1, skip, post1, ops.gate, out_dtype=dtype, res_err=skip_err)
    return conv_ref_bound(ops.x, ops.w1, ops.scale1, ops.shift1, g1x1(CM), act1, ops.res, post1, ops.gate, out_dtype=dtype)


def y2_ref_bound(y1_stored, ops, act2, dtype):
    """(reference, bound) of y2 from the y1 that was stored (any float tensor of 16-bit values, NHWC)"""
    C1 = y1_stored.shape[-1]
    y1 = y1_stored.double()
    ref, _, err = conv_ref_err(y1, ops.w2, ops.scale2, ops.shift2, g1x1(C1), act2)
    sub = torch.where((y1 != 0) & (y1.abs() < SMALLEST_NORMAL[dtype]), y1.abs(), torch.zeros_like(y1))
    if bool((sub != 0).any()):
        extra = ops.scale2.double().abs() * (sub @ ops.w2.double().abs().reshape(-1, C1).t())
        err = err + LIP[act2] * extra
    return ref, out_bound(ref, err, dtype)


# ---- WPairCfg restated (csrc/wpair1x1.hpp) ----------------------------------------------------------------------------------------------
WPairLayout = collections.namedtuple("WPairLayout", "CM C1 NW P NCH A1B A2B SLOT XCH TAB LDS GATE_LDS LDS_GATED")
WPAIR_CONFIGS = ((128, 512), (256, 1024), (128, 256), (256, 512))        # wpair_cfg 0 .. 3 (csrc/pcv_api.hip)
NARROW_TILE = {2: 32, 4: 64}                                              # pair1x1.hpp: P = 16 PB (the gated and identity forms: PB = 2)


def wpair_layout(CM, C1):
    pairw = CM > 128
    nw = (2 if pairw else 1) * 4
    P = 16 * 2 * 4
    A1B = (CM // 64) * 64 * 128
    A2B = CM * 128
    SLOT = A1B + A2B
    XCH = 4 * 2 * 2 * 1024 if pairw else 0
    TAB = 2 * SLOT + XCH
    LDS = TAB + (2 * C1 + 2 * CM) * 4
    gate_lds = LDS + 4 * C1 * 4 <= 80 * 1024
    return WPairLayout(CM, C1, nw, P, C1 // 64, A1B, A2B, SLOT, XCH, TAB, LDS, gate_lds, LDS + (4 * C1 * 4 if gate_lds else 0))
