"""
GPU sweep of the fused inverted-residual unit, pcv_mbconv_fused, on its three kernels - register-resident tiles (csrc/mbr.hpp), wave-
private tiles (csrc/mbw.hpp), block tiles (csrc/mbconv.hpp) - against the float64 reference of tests/mbconv_ref.py
(tests/test_mbconv_ref_bounds.py proves on the CPU that the reference equals torch's float64 composition, that an emulated fp32 kernel
equals it bit for bit on the exact family and stays inside the derived bound on the bounded one, and that the listed kernel bugs are
told from a correct kernel).

The sweep drives the C ABI directly: its own three pcv_conv_desc, pcv_conv_pack / pcv_dwconv_pack, then pcv_mbconv_fused. That reaches
what the engine never sets: any Cmid, act_p / post_act, a residual that is not the unit's input. Two operand families:
  exact    small integers and dyadic BN constants (mbconv_ref.exact_operands): the kernel must equal the reference bit for bit, so one
           wrong tap in one channel, or one wrong column at a tile's edge, fails
  bounded  general operands (mbconv_ref.bounded_operands) against the derived elementwise bound: BN arithmetic with general constants,
           all seven activation codes, fp16 range behaviour
Every case runs on the resident grid and under max_blocks = 8, into a NaN-filled y with a guard tail: an element nobody wrote fails the
comparison, a store behind y fails the guard check. The kernel is forced with the library's own switches (mbr, mbr_xl, mbw = 0 / 1 / 8 /
16); the first assertion of every test is the routing of pcv_mbconv_fused restated here (`route`): this case runs this instance.
Shapes are the smallest at which each tiling can go wrong: Wo in {OC, OC + 1, 2 OC + 1} and Ho in {8, the next value with Ho % RO == 1}
for tiles of RO x OC outputs, N = 2 or 3 so that the tile count is no multiple of the waves per block, ragged last 32-channel chunks.
"""

import collections
import ctypes
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import util
from mbconv_ref import Unit, bounded_operands, exact_operands, exact_result, out_hw, residual_of, unit_ref
from test_gpu_dw_se import CODE, HSIGMOID, HSWISH, NONE, RELU, RELU6, SIGMOID, SWISH, TDT

pytestmark = pytest.mark.gpu

GRIDS = [0, 8]
DTYPES16 = ("bf16", "fp16")
PCV_ERR_INVALID = -1
K_MBW_MAX_LDS, K_MB_MAX_LDS = 160 * 1024, 150 * 1024            # kMbwMaxLds, kMbMaxLds (csrc/pcv_api.hip; checked by the CPU file)
SWITCHES = {"mbr": dict(mbr=1, mbr_xl=1, mbw=1), "mbr_nx": dict(mbr=1, mbr_xl=0, mbw=1), "mbw": dict(mbr=0, mbw=1),
            "mbw8": dict(mbr=0, mbw=8), "mbw16": dict(mbr=0, mbw=16), "blk": dict(mbr=0, mbw=0)}


# ---- LDS layouts restated (csrc/mbr.hpp, csrc/mbw.hpp, csrc/mbconv.hpp) -------------------------------------------------------------
def mbr_lds_total(nrt, nChunks, ka, afl, wel=True, xrows=0, waves=8):
    o = nChunks * ka * 32 * 64 if wel else 0
    o += nChunks * nrt * 16 * 64
    o += nChunks * 6 * 1024 if afl else 0
    o += nChunks * 4 * 32 * 4
    o += 2 * nrt * 16 * 4
    o += waves * 2 * xrows * 1024
    return o


def mbw_npt(stride, tw, rb=0):
    nblk = rb if rb > 0 else (4 if stride == 1 else 2)
    ro = nblk * (16 // tw)
    iw = (tw - 1) * stride + 3
    iws = iw + (1 if stride == 2 and tw == 8 else 0)
    return (((ro - 1) * stride + 3) * iws + 15) // 16


def mbw_lds_total(stride, nrt, nChunks, nWaves, tw, ka=1, rb=0):
    npt, rows = mbw_npt(stride, tw, rb), (rb if rb > 0 else (4 if stride == 1 else 2))
    pitch = 64 if ka == 1 else 80
    o = nChunks * 32 * 64 if ka == 1 else 0
    o += nChunks * nrt * 16 * 64 if ka == 1 else 0
    o += (10 * nChunks * 32 * 2 + 15) & ~15
    o += 4 * nChunks * 32 * 4
    return o + nWaves * (npt * 16 + rows * 16) * pitch


def mb_lds_total(stride, expand, ka, nChunks, nRowT, nbufX):
    npt, outpx = (12, 128) if stride == 1 else (19, 64)
    o = nChunks * ka * 32 * 64 if expand else 0
    o += nChunks * nRowT * 16 * 64
    o += (9 * nChunks * 32 * 2 + 15) & ~15
    o += 4 * nChunks * 32 * 4
    o += nbufX * ka * npt * 16 * 64 if expand else 0
    o += (1 if expand else 2) * npt * 16 * 64
    o += outpx * 64
    o += (npt * 16 + 15) & ~15
    return o


# ---- the routing of pcv_mbconv_fused restated (csrc/pcv_api.hip) ----------------------------------------------------------------------
# kMbr, one dtype: (NRT, RO, S, KA, AFL, WAVES, WEL, XL), each for ACT = ReLU and ReLU6, in table order (pick_mbr takes the first match)
MBR_ROWS = [(2, 7, 1, 1, True, 8, True, True), (2, 7, 1, 1, True, 8, True, False), (4, 4, 1, 1, True, 8, True, False),
            (2, 4, 2, 1, True, 8, True, False), (4, 4, 2, 1, True, 8, True, False), (4, 4, 1, 2, False, 8, True, False),
            (6, 3, 1, 2, False, 8, True, False), (6, 5, 1, 3, False, 4, False, False)]
# kMbw, one dtype: (S, NRT, TW, KA, RB), each for ACT = -1 (launch-time codes), ReLU and ReLU6
MBW_ROWS = ([(s, nrt, tw, 1, 0) for s in (1, 2) for nrt in (2, 4) for tw in (16, 8)] + [(1, 4, tw, 2, 0) for tw in (16, 8)] +
            [(1, 6, 16, ka, 2) for ka in (2, 3)])
Route = collections.namedtuple("Route", "kernel inst RO OC waves lds tw")


def inner_act(u):
    """the activation template argument: the code where both inner stages share ReLU or ReLU6, else -1"""
    return u.act_e if (u.expand and u.act_e == u.act_d and u.act_e in (RELU, RELU6)) else -1


def mbw_shape(Cin, Cout, stride, H, W, wide=1):
    ka = (Cin + 31) // 32
    nrt = 2 if Cout <= 32 else (4 if Cout <= 64 else 6)
    rb = 2 if nrt == 6 else 0
    if H > 250 or W > 250 or Cout > 96:
        ok = False
    elif nrt == 6:
        ok = wide != 0 and stride == 1 and ka in (2, 3)
    else:
        ok = ka == 1 or (ka == 2 and stride == 1 and nrt == 4)
    return ok, ka, nrt, rb


def mbw_waves(stride, nrt, nChunks, tw, ka, rb):
    for nw in (8, 6, 4):
        if mbw_lds_total(stride, nrt, nChunks, nw, tw, ka, rb) <= K_MBW_MAX_LDS:
            return nw
    return 0


def mbconv_plan(stride, expand, ka, nChunks, nRowT):
    """(nbufX, LDS bytes)"""
    two = mb_lds_total(stride, expand, ka, nChunks, nRowT, 2)
    if not expand or two <= 80 * 1024:
        return 2, two
    one = mb_lds_total(stride, expand, ka, nChunks, nRowT, 1)
    if one <= 80 * 1024 or two > K_MB_MAX_LDS:
        return 1, one
    return 2, two


def unsupported(u, dtype="bf16"):
    """mbconv_unsupported for a unit whose three descriptors are otherwise well formed: the reason, or None"""
    if dtype not in DTYPES16:
        return "16-bit storage only"
    if u.stride not in (1, 2):
        return "stride"
    if u.Cmid % 8 != 0:
        return "expanded channels must be a multiple of 8"
    if u.Cout % 8 != 0 or u.Cout > 96:
        return "project stage must be a plain 1x1 with at most 96 channels"
    wave_tiles = u.expand and mbw_shape(u.Cin, u.Cout, u.stride, u.H, u.W)[0]
    if u.Cout > (96 if wave_tiles else 32):
        return "fused unit only pays for narrow projections"
    Ho, Wo = out_hw(u)
    if Wo < (14 if wave_tiles else 24) or Ho < 8:
        return "map too small for the fused unit to pay"
    ka = 0
    if u.expand:
        if u.Cin % 8 != 0:
            return "expand stage must be a plain 1x1 onto the depthwise input"
        ka = (u.Cin + 31) // 32
        if ka > 3:
            return "expand stage input wider than 96 channels"
    elif u.Cin != u.Cmid:
        return "no expand stage: Cin is Cmid"
    nChunks = (u.Cmid + 31) // 32
    if wave_tiles:
        if mbw_waves(u.stride, 2 if u.Cout <= 32 else (4 if u.Cout <= 64 else 6), nChunks, 16, ka, 2 if u.Cout > 64 else 0) == 0:
            return "tiles do not fit the LDS budget"
    elif mbconv_plan(u.stride, u.expand, ka, nChunks, (u.Cout + 31) // 32 * 2)[1] > K_MB_MAX_LDS:
        return "weights + tiles do not fit the LDS budget"
    return None


def pick_mbr(nrt, act, stride, ka, nChunks, use_xl):
    if act not in (RELU, RELU6):
        return None
    for row in MBR_ROWS:
        rnrt, ro, s, rka, afl, waves, wel, xl = row
        nr = ro + 2 if s == 1 else 2 * ro + 1
        lds = mbr_lds_total(rnrt, nChunks, rka, afl, wel, nr if xl else 0, waves)
        if (rnrt, s, rka) == (nrt, stride, ka) and lds <= K_MBW_MAX_LDS and (not xl or use_xl):
            return row, lds
    return None


def route(u, k):
    """the kernel instance pcv_mbconv_fused launches for unit u under the switches SWITCHES[k] (the dtype selects among equal tables)"""
    sw = SWITCHES[k]
    Ho, Wo = out_hw(u)
    S, nChunks = u.stride, (u.Cmid + 31) // 32
    wave_shape, kaw, nrt, rbw = mbw_shape(u.Cin, u.Cout, S, u.H, u.W) if u.expand else (False, 0, 0, 0)
    block_shape = u.Cout <= 32 and Wo >= 24
    act = inner_act(u)
    if wave_shape and sw["mbr"]:
        hit = pick_mbr(nrt, act, S, kaw, nChunks, sw.get("mbr_xl", 1))
        if hit:
            row, lds = hit
            oc = 14 if S == 1 else (15 if nrt == 2 else 7)
            return Route("mbr", (act,) + row, row[1], oc, row[5], lds, 0)
    if wave_shape and (sw["mbw"] or not block_shape):
        nblk = rbw if rbw > 0 else (4 if S == 1 else 2)

        def tiles_of(tw):
            ro = nblk * (16 // tw)
            return ((Ho + ro - 1) // ro) * ((Wo + tw - 1) // tw)
        tw = 8 if mbw_npt(S, 8, rbw) * tiles_of(8) < mbw_npt(S, 16, rbw) * tiles_of(16) else 16
        if sw["mbw"] in (8, 16):
            tw = sw["mbw"]
        if rbw > 0:
            tw = 16
        nw = mbw_waves(S, nrt, nChunks, tw, kaw, rbw)
        if nw > 0:
            row = (S, nrt, tw, kaw, rbw)
            assert row in MBW_ROWS, row                         # pick_mbw would find no instantiation
            return Route("mbw", (act,) + row, nblk * (16 // tw), tw, nw, mbw_lds_total(S, nrt, nChunks, nw, tw, kaw, rbw), tw)
    ka = (u.Cin + 31) // 32 if u.expand else 0
    nRowT = (u.Cout + 31) // 32 * 2
    nbuf, lds = mbconv_plan(S, u.expand, ka, nChunks, nRowT)
    assert nRowT == 2, u                                    # the block kernel is compiled for Cout <= 32 (pcv_mbconv_fused refuses the rest)
    return Route("blk", (S, u.expand), 8 if S == 1 else 4, 16, 4, lds, nbuf)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "u k want")              # want: the kernel the case is meant to run on


def U(Cin, Cmid, Cout, stride, N, H, W, acts=(RELU6, RELU6), expand=True, act_p=NONE, post=NONE, res=None):
    return Unit(N, H, W, Cin, Cmid, Cout, stride, expand, acts[0] if expand else NONE, acts[1], act_p, post, res)


R, R6 = RELU, RELU6
# the epilogue on one small shape per kernel: residual on / off x post_act none / ReLU x act_p none / ReLU6
_EPI = [dict(res=r, post=po, act_p=ap) for r in ("own", None) for po in (NONE, RELU) for ap in (NONE, RELU6)]

# (Cin, Cmid, Cout, stride, N, H, W): per instance row the deciding map sizes, ragged chunks, the 96 -> 576 -> 96 unit once
_MBR_GEOM = [
    (8, 8, 8, 1, 2, 8, 14), (8, 8, 8, 1, 3, 15, 15), (24, 40, 24, 1, 3, 15, 15), (32, 72, 32, 1, 2, 8, 29), (24, 200, 8, 1, 2, 8, 15),
    (24, 40, 64, 1, 3, 9, 15), (32, 144, 40, 1, 2, 8, 29), (8, 72, 64, 1, 2, 9, 14),
    (24, 40, 24, 2, 3, 17, 30), (8, 72, 32, 2, 2, 16, 31), (32, 144, 8, 2, 2, 18, 61),
    (24, 40, 64, 2, 3, 17, 28), (32, 72, 40, 2, 2, 16, 29),
    (40, 72, 64, 1, 3, 9, 15), (64, 144, 40, 1, 2, 8, 29), (64, 200, 64, 1, 2, 9, 14),
    (64, 144, 96, 1, 3, 10, 15), (40, 72, 72, 1, 2, 8, 29),
    (96, 576, 96, 1, 2, 11, 15), (72, 144, 72, 1, 3, 8, 29), (96, 200, 96, 1, 2, 11, 14),
]
_MBW_GEOM = [
    (24, 40, 24, 1, 3, 9, 17), (32, 72, 32, 1, 2, 8, 24), (8, 40, 64, 1, 3, 9, 25), (24, 144, 40, 1, 2, 8, 16),
    (24, 40, 24, 2, 3, 17, 33), (32, 72, 8, 2, 2, 16, 48), (8, 40, 64, 2, 3, 18, 49), (32, 72, 40, 2, 2, 16, 31),
    (40, 72, 64, 1, 3, 9, 17), (64, 200, 40, 1, 2, 8, 24),
]
_MBW_WIDE = [(64, 144, 96, 1, 3, 9, 17), (72, 200, 72, 1, 2, 9, 25), (96, 576, 96, 1, 2, 8, 16)]
# block tiles: Cout <= 32 and Wo >= 24; with and without the expand stage, ka = 1 / 2 / 3; Cout = 16 (half of the second projection row
# tile is padding) is what MobileNetV3's first unit runs
_BLK_GEOM = [
    (24, 40, 24, 1, 3, 9, 33, True), (32, 72, 32, 1, 2, 8, 24, True), (8, 8, 8, 1, 2, 9, 32, True), (24, 40, 24, 2, 3, 17, 65, True),
    (32, 144, 8, 2, 2, 16, 48, True), (64, 144, 32, 1, 2, 8, 24, True), (96, 200, 24, 1, 3, 9, 33, True), (72, 72, 8, 2, 2, 17, 48, True),
    (40, 40, 24, 1, 2, 9, 33, False), (72, 72, 32, 2, 3, 18, 64, False), (8, 8, 8, 1, 2, 8, 24, False),
    (16, 16, 16, 1, 2, 9, 33, False), (16, 72, 16, 2, 2, 17, 48, True),
]


def _exact_cases():
    out = []
    for i, g in enumerate(_MBR_GEOM):
        out.append(Case(U(*g, acts=((R6, R6), (R, R))[i % 2], res="own" if i % 3 == 0 else None), "mbr", "mbr"))
        out.append(Case(U(*g, acts=((R, R), (R6, R6))[i % 2]), "mbr", "mbr"))
    out.append(Case(U(8, 8, 8, 1, 2, 15, 29, acts=(R6, R6)), "mbr_nx", "mbr"))
    out.append(Case(U(8, 8, 8, 1, 2, 15, 29, acts=(R, R)), "mbr_nx", "mbr"))
    for g in ((24, 40, 24, 1, 3, 15, 15), (64, 200, 64, 1, 2, 9, 14), (96, 576, 96, 1, 2, 11, 15)):    # the skip tensor is the unit's input
        out.append(Case(U(*g, acts=(R6, R6), res="x"), "mbr", "mbr"))
    out += [Case(U(24, 40, 24, 1, 3, 15, 15, acts=(R6, R6), **e), "mbr", "mbr") for e in _EPI]
    for i, g in enumerate(_MBW_GEOM):                   # every (stride, NRT, KA) row with both pixel-block widths and the three activation forms
        for j, k in enumerate(("mbw8", "mbw16")):
            for m, a in enumerate(((R6, R6), (R, R), (R, R6))):
                out.append(Case(U(*g, acts=a, res="own" if (i + j + m) % 2 else None), k, "mbw"))
    out += [Case(U(*g, acts=(R6, R6)), "mbw", "mbw") for g in _MBW_GEOM[::3]]           # the library's own choice of the width
    out += [Case(U(*g, acts=a, res="own" if a[0] == R else None), "mbw", "mbw") for g in _MBW_WIDE for a in ((R6, R6), (R, R), (R6, R))]
    out.append(Case(U(24, 40, 24, 1, 3, 9, 17, acts=(R6, R6), res="x"), "mbw", "mbw"))
    out += [Case(U(24, 40, 24, 1, 3, 9, 17, acts=(R6, R), **e), "mbw16", "mbw") for e in _EPI]
    for i, g in enumerate(_BLK_GEOM):
        for a in ((R6, R6), (R, R6)):
            out.append(Case(U(*g[:7], acts=a, expand=g[7], res="own" if i % 2 else None), "blk", "blk"))
    out.append(Case(U(24, 40, 24, 1, 3, 9, 33, acts=(R6, R6), res="x"), "blk", "blk"))
    out += [Case(U(24, 40, 24, 1, 3, 9, 33, acts=(R, R), **e), "blk", "blk") for e in _EPI]
    return list(dict.fromkeys(out))


_ALL_ACTS = (NONE, RELU, RELU6, SIGMOID, SWISH, HSIGMOID, HSWISH)


def _bounded_cases():
    """small Cmid (8 .. 40): BN arithmetic with general constants, every activation code on the inner stages (the launch-time instances of
    mbw.hpp / mbconv.hpp), the clamp codes and h-swish behind the projection, and mbr.hpp's compile-time forms"""
    out = []
    for k, want, g in (("mbw", "mbw", (24, 40, 24, 1, 2, 9, 17)), ("blk", "blk", (24, 40, 24, 1, 2, 9, 33))):
        for i, a in enumerate(_ALL_ACTS):
            out.append(Case(U(*g, acts=(a, _ALL_ACTS[(i + 3) % 7])), k, want))
        for ap, po in ((HSWISH, NONE), (NONE, HSWISH), (RELU6, RELU), (RELU, RELU6)):
            out.append(Case(U(*g, acts=(HSWISH, HSWISH), act_p=ap, post=po, res="own"), k, want))
    out += [Case(U(8, 8, 8, 2, 3, 17, 33, acts=(SWISH, SWISH)), "mbw8", "mbw"), Case(U(40, 40, 64, 1, 2, 9, 17, acts=(HSWISH, RELU)), "mbw", "mbw"),
            Case(U(40, 40, 24, 2, 2, 17, 49, acts=(NONE, HSWISH), expand=False), "blk", "blk")]
    for g in ((8, 8, 8, 1, 2, 8, 15), (24, 40, 24, 1, 3, 15, 15), (24, 40, 64, 1, 2, 9, 15), (24, 40, 24, 2, 3, 17, 30), (8, 24, 40, 2, 2, 16, 29),
              (40, 40, 64, 1, 2, 9, 15), (64, 40, 96, 1, 2, 10, 15), (72, 40, 72, 1, 2, 11, 15)):
        for a in ((R6, R6), (R, R)):
            out.append(Case(U(*g, acts=a, res="own", post=(RELU if a[0] == R else NONE)), "mbr", "mbr"))
    return list(dict.fromkeys(out))


EXACT, BOUNDED = _exact_cases(), _bounded_cases()


def case_id(c):
    u = c.u
    s = "{}_n{}_{}x{}_{}-{}-{}_s{}_a{}{}{}{}".format(c.k, u.N, u.H, u.W, u.Cin if u.expand else "x", u.Cmid, u.Cout, u.stride, u.act_e,
                                                 u.act_d, u.act_p, u.post)
    return s + ("_r" + u.res if u.res else "")


def seed_of(u):
    return zlib.crc32(repr(tuple(u)).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=16)
def exact_reference(u, dtype):
    ops = exact_operands(u, seed_of(u))
    return ops, exact_result(u, ops, dtype)


@functools.lru_cache(maxsize=16)
def bounded_reference(u, dtype):
    ops = bounded_operands(u, dtype, seed_of(u))
    y, bound, _, _ = unit_ref(u, ops, dtype)
    return ops, y, bound


# ---- launching --------------------------------------------------------------------------------------------------------------------------
def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def make_descs(u, dtype):
    """(d_exp or None, d_dw, d_proj)"""
    from pytorchcv_amd._lib import ConvDesc
    Ho, Wo = out_hw(u)

    def desc(H, W, Cin, Cout, k, s, groups, act, post=NONE, res=False):
        d = ConvDesc()
        d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw = u.N, H, W, Cin, Cout, k, k
        d.stride_h = d.stride_w = s
        d.pad_t = d.pad_l = d.pad_b = d.pad_r = k // 2
        d.dil_h = d.dil_w = 1
        d.groups, d.act, d.post_act, d.has_residual = groups, act, post, int(res)
        d.dtype = d.out_dtype = CODE[dtype]
        d.x_cpitch, d.x_wpitch, d.y_cpitch = Cin, W, 0
        return d
    de = desc(u.H, u.W, u.Cin, u.Cmid, 1, 1, 1, u.act_e) if u.expand else None
    dd = desc(u.H, u.W, u.Cmid, u.Cmid, 3, u.stride, u.Cmid, u.act_d)
    dp = desc(Ho, Wo, u.Cmid, u.Cout, 1, 1, 1, u.act_p, u.post, u.res is not None)
    return de, dd, dp


def _byref(d):
    return ctypes.byref(d) if d is not None else None


class Launch(object):
    """one unit on the device: the three packed blobs, the operands, and `run()` into a fresh NaN-filled y with its guard tail"""
    def __init__(self, u, dtype, ops, dev):
        lb, L, ctx = _lib()
        self.u, self.dtype, self.dev = u, dtype, dev
        self.de, self.dd, self.dp = make_descs(u, dtype)

        def pack(d, w, dw):
            if d is None:
                return None
            n = ctypes.c_size_t(0)
            lb.check((L.pcv_dwconv_packed_bytes if dw else L.pcv_conv_packed_bytes)(ctypes.byref(d), ctypes.byref(n)), None)
            blob = torch.zeros(n.value + 16, dtype=torch.uint8, device=dev)
            wd = w.to(dev).contiguous()
            lb.check((L.pcv_dwconv_pack if dw else L.pcv_conv_pack)(ctx, ctypes.byref(d), _p(wd), _p(blob), _stream()), ctx)
            torch.cuda.synchronize()
            return blob
        self.pe, self.pd, self.pp = pack(self.de, ops.w_exp, False), pack(self.dd, ops.w_dw, True), pack(self.dp, ops.w_proj, False)
        f = lambda t: t.to(dev).contiguous() if t is not None else None          # noqa: E731
        self.bn = [f(t) for t in (ops.scale_e, ops.shift_e, ops.scale_d, ops.shift_d, ops.scale_p, ops.shift_p)]
        self.x = ops.x.to(dev, TDT[dtype]).contiguous()
        res = residual_of(u, ops)
        self.res = self.x if u.res == "x" else (res.to(dev, TDT[dtype]).contiguous() if res is not None else None)
        self.oshape = (u.N,) + out_hw(u) + (u.Cout,)

    def call(self, y, x=None, de="same", dd=None):
        """the return code of pcv_mbconv_fused (x / d_exp / d_dw replaceable: the refusal tests)"""
        lb, L, ctx = _lib()
        de = self.de if de == "same" else de
        se, he, sd, hd, sp, hp = self.bn
        return L.pcv_mbconv_fused(ctx, _byref(de), ctypes.byref(dd or self.dd), ctypes.byref(self.dp), x or _p(self.x), _p(self.pe), _p(se),
                                  _p(he), _p(self.pd), _p(sd), _p(hd), _p(self.pp), _p(sp), _p(hp), _p(self.res), y, _stream())

    def run(self):
        lb, L, ctx = _lib()
        n = int(np.prod(self.oshape))
        ybuf = torch.full((n + 256 * self.u.Cout + 64,), float("nan"), dtype=TDT[self.dtype], device=self.dev)     # tail: a 16 x 16 tile and more
        lb.check(self.call(_p(ybuf)), ctx)
        torch.cuda.synchronize()
        return ybuf[:n].view(self.oshape), ybuf[n:]


_STATS = os.environ.get("PCV_MBCONV_SWEEP_STATS")      # a file name: one JSON line per comparison (measurements, nothing is asserted from them)


def where(idx, shape, rt):
    """(n, ho, wo, c), border or interior, and the position inside the kernel's RO x OC tile"""
    n, ho, wo, ch = [int(v) for v in np.unravel_index(idx, shape)]
    border = ho in (0, shape[1] - 1) or wo in (0, shape[2] - 1)
    return "(n {}, ho {}, wo {}, c {}) - {} - row {} of {}, column {} of {} of its {} tile, channel {} of its 32-channel block".format(
        n, ho, wo, ch, "on a border" if border else "interior", ho % rt.RO, rt.RO, wo % rt.OC, rt.OC, rt.kernel, ch % 32)


def check_exact(out, want, what, rt):
    out, want = out.cpu(), want
    if torch.equal(out, want):
        return
    bad = ~(out.float() == want.float())                # NaN (an element nobody wrote) counts as a failure
    first = int(torch.where(bad.flatten())[0][0])
    pytest.fail("{}: {} of {} elements differ; first at {} - got {!r}, want {!r}".format(
        what, int(bad.sum()), bad.numel(), where(first, tuple(want.shape), rt), float(out.flatten()[first]), float(want.flatten()[first])))


def check_bounded(out, ref, bound, what, rt, dtype):
    err = (out.double().cpu() - ref).abs()
    ratio = err / bound
    if _STATS:
        with open(_STATS, "a") as f:
            f.write(json.dumps(dict(family="bounded", kernel=rt.kernel, dtype=dtype, case=what, ratio=float(ratio.nan_to_num(nan=1e30).max()))) + "\n")
    bad = ~(err <= bound)
    if bool(bad.any()):
        worst = int(torch.where(bad, ratio.nan_to_num(nan=float("inf")), torch.zeros_like(ratio)).argmax())
        pytest.fail("{}: {} of {} elements out of bound; worst at {} - got {:.6e}, ref {:.6e}, bound {:.3e}".format(
            what, int(bad.sum()), bad.numel(), where(worst, tuple(ref.shape), rt), float(out.flatten()[worst]), float(ref.flatten()[worst]),
            float(bound.flatten()[worst])))


def _routed(c):
    """the first assertion of every test: the unit is accepted and this case runs the kernel it names"""
    assert unsupported(c.u) is None, unsupported(c.u)
    rt = route(c.u, c.k)
    assert rt.kernel == c.want, rt
    if c.k == "mbr_nx":
        assert rt.inst[-1] is False and route(c.u, "mbr").inst[-1] is True, rt          # the x-through-LDS instance was the first choice
    if c.k in ("mbw8", "mbw16"):
        assert rt.tw == int(c.k[3:]), rt
    return rt


def _params(cases):
    return [pytest.param(c, dt, id=case_id(c) + "-" + dt) for c in cases for dt in DTYPES16]


@pytest.mark.parametrize("c,dtype", _params(EXACT))
def test_exact_family_equals_float64_bit_for_bit(c, dtype, cuda_device):
    rt = _routed(c)
    lb, L, ctx = _lib()
    d = make_descs(c.u, dtype)
    assert L.pcv_mbconv_supported(_byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2])) == 1
    ops, want = exact_reference(c.u, dtype)
    run = Launch(c.u, dtype, ops, cuda_device)
    for g in GRIDS:
        what = "exact {} {} grid {}".format(case_id(c), dtype, g)
        with util.tuning(max_blocks=g, **SWITCHES[c.k]):
            out, tail = run.run()
        assert bool(torch.isnan(tail).all()), what + ": the guard tail behind y was written"
        check_exact(out, want, what, rt)
        if _STATS:
            with open(_STATS, "a") as f:
                f.write(json.dumps(dict(family="exact", kernel=rt.kernel, dtype=dtype, case=what, ratio=0.0)) + "\n")


@pytest.mark.parametrize("c,dtype", _params(BOUNDED))
def test_bounded_family_inside_the_derived_bound(c, dtype, cuda_device):
    rt = _routed(c)
    ops, ref, bound = bounded_reference(c.u, dtype)
    run = Launch(c.u, dtype, ops, cuda_device)
    for g in GRIDS:
        what = "bounded {} {} grid {}".format(case_id(c), dtype, g)
        with util.tuning(max_blocks=g, **SWITCHES[c.k]):
            out, tail = run.run()
        assert bool(torch.isnan(tail).all()), what + ": the guard tail behind y was written"
        check_bounded(out, ref, bound, what, rt, dtype)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
_OK = U(24, 40, 24, 1, 2, 9, 17)
REFUSED = {"cmid_not_8": _OK._replace(Cmid=44), "cout_104": _OK._replace(Cin=64, Cout=104), "wo_13": _OK._replace(W=13),
           "ho_7": _OK._replace(H=7)}


@pytest.mark.parametrize("which", sorted(REFUSED) + ["dw_pad_0", "fp32", "stale_desc", "unaligned_x"])
def test_unsupported_units_are_refused_and_nothing_is_launched(which, cuda_device):
    """PCV_ERR_INVALID, and y keeps all its NaNs"""
    lb, L, ctx = _lib()
    assert unsupported(_OK) is None
    bad = REFUSED.get(which, _OK)
    if which in REFUSED:
        assert unsupported(bad) is not None
    ok = Launch(_OK, "bf16", exact_operands(_OK, 1), cuda_device)           # live blobs and constants, large enough for every variant
    run = ok
    if which in REFUSED:
        run = Launch.__new__(Launch)
        run.__dict__.update(ok.__dict__)
        run.u = bad
        run.de, run.dd, run.dp = make_descs(bad, "bf16")
        run.x = torch.zeros((bad.N, bad.H, bad.W, bad.Cin), dtype=torch.bfloat16, device=cuda_device)
        big = torch.zeros(1 << 18, dtype=torch.uint8, device=cuda_device)
        run.pe = run.pd = run.pp = big
        run.bn = [torch.zeros(1024, device=cuda_device)] * 6
    y = torch.full((1 << 16,), float("nan"), dtype=torch.bfloat16, device=cuda_device)
    kw = {}
    if which == "dw_pad_0":
        dd = make_descs(_OK, "bf16")[1]
        dd.pad_t = dd.pad_l = dd.pad_b = dd.pad_r = 0
        kw = dict(dd=dd)
    elif which == "fp32":
        run = Launch.__new__(Launch)
        run.__dict__.update(ok.__dict__)
        run.de, run.dd, run.dp = make_descs(_OK, "fp32")
        assert unsupported(_OK, "fp32") is not None
    elif which == "stale_desc":
        dd = make_descs(_OK, "bf16")[1]
        dd.struct_size -= 4
        kw = dict(dd=dd)
    elif which == "unaligned_x":
        xb = torch.zeros(ok.x.numel() + 8, dtype=torch.bfloat16, device=cuda_device)
        kw = dict(x=ctypes.c_void_p(xb.data_ptr() + 2))
    assert run.call(_p(y), **kw) == PCV_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
