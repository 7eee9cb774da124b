"""
GPU sweep of the two kernels every dedicated dense kernel is compared with bit for bit - the generic implicit GEMM
(csrc/igemm_conv.hpp) and the stem kernel (csrc/stem_conv.hpp) - and of the two grouped 3x3 kernels against the float64 reference and the derived bound of
tests/conv_ref.py (tests/test_conv_ref_bounds.py proves on the CPU that the reference equals torch's float64 convolution, that an
emulated fp32 kernel stays inside the bound for every case below and that plausible kernel bugs leave it).

The sweep drives the C ABI directly (its own pcv_conv_desc, pcv_conv_packed_bytes / pcv_conv_pack, pcv_conv2d_fused and its
siblings), which reaches what the engine never sets: x_wpitch, x_cpitch, y_cpitch, out_dtype, ragged Cout, unequal strides and
dilations. Families:
  F1  table mode (KHW == 0: taps from ktab, 16 + 16-bit row / column mask), dense - every kernel size but 1x1 / 3x3, dilation, 1x1
      with padding, 3x3 with a ragged channel count, pitches wider than the tensor, unequal strides - plus the epilogue variants and
      the forced tiles / non-persistent launch / weight-stationary switch on all three tap modes
  F2  block-diagonal grouped convolution on the generic kernel (gpb group blocking, ngb > 1, cin_blk offsets)
  F3  the "special" instantiations: ragged Cout, fp32 output from 16-bit input, pcv_gemm_bias
  F4  the pixel-pair scheme on the generic kernel (x_cpitch 4 at 16 bit and not a stem shape)
  F5  the stem kernel: plain, fused max-pool, from fp32 NCHW, both
  F6  grouped 3x3 on the flat kernel (csrc/gconv3x3.hpp), F7 on the row kernel (csrc/gconv3x3r.hpp) - the only two families that set no
      switch: the library's own routing, restated in `plan` (route_conv's gconv_ok, plan_gconvr) and asserted first
Every case runs on the resident grid and under max_blocks = 8 (several tiles per block through the cross-tile pipeline), into a
NaN-filled output with a guard tail of at least one 256-pixel tile: an element nobody wrote fails the comparison, a write outside
the tensor (or outside the channel slice of a wider y) fails the guard check. The first assertion of each family restates
plan_conv's / route_igemm's own conditions (`plan` below), so that a routing change cannot silently move a case onto another kernel.
Tuples are (N, Cin, Cout, H, W, kernel, stride, pad (t, l, b, r), dilation).
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
from conv_ref import Geom, conv_ref_bound, operands, out_hw, pool_out_hw, pool_ref_bound, storage_normal
from test_gpu_dw_se import CODE, HSIGMOID, HSWISH, NONE, RELU, RELU6, SIGMOID, SWISH, TDT

pytestmark = pytest.mark.gpu

GRIDS = [0, 8]
DTYPES = ("fp32", "bf16", "fp16")
DTYPES16 = ("bf16", "fp16")
PCV_ERR_INVALID = -1
GENERIC = dict(d3x3=0, d1x1=0, d1i=0, gconvr=0, head=0)       # keep every dedicated dense kernel away
TILES = {0: (32, 256), 1: (64, 256), 2: (128, 128), 3: (256, 64), 4: (64, 128), 5: (128, 64)}      # kTiles: (BM, BP)

_FIELDS = ("N Cin Cout H W kh kw sh sw pt pl pb pr dh dw groups act post res gate cpitch wpitch yslice out_f32 tune entry khw khw32 "
           "special note")
Case = collections.namedtuple("Case", _FIELDS)


def _two(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def C(N, Cin, Cout, H, W, k=3, s=1, p=None, d=1, groups=1, act=RELU, post=NONE, res=False, gate=False, cpitch=0, wpitch=0,
      yslice=None, out_f32=False, tune=(), entry="conv", khw=0, khw32=None, special=False, note=""):
    """k / s / d: an int or (h, w); p: an int or (top, left, bottom, right); khw / khw32: the tap mode this case is meant to run in
    (16-bit / fp32 storage); tune: extra pcv_set_tuning switches as a dict"""
    kh, kw = _two(k)
    sh, sw = _two(s)
    dh, dw = _two(d)
    if p is None:
        p = (dh * (kh - 1) // 2, dw * (kw - 1) // 2) * 2
    pt, pl, pb, pr = (p,) * 4 if isinstance(p, int) else p
    tune = tuple(sorted(dict(tune).items()))
    return Case(N, Cin, Cout, H, W, kh, kw, sh, sw, pt, pl, pb, pr, dh, dw, groups, act, post, res, gate, cpitch, wpitch, yslice,
                out_f32, tune, entry, khw, khw if khw32 is None else khw32, special, note)


def geom_of(c):
    return Geom(c.kh, c.kw, c.sh, c.sw, c.pt, c.pl, c.pb, c.pr, c.dh, c.dw, c.groups, c.Cin)


def case_id(c):
    s = "n{}_{}to{}_{}x{}_k{}x{}_s{}{}_p{}{}{}{}_d{}{}".format(c.N, c.Cin, c.Cout, c.H, c.W, c.kh, c.kw, c.sh, c.sw, c.pt, c.pl,
                                                              c.pb, c.pr, c.dh, c.dw)
    if c.groups > 1:
        s += "_g{}".format(c.groups)
    s += "_a{}{}".format(c.act, c.post) + ("r" if c.res else "") + ("g" if c.gate else "")
    if c.cpitch:
        s += "_cp{}".format(c.cpitch)
    if c.wpitch:
        s += "_wp{}".format(c.wpitch)
    if c.yslice:
        s += "_ys"
    if c.out_f32:
        s += "_of32"
    if c.entry != "conv":
        s += "_" + c.entry
    for k, v in c.tune:
        s += "_{}{}".format(k, v)
    return s


# ---- plan_conv / route_igemm restated (csrc/pcv_api.hip) ----------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "ok pair stem conv3 gconv gpb ngb cin_blk cout_blk special khw nk tile nPixTiles nChTiles Ho Wo "
                              "gkernel R XH wrows")
K_GCONVR_MAX_LDS = 160 * 1024        # kGconvRMaxLds


def plan_gconvr(stride, H, W, Ho, Wo):
    """plan_gconvr: (R output rows per tile, XH, window rows in LDS), or None where the row-tile kernel does not take the map"""
    if stride == 2 and ((H | W) & 1):
        return None
    if Wo > 64 or Ho <= 0:
        return None
    for R in range(64 // Wo, 0, -1):
        win = (2 * R + 1) * W + 2 if stride == 2 else (R + 2) * W + 2
        XH = ((win + 1) // 2 + 7) // 8 * 8 if stride == 2 else 0
        rows = ((2 * XH if stride == 2 else win) + 31) // 32 * 32
        lds = 2 * rows * 128
        if lds * 2 <= K_GCONVR_MAX_LDS or (R == 1 and lds <= K_GCONVR_MAX_LDS):
            return R, XH, rows
    return None


def plan(c, dtype):
    ES = 4 if dtype == "fp32" else 2
    CE = 16 // ES
    cpitch = c.cpitch or c.Cin
    cgi, cgo = c.Cin // c.groups, c.Cout // c.groups
    pair = c.groups == 1 and cpitch == 4 and ES == 2
    gpb, ok = 1, True
    if c.groups > 1:
        while gpb < c.groups and ((gpb * cgo) % 8 != 0 or (gpb * cgi) % CE != 0 or gpb * cgo < 32):
            gpb += 1
        while gpb < c.groups and c.groups % gpb != 0:
            gpb += 1
        ok = c.groups % gpb == 0 and (gpb * cgo) % 8 == 0 and (gpb * cgi) % CE == 0
    ok = ok and (pair or cpitch % CE == 0)
    ngb = c.groups // gpb if ok else 0
    cin_blk = c.Cin if c.groups == 1 else gpb * cgi
    cout_blk = gpb * cgo
    out_same = not c.out_f32 or dtype == "fp32"
    k33 = (c.kh, c.kw) == (3, 3)
    d11 = (c.dh, c.dw) == (1, 1)
    pads = (c.pt, c.pl, c.pb, c.pr)
    conv3 = (c.groups == 1 and k33 and (c.sh, c.sw) == (1, 1) and d11 and pads == (1, 1, 1, 1) and c.Cin % (8 * CE) == 0 and
             cpitch == c.Cin and c.wpitch in (0, c.W) and out_same and c.Cout % 8 == 0)
    stem = (pair and (c.sh, c.sw) == (2, 2) and c.dh == 1 and c.Cout <= 64 and c.Cout % 8 == 0 and c.kh <= 7 and
            c.kw + (c.pl & 1) <= 8 and out_same)
    gconv = (c.groups > 1 and k33 and c.sh == c.sw and c.sh in (1, 2) and d11 and pads == (1, 1, 1, 1) and c.Cin == c.Cout and
             c.Cin % 64 == 0 and ES == 2 and cgi in (4, 8, 16, 32) and out_same)
    special = c.Cout % 8 != 0 or cout_blk % 8 != 0 or not out_same
    khw = 0
    if not special and not pair and d11:
        if (c.kh, c.kw) == (1, 1) and pads == (0, 0, 0, 0):
            khw = 1
        elif k33 and cin_blk % (8 * CE) == 0:
            khw = 9
    if pair:
        nchunks = c.kh * ((c.kw + (c.pl & 1) + 1) // 2)
    else:
        nchunks = c.kh * c.kw * ((cin_blk + CE - 1) // CE)
    nk = (nchunks + 7) // 8
    if special:
        tile = 2
    elif cout_blk <= 32:
        tile = 0
    elif cout_blk <= 64:
        tile = 1
    elif cout_blk <= 128:
        tile = 2
    elif cout_blk <= 256:
        tile = 2 if c.kh * c.kw > 1 else 3
    else:
        tile = 2
    if khw == 1:
        if tile == 1 and c.Cin >= 256:
            tile = 4
        elif tile == 2 and cout_blk <= 128 and c.Cin >= 512:
            tile = 5
        elif tile == 3 and c.Cin > 128:
            tile = 2
        if c.act in (SWISH, SIGMOID) and nk <= 2 and ngb == 1 and not c.res:
            tile = 4 if (cout_blk + 63) // 64 * 64 < (cout_blk + 127) // 128 * 128 else 5
    forced = dict(c.tune).get("tile", -1)
    if 0 <= forced < 6 and not special and (forced < 4 or khw == 1):
        tile = forced
    Ho, Wo = out_hw(c.H, c.W, geom_of(c))
    BM, BP = TILES[tile]
    # route_conv: the two grouped 3x3 kernels in front of the generic one
    gconv_ok = (gconv and not c.gate and not c.yslice and not c.res and c.post == NONE and cpitch == c.Cin and c.wpitch in (0, c.W) and
                c.N * Ho * Wo * c.Cin * 2 < 1 << 31)
    gkernel, rows = "generic", None
    if gconv_ok and dict(c.tune).get("gconvr", 1) != 0 and (c.sh == 2 or cgi == 32):
        rows = plan_gconvr(c.sh, c.H, c.W, Ho, Wo)
    if rows:
        gkernel = "rows"
    elif gconv_ok and c.sh == 1 and cgi != 32 and c.W <= 63:
        gkernel = "flat"
    R, XH, wrows = rows or (0, 0, 0)
    return Plan(ok, pair, stem, conv3, gconv, gpb, ngb, cin_blk, cout_blk, special, khw, nk, tile, (c.N * Ho * Wo + BP - 1) // BP,
                (cout_blk + BM - 1) // BM, Ho, Wo, gkernel, R, XH, wrows)


# ---- F1: table mode, dense ------------------------------------------------------------------------------------------------------------
_BIG = (9, 8, 200, 13, 11)          # several pixel tiles with a tail on every tile shape (M = 1287), two or more channel tiles
_EPI_A = dict(N=2, Cin=24, Cout=40, H=13, W=11, k=5)
_EPI_B = dict(N=3, Cin=16, Cout=24, H=10, W=14, k=4, s=2, p=1)
_ACTS = (NONE, RELU, RELU6, SIGMOID, SWISH, HSIGMOID, HSWISH)

F1_GEOMETRY = [
    C(2, 24, 40, 13, 11, k=5),
    C(1, 16, 32, 9, 10, k=7),
    C(2, 32, 48, 9, 17, k=(1, 7), p=(0, 3, 0, 3)),
    C(2, 32, 48, 9, 17, k=(7, 1), p=(3, 0, 3, 0)),
    C(3, 16, 24, 10, 14, k=2, s=2, p=0),
    C(3, 16, 24, 10, 14, k=4, s=2, p=1),
    C(2, 32, 32, 12, 12, d=2, p=2),
    C(2, 32, 32, 9, 7, d=(1, 3), p=(1, 3, 1, 3), note="the dilated extent equals W: almost every column tap is masked"),
    C(2, 32, 32, 7, 7, d=4, p=4),
] + [
    C(2, (16, 24)[(i + j) % 2], 32, H, W, s=2, p=p)
    for i, (H, W) in enumerate([(15, 15), (14, 9), (8, 8)]) for j, p in enumerate([(0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 1, 1)])
] + [
    C(2, 32, 32, 11, 13, s=(2, 1), khw32=9),
    C(2, 32, 32, 11, 13, s=(1, 2), khw32=9),
    C(1, 8, 16, 5, 6, p=3, note="padding wider than the kernel: border outputs see only zeros"),
    C(2, 32, 64, 6, 7, k=1, p=1),
    C(2, 3, 64, 9, 9, cpitch=8, note="VGG conv1"),
    C(2, 58, 58, 14, 14, cpitch=64, special=True, note="ShuffleNet width: ragged Cout too, so the 128 x 128 descriptor-driven variant"),
    C(*_BIG),
    C(2, 64, 32, 7, 7, k=1, cpitch=160, khw=1, note="DenseNet form: live data behind the slice"),
    C(2, 64, 32, 7, 7, k=3, cpitch=160, khw=9, note="DenseNet form; the computed-tap mode with a channel pitch"),
    C(2, 16, 16, 7, 9, wpitch=10, note="finite garbage in the pad column"),
]
F1_EPILOGUE = (
    [C(act=a, **_EPI_A) for a in _ACTS] + [C(act=a, **_EPI_B) for a in _ACTS] +
    [C(act=a, post=p, res=True, **_EPI_A) for a, p in ((NONE, NONE), (RELU, RELU), (NONE, RELU6), (SWISH, HSWISH))] +
    [C(act=a, post=p, res=True, **_EPI_B) for a, p in ((HSWISH, NONE), (NONE, RELU), (RELU6, RELU6), (NONE, HSWISH))] +
    [C(yslice=(40, 72), **_EPI_A), C(yslice=(40, 72), res=True, post=RELU, act=NONE, **_EPI_B),
     C(2, 24, 40, 13, 11, gate=True, res=True, act=NONE, post=RELU), C(2, 24, 40, 13, 11, gate=True, act=HSWISH)])
F1_TILES = (
    [C(*_BIG, tune=dict(tile=t, persist=ps)) for t in range(4) for ps in (1, 0)] +
    [C(9, 64, 200, 13, 11, khw=9, tune=dict(tile=t, persist=ps)) for t in range(4) for ps in (1, 0)] +
    [C(9, 72, 200, 13, 11, k=1, khw=1, tune=dict(tile=t, persist=ps), note="zero-filled chunk beyond Cin") for t in range(6) for ps in (1, 0)] +
    [C(9, 32, 64, 13, 11, k=1, khw=1, tune=dict(wstat=ws), note="one K-step, one channel tile: weight-stationary") for ws in (1, 0)])
F1 = list(dict.fromkeys(F1_GEOMETRY + F1_EPILOGUE + F1_TILES))          # (the ReLU rows of the epilogue list repeat two geometry rows)

# ---- F2: grouped on the generic kernel --------------------------------------------------------------------------------------------------
# (groups, Cin, Cout, kernel, stride, gpb, tap mode)
_F2_LAYERS = [(4, 32, 64, 3, 1, 2, 0), (3, 48, 96, 3, 2, 1, 0), (8, 64, 64, 5, 1, 4, 0), (2, 128, 128, 3, 2, 1, 9), (2, 128, 64, 1, 1, 1, 1)]
F2 = [C(3, ci, co, H, W, k=k, s=s, groups=g, khw=khw, act=(RELU, NONE)[i % 2]) for i, (g, ci, co, k, s, gpb, khw) in enumerate(_F2_LAYERS)
      for (H, W) in ((9, 7), (14, 14))]
F2_GPB = {(g, ci, co): gpb for (g, ci, co, k, s, gpb, khw) in _F2_LAYERS}

# ---- F3: special instantiations -----------------------------------------------------------------------------------------------------------
F3_RAGGED = [C(5, 32, co, 7, 9, k=k, special=True, act=(NONE, RELU, HSWISH)[i % 3]) for i, co in enumerate((10, 100, 138)) for k in (1, 3)]
F3_F32OUT = [C(5, 32, co, 7, 9, k=k, out_f32=True, special=True, res=r, post=RELU if r else NONE, act=NONE if r else RELU)
             for co in (64, 136) for k in (1, 3) for r in (False, True)]
F3_GEMM = [C(33, 72, co, 1, 1, k=1, out_f32=True, special=True, act=NONE, entry="gemm") for co in (10, 136)]

# ---- F4: pixel pairs on the generic kernel (16 bit, x_cpitch 4, even x_wpitch) --------------------------------------------------------------
F4 = [
    C(2, 3, 96, 10, 14, s=2, p=1, cpitch=4),
    C(1, 3, 72, 33, 35, k=7, s=2, p=3, cpitch=4, wpitch=36),
    C(2, 4, 32, 9, 9, s=(1, 2), p=1, cpitch=4, wpitch=10, note="pad column live-zero"),
    C(2, 1, 32, 33, 35, s=(4, 2), p=1, cpitch=4, wpitch=36),
    C(2, 3, 32, 10, 14, s=2, d=(2, 1), p=(2, 1, 2, 1), cpitch=4),
    C(1, 4, 40, 33, 35, k=(9, 3), s=2, p=(4, 1, 4, 1), cpitch=4, wpitch=36),
    C(2, 3, 32, 9, 9, s=2, p=1, cpitch=4, wpitch=10, out_f32=True, special=True, note="a stem shape but for its fp32 output"),
    C(2, 3, 96, 9, 9, k=5, s=2, p=2, cpitch=4, wpitch=10, note="even pad_l: no leading half pair"),
    C(3, 1, 72, 10, 14, k=(3, 7), s=2, p=(0, 2, 1, 3), cpitch=4, act=HSWISH),
]

# ---- F5: stem kernel (16 bit) -----------------------------------------------------------------------------------------------------------------
# (entry, (kh, kw), (pad t, l, b, r), Cin, Cout, (H, W), N, act, stem32)
_STEM = [
    ("conv", (3, 3), (1, 1, 1, 1), 3, 32, (33, 35), 3, RELU, 1), ("conv", (7, 7), (3, 3, 3, 3), 3, 64, (31, 33), 1, RELU, 1),
    ("conv", (5, 5), (0, 2, 1, 3), 1, 8, (5, 7), 3, RELU6, 0), ("conv", (1, 1), (0, 0, 0, 0), 2, 24, (2, 2), 1, NONE, 1),
    ("conv", (2, 2), (0, 1, 0, 1), 4, 40, (32, 32), 3, HSWISH, 1), ("conv", (4, 4), (1, 1, 1, 1), 3, 32, (20, 70), 1, SWISH, 0),
    ("conv", (6, 6), (3, 5, 2, 0), 4, 64, (33, 35), 1, SIGMOID, 1), ("conv", (3, 7), (1, 3, 1, 3), 2, 24, (1, 40), 3, HSIGMOID, 1),
    ("conv", (7, 3), (4, 0, 3, 1), 1, 8, (31, 33), 1, RELU, 1), ("conv", (7, 1), (3, 0, 3, 0), 3, 40, (5, 7), 3, RELU6, 1),
    ("conv", (3, 3), (0, 1, 0, 1), 3, 32, (32, 32), 1, RELU, 0), ("conv", (5, 5), (4, 5, 1, 2), 4, 64, (20, 70), 1, NONE, 1),
    ("conv", (7, 7), (3, 3, 3, 3), 3, 64, (2, 2), 3, RELU, 1),
] + [("conv", (3, 3), (1, 1, 1, 1), 3, 24, (5, 7), 1, a, 1) for a in _ACTS] + [
    ("pool", (7, 7), (3, 3, 3, 3), 3, 64, (33, 35), 3, RELU, 1), ("pool", (3, 3), (1, 1, 1, 1), 4, 32, (31, 33), 1, RELU6, 1),
    ("pool", (5, 5), (0, 2, 1, 3), 1, 8, (20, 70), 1, RELU, 1), ("pool", (1, 1), (0, 0, 0, 0), 2, 24, (5, 7), 3, RELU, 1),
    ("pool", (2, 2), (0, 1, 0, 1), 3, 40, (32, 32), 1, RELU6, 1), ("pool", (4, 4), (3, 5, 0, 0), 4, 64, (1, 40), 3, RELU, 1),
    ("pool", (6, 6), (4, 3, 1, 2), 2, 8, (2, 2), 1, RELU, 1), ("pool", (3, 7), (1, 3, 1, 3), 1, 24, (33, 35), 1, RELU6, 1),
    ("pool", (7, 3), (3, 0, 3, 1), 3, 40, (31, 33), 3, RELU, 1), ("pool", (7, 1), (3, 0, 3, 0), 2, 32, (20, 70), 1, RELU, 1),
    ("pool", (5, 5), (4, 2, 0, 2), 3, 64, (5, 7), 1, RELU, 1), ("pool", (3, 3), (0, 1, 0, 1), 3, 32, (32, 32), 3, RELU, 1),
    # from fp32 NCHW: at most 3 planes and W % 4 == 0, so (5, 8) and (33, 36) stand in for the maps of the list above that are not
    ("nchw", (3, 3), (1, 1, 1, 1), 3, 32, (32, 32), 3, RELU, 1), ("nchw", (7, 7), (3, 3, 3, 3), 3, 64, (33, 36), 1, RELU, 1),
    ("nchw", (5, 5), (0, 2, 1, 3), 1, 8, (5, 8), 3, RELU6, 0), ("nchw", (1, 1), (0, 0, 0, 0), 2, 24, (1, 40), 1, NONE, 1),
    ("nchw", (2, 2), (0, 1, 0, 1), 3, 40, (32, 32), 1, HSWISH, 1), ("nchw", (4, 4), (1, 5, 1, 0), 2, 32, (33, 36), 1, SWISH, 0),
    ("nchw", (6, 6), (3, 3, 2, 2), 1, 64, (5, 8), 1, SIGMOID, 1), ("nchw", (3, 7), (1, 3, 1, 3), 2, 24, (1, 40), 3, HSIGMOID, 1),
    ("nchw", (7, 3), (4, 0, 3, 1), 1, 8, (33, 36), 1, RELU, 1), ("nchw", (7, 1), (3, 0, 3, 0), 3, 40, (32, 32), 3, RELU6, 1),
    ("nchw", (3, 3), (0, 1, 0, 1), 3, 32, (5, 8), 1, RELU, 1), ("nchw", (5, 5), (4, 5, 1, 2), 3, 64, (32, 32), 1, RELU, 1),
    ("nchw_pool", (7, 7), (3, 3, 3, 3), 3, 64, (32, 32), 3, RELU, 1), ("nchw_pool", (3, 3), (1, 1, 1, 1), 2, 32, (33, 36), 1, RELU6, 1),
    ("nchw_pool", (5, 5), (0, 2, 1, 3), 1, 8, (5, 8), 1, RELU, 1), ("nchw_pool", (1, 1), (0, 0, 0, 0), 2, 24, (1, 40), 3, RELU, 1),
    ("nchw_pool", (2, 2), (0, 1, 0, 1), 3, 40, (32, 32), 1, RELU6, 1), ("nchw_pool", (4, 4), (3, 5, 0, 0), 1, 64, (1, 40), 1, RELU, 1),
    ("nchw_pool", (6, 6), (4, 3, 1, 2), 2, 8, (5, 8), 3, RELU, 1), ("nchw_pool", (3, 7), (1, 3, 1, 3), 1, 24, (33, 36), 1, RELU, 1),
    ("nchw_pool", (7, 3), (3, 0, 3, 1), 3, 40, (32, 32), 1, RELU6, 1), ("nchw_pool", (7, 1), (3, 0, 3, 0), 2, 32, (33, 36), 3, RELU, 1),
    ("nchw_pool", (5, 5), (4, 1, 0, 2), 3, 64, (5, 8), 1, RELU, 1),
]
F5 = [C(N, ci, co, H, W, k=k, s=2, p=p, act=a, cpitch=4, wpitch=W + (W & 1), entry=e, tune=dict(stem32=s32) if co <= 32 else ())
      for (e, k, p, ci, co, (H, W), N, a, s32) in _STEM]

# ---- F6: grouped 3x3 on the flat kernel (csrc/gconv3x3.hpp: 128-pixel tiles, stride 1, 4 / 8 / 16 channels per group, 16 bit) -------------
# (N, C, groups, H, W): every channels-per-group value in every halo class (W + 1 <= 16 / 32 / 64) and on the classes' edges, H = 1 / 3 / 9,
# images that end inside a 128-pixel tile, 1 / 9 / more than 16 tiles; C = 128: two channel blocks (the weights are loaded again)
_F6 = [(1, 64, 16, 1, 5), (3, 64, 8, 3, 15), (5, 64, 4, 9, 16), (4, 64, 16, 9, 31), (3, 64, 8, 3, 32), (4, 64, 4, 9, 63), (2, 64, 8, 1, 63),
       (7, 64, 4, 3, 5), (3, 64, 16, 9, 15), (9, 64, 16, 1, 16), (2, 64, 4, 9, 32), (2, 64, 16, 3, 32), (2, 64, 8, 9, 16), (3, 128, 8, 9, 31),
       (5, 128, 16, 9, 31)]
F6 = ([C(N, ch, ch, H, W, groups=g, act=(RELU, NONE, RELU6)[i % 3]) for i, (N, ch, g, H, W) in enumerate(_F6)] +
      [C(3, 64, 64, 3, 15, groups=8, act=a) for a in _ACTS])
F6_GENERIC = [C(2, 64, 64, 3, 64, groups=8, note="W = 64: wider than the flat kernel's halo rows")]

# ---- F7: grouped 3x3 on the row kernel (csrc/gconv3x3r.hpp: R whole output rows per tile; stride 2, and 32 channels per group) ---------------
# (N, C, groups, H, W, stride): even maps with Wo = 1 / 2 / 7 / 16 / 21 / 64, so that R = 64 / Wo is 64 / 32 / 9 / 4 / 3 / 1; N Ho is no multiple
# of R (a tile straddles two images) wherever R > 1
_F7 = [(3, 64, 16, 2, 2, 2), (3, 64, 8, 6, 4, 2), (2, 64, 4, 10, 14, 2), (3, 64, 2, 6, 32, 2), (2, 64, 16, 8, 42, 2), (3, 64, 8, 4, 128, 2),
       (2, 64, 2, 10, 14, 2), (2, 64, 16, 10, 14, 2), (3, 64, 8, 6, 32, 2), (3, 64, 4, 6, 32, 2), (2, 128, 4, 10, 14, 2),
       (3, 64, 2, 1, 1, 1), (3, 64, 2, 3, 2, 1), (2, 64, 2, 5, 7, 1), (3, 64, 2, 3, 16, 1), (2, 64, 2, 4, 21, 1), (3, 64, 2, 2, 64, 1),
       (2, 128, 4, 5, 7, 1)]
F7_R = {1: 64, 2: 32, 7: 9, 16: 4, 21: 3, 64: 1}            # Wo -> R
F7 = ([C(N, ch, ch, H, W, s=s, groups=g, act=(RELU, NONE, RELU6)[i % 3]) for i, (N, ch, g, H, W, s) in enumerate(_F7)] +
      [C(2, 64, 64, 10, 14, s=2, groups=4, act=a) for a in _ACTS])
F7_GENERIC = [C(2, 64, 64, 15, 15, s=2, groups=16, note="an odd map at stride 2: no parity split")]

FAMILIES = {"F1": (F1, DTYPES), "F2": (F2, DTYPES), "F3": (F3_RAGGED, DTYPES), "F3f": (F3_F32OUT + F3_GEMM, DTYPES16), "F4": (F4, DTYPES16),
            "F5": (F5, DTYPES16), "F6": (list(dict.fromkeys(F6)) + F6_GENERIC, DTYPES16), "F7": (list(dict.fromkeys(F7)) + F7_GENERIC, DTYPES16)}


def all_cases():
    """(family, case, dtype) of everything the sweep launches (tests/test_conv_ref_bounds.py walks the same list)"""
    return [(f, c, dt) for f, (cases, dts) in FAMILIES.items() for c in cases for dt in dts]


# ---- reference, once per (case, dtype) whatever the tuning switches ---------------------------------------------------------------------
def base_of(c):
    return c._replace(tune=(), note="", khw=0, khw32=0, special=False)


def seed_of(c):
    return zlib.crc32(repr(base_of(c)).encode()) & 0x7FFFFFFF


def case_operands(c, dtype):
    return operands(c.N, c.H, c.W, c.Cout, geom_of(c), dtype, seed_of(c), with_res=c.res, with_gate=c.gate)


def x_buffer(c, ops, dtype):
    """x as the kernel addresses it, [N][H][wpitch][cpitch] (fp32 tensor of storage-type values): live finite data in the pad column and
    behind the channel slice; zeros there for the padded 4-channel input, whose contract says so"""
    cp, wp = c.cpitch or c.Cin, c.wpitch or c.W
    if cp == 4:
        buf = torch.zeros((c.N, c.H, wp, cp))
    else:
        buf = storage_normal(seed_of(c), 7, (c.N, c.H, wp, cp), dtype)
    buf[:, :, :c.W, :c.Cin] = ops.x
    return buf


def case_reference(c, dtype):
    """(operands, reference, bound) of a case; the bias-only pcv_gemm_bias has scale 1"""
    ops = case_operands(c, dtype)
    if c.entry == "gemm":
        ops = ops._replace(scale=None)
    odt = "fp32" if c.out_f32 else dtype
    ref, bound = conv_ref_bound(ops.x, ops.w, ops.scale, ops.shift, geom_of(c), c.act, ops.res, c.post, ops.gate, out_dtype=odt)
    if c.entry in ("pool", "nchw_pool"):
        ref, bound = pool_ref_bound(ref, bound, dtype)
    return ops, ref, bound


@functools.lru_cache(maxsize=48)
def _cached_reference(base, dtype):
    return case_reference(base, dtype)


# ---- launching -------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def make_desc(c, dtype):
    from pytorchcv_amd._lib import ConvDesc
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw = c.N, c.H, c.W, c.Cin, c.Cout, c.kh, c.kw
    d.stride_h, d.stride_w, d.pad_t, d.pad_l, d.pad_b, d.pad_r, d.dil_h, d.dil_w = c.sh, c.sw, c.pt, c.pl, c.pb, c.pr, c.dh, c.dw
    d.groups, d.act, d.post_act, d.has_residual = c.groups, c.act, c.post, int(c.res)
    d.dtype = CODE[dtype]
    d.out_dtype = 0 if c.out_f32 else CODE[dtype]
    d.x_cpitch, d.x_wpitch = c.cpitch or c.Cin, c.wpitch or c.W
    d.y_cpitch = c.Cout + c.yslice[1] if c.yslice else 0
    return d


class Launch(object):
    """one case on the device: packed weights, operands, and `run()` into a fresh NaN-filled output with its guard tail"""
    def __init__(self, c, dtype, ops, dev):
        lb, L, ctx = _lib()
        self.c, self.dtype, self.dev = c, dtype, dev
        self.d = make_desc(c, dtype)
        n = ctypes.c_size_t(0)
        lb.check(L.pcv_conv_packed_bytes(ctypes.byref(self.d), ctypes.byref(n)), None)
        self.packed = torch.zeros(n.value + 16, dtype=torch.uint8, device=dev)
        w = ops.w.to(dev).contiguous()
        lb.check(L.pcv_conv_pack(ctx, ctypes.byref(self.d), _p(w), _p(self.packed), _stream()), ctx)
        if c.entry in ("nchw", "nchw_pool"):
            self.x = ops.x.permute(0, 3, 1, 2).contiguous().to(dev)            # fp32 [N][Cin][H][W] of storage-type values
        else:
            self.x = x_buffer(c, ops, dtype).to(dev, TDT[dtype]).contiguous()
        self.scale = ops.scale.to(dev) if ops.scale is not None else None
        self.shift = ops.shift.to(dev)
        self.res = ops.res.to(dev, TDT[dtype]).contiguous() if ops.res is not None else None
        self.gate = ops.gate.to(dev).contiguous() if ops.gate is not None else None
        Ho, Wo = out_hw(c.H, c.W, geom_of(c))
        self.oshape = (c.N,) + (pool_out_hw(Ho, Wo) if c.entry in ("pool", "nchw_pool") else (Ho, Wo)) + (c.Cout,)
        self.odt = torch.float32 if c.out_f32 else TDT[dtype]

    def run(self):
        """(y [N][Ho][Wo][Cout], the channels of a wider y outside the slice or None, the guard tail)"""
        lb, L, ctx = _lib()
        c, d = self.c, self.d
        M = self.oshape[0] * self.oshape[1] * self.oshape[2]
        off, pitch = (c.yslice[0], c.Cout + c.yslice[1]) if c.yslice else (0, c.Cout)
        ybuf = torch.full((M * pitch + 256 * pitch + 64,), float("nan"), dtype=self.odt, device=self.dev)
        y = ctypes.c_void_p(ybuf.data_ptr() + off * ybuf.element_size())
        a = (ctx, ctypes.byref(d), _p(self.x), _p(self.packed), _p(self.scale), _p(self.shift))
        if c.entry == "conv" and c.gate:
            rc = L.pcv_conv2d_gated_fused(*a, _p(self.gate), _p(self.res), y, _stream())
        elif c.entry == "conv":
            rc = L.pcv_conv2d_fused(*a, _p(self.res), y, _stream())
        elif c.entry == "gemm":
            rc = L.pcv_gemm_bias(ctx, _p(self.x), _p(self.packed), _p(self.shift), y, c.N, c.Cin, c.Cout, d.dtype, d.out_dtype, _stream())
        elif c.entry == "pool":
            rc = L.pcv_conv2d_maxpool_fused(*a, y, 3, 2, 1, 0, _stream())
        else:
            rc = L.pcv_conv2d_nchw_stem_fused(*a, y, int(c.entry == "nchw_pool"), _stream())
        lb.check(rc, ctx)
        torch.cuda.synchronize()
        body = ybuf[:M * pitch].view(M, pitch)
        out = body[:, off:off + c.Cout].reshape(self.oshape)
        outside = torch.cat((body[:, :off], body[:, off + c.Cout:]), dim=1) if c.yslice else None
        return out, outside, ybuf[M * pitch:]


_STATS = os.environ.get("PCV_CONV_SWEEP_STATS")       # a file name: one JSON line per comparison (measurements, nothing is asserted from them)


def check(out, ref, bound, what, family=None, dtype=None):
    """|y - ref| <= bound elementwise; names the worst element's (n, ho, wo, c) and whether it lies on a border"""
    err = (out.double().cpu() - ref).abs()
    ratio = err / bound
    if _STATS:
        with open(_STATS, "a") as f:
            f.write(json.dumps(dict(family=family, dtype=dtype, case=what, ratio=float(ratio.nan_to_num(nan=1e30).max()))) + "\n")
    bad = ~(err <= bound)                         # NaN (an element nobody wrote) counts as a failure
    if bool(bad.any()):
        worst = int(torch.where(bad, ratio.nan_to_num(nan=float("inf")), torch.zeros_like(ratio)).argmax())
        n, ho, wo, ch = [int(v) for v in np.unravel_index(worst, tuple(ref.shape))]
        border = ho in (0, ref.shape[1] - 1) or wo in (0, ref.shape[2] - 1)
        pytest.fail("{}: {} of {} elements out of bound; worst at (n {}, ho {}, wo {}, c {}) - {} - got {:.6e}, ref {:.6e}, bound "
                    "{:.3e}".format(what, int(bad.sum()), bad.numel(), n, ho, wo, ch, "on a border" if border else "interior",
                                    float(out.flatten()[worst]), float(ref.flatten()[worst]), float(bound.flatten()[worst])))


def sweep(family, c, dtype, dev, tune):
    ops, ref, bound = _cached_reference(base_of(c), dtype)
    run = Launch(c, dtype, ops, dev)
    assert tuple(ref.shape) == run.oshape
    switches = dict(tune)
    switches.update(dict(c.tune))
    for g in GRIDS:
        what = "{} {} {} grid {}".format(family, case_id(c), dtype, g)
        with util.tuning(max_blocks=g, **switches):
            out, outside, tail = run.run()
        assert bool(torch.isnan(tail).all()), what + ": the guard tail behind y was written"
        if outside is not None:
            assert bool(torch.isnan(outside).all()), what + ": channels outside the slice of y were written"
        check(out, ref, bound, what, family, dtype)


def _params(cases, dtypes):
    return [pytest.param(c, dt, id=case_id(c) + "-" + dt) for c in cases for dt in dtypes]


# ---- F1 ---------------------------------------------------------------------------------------------------------------------------------------
def f1_runs_the_generic_kernel(c, dtype):
    """the conditions under which conv2d_impl takes the generic kernel in the tap mode the case names (with GENERIC set: no d3 / d1 /
    gconv-rows / head kernel; the flat gconv kernel and the stem kernel are kept away by the shapes themselves)"""
    P = plan(c, dtype)
    want = c.khw32 if dtype == "fp32" else c.khw
    return P.ok and not P.pair and not P.stem and not P.gconv and P.ngb == 1 and P.special == c.special and P.khw == want


@pytest.mark.parametrize("c,dtype", _params(F1, DTYPES))
def test_f1_table_mode_and_forced_tiles_vs_float64(c, dtype, cuda_device):
    assert f1_runs_the_generic_kernel(c, dtype), plan(c, dtype)
    P = plan(c, dtype)
    forced = dict(c.tune).get("tile")
    if forced is not None:
        assert P.tile == forced and P.nPixTiles >= 5, P            # the forced tile is legal here, and the case has a tile tail
        assert c.N * P.Ho * P.Wo % TILES[P.tile][1] != 0
        if forced == 0:
            assert P.nChTiles >= 2 and c.Cout % TILES[0][0] != 0, P     # many channel tiles, the last one ragged
    if "wstat" in dict(c.tune):
        assert P.nk == 1 and P.nChTiles == 1 and P.khw == 1, P
    sweep("F1", c, dtype, cuda_device, GENERIC)


# ---- F2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dtype", _params(F2, DTYPES))
def test_f2_grouped_generic_vs_float64(c, dtype, cuda_device):
    P = plan(c, dtype)
    assert P.ok and P.ngb > 1 and not P.gconv and not P.pair and not P.special, P       # P.gconv rejects these shapes by itself
    assert P.gpb == F2_GPB[(c.groups, c.Cin, c.Cout)] and P.khw == c.khw, P
    sweep("F2", c, dtype, cuda_device, GENERIC)


@pytest.mark.parametrize("dtype", DTYPES16)
def test_f2_f3_unsupported_group_shapes_are_refused(dtype, cuda_device):
    """groups 3 with 12 -> 12 channels (12 output channels per block: no multiple of 8) and a ragged Cout with groups: PCV_ERR_INVALID
    from pcv_conv_packed_bytes and from pcv_conv2d_fused, nothing launched (y keeps its NaNs)"""
    lb, L, ctx = _lib()
    for c in (C(2, 12, 12, 6, 6, groups=3), C(2, 32, 20, 6, 6, groups=2), C(2, 32, 20, 6, 6, k=1, groups=2)):
        assert not plan(c, dtype).ok
        d = make_desc(c, dtype)
        n = ctypes.c_size_t(0)
        assert L.pcv_conv_packed_bytes(ctypes.byref(d), ctypes.byref(n)) == PCV_ERR_INVALID
        x = torch.zeros((c.N, c.H, c.W, c.Cin), dtype=TDT[dtype], device=cuda_device)
        packed = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda_device)
        y = torch.full((c.N * c.H * c.W * c.Cout + 4096,), float("nan"), dtype=TDT[dtype], device=cuda_device)
        assert L.pcv_conv2d_fused(ctx, ctypes.byref(d), _p(x), _p(packed), None, None, None, _p(y), _stream()) == PCV_ERR_INVALID
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all())


def test_filter_larger_than_the_padded_input_is_refused(cuda_device):
    """3x3 / stride 2 / no padding on a 2 x 2 map has no output (the extent is -1; a division rounding towards zero once made one output
    row of it): PCV_ERR_INVALID, nothing launched"""
    lb, L, ctx = _lib()
    for c in (C(1, 16, 16, 2, 2, s=2, p=0), C(1, 16, 16, 6, 2, s=(1, 2), p=0), C(1, 3, 32, 2, 8, s=2, p=0, cpitch=4)):
        assert 0 in out_hw(c.H, c.W, geom_of(c))
        d = make_desc(c, "bf16")
        x = torch.zeros((c.N, c.H, c.W, c.cpitch or c.Cin), dtype=torch.bfloat16, device=cuda_device)
        packed = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda_device)
        y = torch.full((4096,), float("nan"), dtype=torch.bfloat16, device=cuda_device)
        assert L.pcv_conv2d_fused(ctx, ctypes.byref(d), _p(x), _p(packed), None, None, None, _p(y), _stream()) == PCV_ERR_INVALID
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all())


# ---- F3 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dtype", _params(F3_RAGGED, DTYPES) + _params(F3_F32OUT + F3_GEMM, DTYPES16))
def test_f3_special_instantiations_vs_float64(c, dtype, cuda_device):
    P = plan(c, dtype)
    # ragged Cout or fp32 output from 16-bit input: route_igemm's `special`, i.e. the RAGGED 128 x 128 instance in table mode
    assert P.ok and P.special and P.tile == 2 and P.khw == 0 and P.ngb == 1 and not P.pair, P
    assert (c.Cout % 8 != 0) or (c.out_f32 and dtype != "fp32")
    sweep("F3f" if c.out_f32 else "F3", c, dtype, cuda_device, GENERIC)


# ---- F4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dtype", _params(F4, DTYPES16))
def test_f4_pixel_pairs_on_the_generic_kernel_vs_float64(c, dtype, cuda_device):
    P = plan(c, dtype)
    assert P.ok and P.pair and P.khw == 0, P
    # P.stem restated: stride 2 x 2, dil_h 1, Cout <= 64 and a multiple of 8, kh <= 7, kw + (pad_l & 1) <= 8, y in the storage type
    assert not ((c.sh, c.sw) == (2, 2) and c.dh == 1 and c.Cout <= 64 and c.Cout % 8 == 0 and c.kh <= 7 and c.kw + (c.pl & 1) <= 8 and
                not c.out_f32) and not P.stem
    assert (c.wpitch or c.W) % 2 == 0 and c.sw % 2 == 0 and c.dw == 1
    sweep("F4", c, dtype, cuda_device, GENERIC)


# ---- F5 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dtype", _params(F5, DTYPES16))
def test_f5_stem_kernel_vs_float64(c, dtype, cuda_device):
    lb, L, ctx = _lib()
    P = plan(c, dtype)
    assert P.ok and P.pair and P.stem, P
    assert (c.sh, c.sw) == (2, 2) and c.dh == 1 and c.Cout <= 64 and c.Cout % 8 == 0 and c.kh <= 7 and c.kw + (c.pl & 1) <= 8
    d = make_desc(c, dtype)
    if c.entry in ("pool", "nchw_pool"):
        assert L.pcv_conv2d_maxpool_supported(ctypes.byref(d), 3, 2, 1, 0) == 1
    if c.entry in ("nchw", "nchw_pool"):
        assert c.Cin <= 3 and c.W % 4 == 0 and L.pcv_conv2d_nchw_stem_supported(ctypes.byref(d), int(c.entry == "nchw_pool")) == 1
    sweep("F5", c, dtype, cuda_device, {})


# ---- F6 / F7: the grouped 3x3 kernels (no switch is set: the library's own routing) -----------------------------------------------------------
@pytest.mark.parametrize("c,dtype", _params(FAMILIES["F6"][0], DTYPES16))
def test_f6_grouped_flat_kernel_vs_float64(c, dtype, cuda_device):
    P = plan(c, dtype)
    assert P.ok and P.gconv and c.Cin == c.Cout and c.Cin % 64 == 0 and c.Cin // c.groups in (4, 8, 16), P
    assert P.gkernel == ("generic" if c.W > 63 else "flat"), P
    sweep("F6", c, dtype, cuda_device, {})


@pytest.mark.parametrize("c,dtype", _params(FAMILIES["F7"][0], DTYPES16))
def test_f7_grouped_row_kernel_vs_float64(c, dtype, cuda_device):
    P = plan(c, dtype)
    assert P.ok and P.gconv and c.Cin == c.Cout and c.Cin % 64 == 0 and (c.sh == 2 or c.Cin // c.groups == 32), P
    if (c.H | c.W) & 1 and c.sh == 2:
        assert P.gkernel == "generic", P
    else:
        assert P.gkernel == "rows" and P.R == F7_R[P.Wo], P
    sweep("F7", c, dtype, cuda_device, {})
