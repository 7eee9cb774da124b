"""
CPU checks of the convolution sweep in tests/test_gpu_conv_sweep.py: the float64 reference of tests/conv_ref.py equals torch's
float64 convolution; an emulated kernel (fp32 F.conv2d on the rounded operands, fp32 epilogue, one rounding to the storage type) stays
inside the derived bound for EVERY case the GPU sweep launches; and the bound is tight enough to fail - on every case, each kernel bug
model its geometry can tell from the correct kernel leaves the bound somewhere, in every storage type. The bug models are applied to
the emulated kernel:
  drop_col      one (tap, channel) weight column is not multiplied
  drop_tap      one whole filter tap is skipped
  row_wrap      a tap outside [0, W) reads the neighbouring row's pixel (the address it would have in memory) instead of zero
  dil_swap      dil_h used for dil_w
  pad_swap      pad_t and pad_l swapped
  stride_swap   stride_h and stride_w swapped
  group_shift   group block g reads block g + 1's input channels
  cpitch_leak   channels [Cin, x_cpitch) of a wider buffer are not excluded
  chtile_prev   the last 64-channel tile's rows come from the tile before it
  pool_shift    the pooled stem's window starts one convolution row late
  stem_origin   the stem's patch origin is one pixel off when pad_l is odd
The lists of the GPU file are also checked for what the issue of this sweep asked of them (every stem value with every entry point).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from conv_ref import Geom, conv_ref, out_hw, pool_values, round_to
from test_gpu_conv_sweep import (DTYPES, DTYPES16, F1, F2, F4, F5, F6, F6_GENERIC, F7, F7_GENERIC, F7_R, FAMILIES, _STEM, base_of, case_id, case_reference, geom_of, plan,
                                 x_buffer)
from test_gpu_dw_se import act64


# ---- 1. the reference against torch --------------------------------------------------------------------------------------------------
_REF_GEOMS = [
    # (N, H, W, Cout, Geom(kh kw sh sw pt pl pb pr dh dw groups Cin))
    (2, 13, 11, 40, Geom(5, 5, 1, 1, 2, 2, 2, 2, 1, 1, 1, 24)), (2, 9, 17, 48, Geom(1, 7, 1, 1, 0, 3, 0, 3, 1, 1, 1, 32)),
    (3, 10, 14, 24, Geom(4, 4, 2, 2, 1, 1, 1, 1, 1, 1, 1, 16)), (2, 9, 7, 32, Geom(3, 3, 1, 1, 1, 3, 1, 3, 1, 3, 1, 32)),
    (2, 15, 15, 32, Geom(3, 3, 2, 2, 0, 1, 0, 1, 1, 1, 1, 16)), (2, 11, 13, 32, Geom(3, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 32)),
    (1, 5, 6, 16, Geom(3, 3, 1, 1, 3, 3, 3, 3, 1, 1, 1, 8)), (2, 6, 7, 64, Geom(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 32)),
    (3, 9, 7, 64, Geom(3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 4, 32)), (3, 14, 14, 96, Geom(3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 3, 48)),
    (3, 9, 7, 64, Geom(5, 5, 1, 1, 2, 2, 2, 2, 1, 1, 8, 64)), (2, 10, 14, 32, Geom(3, 3, 2, 2, 2, 1, 2, 1, 2, 1, 1, 3)),
    (1, 33, 35, 40, Geom(9, 3, 2, 2, 4, 1, 4, 1, 1, 1, 1, 4)), (1, 20, 70, 64, Geom(5, 5, 2, 2, 4, 5, 1, 2, 1, 1, 1, 4)),
    (2, 12, 12, 32, Geom(3, 3, 1, 1, 4, 4, 4, 4, 4, 4, 2, 32)),
]


@pytest.mark.parametrize("N,H,W,Cout,g", _REF_GEOMS, ids=["{}x{}_k{}x{}_g{}".format(r[1], r[2], r[4].kh, r[4].kw, r[4].groups) for r in _REF_GEOMS])
def test_reference_equals_torch_float64_convolution(N, H, W, Cout, g):
    gen = torch.Generator().manual_seed(H * W + Cout)
    x = torch.randn((N, H, W, g.Cin + 3), generator=gen, dtype=torch.float64)           # three channels behind the slice: ignored
    w = torch.randn((Cout, g.Cin // g.groups, g.kh, g.kw), generator=gen, dtype=torch.float64)
    sc = torch.rand(Cout, generator=gen, dtype=torch.float64) + 0.5
    sh = torch.randn(Cout, generator=gen, dtype=torch.float64)
    ref, S = conv_ref(x, w, sc, sh, g, 0)
    xn = F.pad(x[..., :g.Cin].permute(0, 3, 1, 2), (g.pl, g.pr, g.pt, g.pb))
    want = F.conv2d(xn, w, stride=(g.sh, g.sw), dilation=(g.dh, g.dw), groups=g.groups) * sc[:, None, None] + sh[:, None, None]
    want = want.permute(0, 2, 3, 1)
    assert ref.shape == want.shape == (N,) + out_hw(H, W, g) + (Cout,)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    wantS = F.conv2d(xn.abs(), w.abs(), stride=(g.sh, g.sw), dilation=(g.dh, g.dw), groups=g.groups).permute(0, 2, 3, 1)
    assert float((S - wantS).abs().max()) <= 1e-12 * float(wantS.abs().max())


# ---- 2. the emulated kernel and its bug models ------------------------------------------------------------------------------------------
def _conv32(x, w, c, Ho, Wo, sh=None, sw=None, pt=None, pl=None, dh=None, dw=None):
    """fp32 convolution of NHWC x with the case's geometry (any of it overridden), the first Ho x Wo outputs: bottom / right zero
    padding as far as those need, which for the true geometry is the true convolution"""
    sh, sw = c.sh if sh is None else sh, c.sw if sw is None else sw
    pt, pl = c.pt if pt is None else pt, c.pl if pl is None else pl
    dh, dw = c.dh if dh is None else dh, c.dw if dw is None else dw
    H, W = x.shape[1], x.shape[2]
    pb = max(0, (Ho - 1) * sh + dh * (c.kh - 1) + 1 - (H + pt))
    pr = max(0, (Wo - 1) * sw + dw * (c.kw - 1) + 1 - (W + pl))
    xn = F.pad(x.permute(0, 3, 1, 2).float(), (pl, pr, pt, pb))
    y = F.conv2d(xn, w.float(), stride=(sh, sw), dilation=(dh, dw), groups=c.groups)
    return y[:, :, :Ho, :Wo].permute(0, 2, 3, 1)


def _wrapped(xfull, c, Wo):
    """NHWC input whose left / right padding columns hold what lies at those addresses: the end of the row above, the start of the row
    below (through the pad column of a wider row pitch), zero only outside the image"""
    N, H, wp, Cc = xfull.shape
    pr = max(0, (Wo - 1) * c.sw + c.dw * (c.kw - 1) + 1 - (c.W + c.pl))
    cols = torch.arange(-c.pl, c.W + pr)
    idx = torch.arange(H)[:, None] * wp + cols[None, :]
    ok = (idx >= 0) & (idx < H * wp)
    flat = xfull.reshape(N, H * wp, Cc)
    out = flat[:, idx.clamp(0, H * wp - 1).reshape(-1)].reshape(N, H, cols.numel(), Cc)
    return out * ok[None, :, :, None]


def relevant_mutants(c, dtype):
    """the bug models the geometry of a case can tell from the correct kernel"""
    P = plan(c, dtype)
    m = ["drop_col", "drop_tap"]
    # columns a tap reaches beyond either edge; the first one is the pad column of the padded 4-channel input where it has one (zero
    # by contract, so reading it is no error)
    zero_col = int(c.cpitch == 4 and (c.wpitch or c.W) > c.W)
    right = (P.Wo - 1) * c.sw - c.pl + c.dw * (c.kw - 1) - (c.W - 1)
    if (c.pl > zero_col or right > zero_col) and c.H > 1 and not P.stem:
        m.append("row_wrap")
    if c.dh != c.dw and c.kw > 1:
        m.append("dil_swap")
    if c.pt != c.pl:
        m.append("pad_swap")
    if c.sh != c.sw:
        m.append("stride_swap")
    if c.groups > 1:
        m.append("group_shift")
    if (c.cpitch or c.Cin) > c.Cin and not P.pair:
        m.append("cpitch_leak")
    if c.Cout > 64:
        m.append("chtile_prev")
    if c.entry in ("pool", "nchw_pool") and P.Ho > 1:
        m.append("pool_shift")
    if P.stem and c.pl & 1:
        m.append("stem_origin")
    return m


def emulate(c, ops, dtype, mutant=None):
    """the output of an fp32 kernel on the case's operands, rounded to the output type; NHWC float64"""
    P = plan(c, dtype)
    Ho, Wo = P.Ho, P.Wo
    x, w = ops.x, ops.w
    kw = {}
    # the tap that reads input pixel (0, 0) for output (0, 0) (the last one where the padding is wider than the filter): it meets data
    # on every map, also on a one-row map under a tall filter
    r, q = min(c.kh - 1, -(-c.pt // c.dh)), min(c.kw - 1, -(-c.pl // c.dw))
    if mutant == "drop_col":
        w = w.clone()
        w[:, w.shape[1] // 2, r, q] = 0
    elif mutant == "drop_tap":
        w = w.clone()
        w[:, :, r, q] = 0
    elif mutant == "row_wrap":
        x = _wrapped(x_buffer(c, ops, dtype)[..., :c.Cin], c, Wo)
        kw = dict(pl=0)
    elif mutant == "dil_swap":
        kw = dict(dw=c.dh)
    elif mutant == "pad_swap":
        kw = dict(pt=c.pl, pl=c.pt)
    elif mutant == "stride_swap":
        kw = dict(sh=c.sw, sw=c.sh)
    elif mutant == "group_shift":
        x = x.roll(-(c.Cin // c.groups), dims=3)
    elif mutant == "cpitch_leak":
        x = x_buffer(c, ops, dtype)[:, :, :c.W]
        extra = torch.arange(x.shape[3] - c.Cin) % c.Cin
        w = torch.cat((w, w[:, extra]), dim=1)
    elif mutant == "stem_origin":
        kw = dict(pl=c.pl + 1)
    v = _conv32(x, w, c, Ho, Wo, **kw)
    if ops.scale is not None:
        v = v * ops.scale
    v = act64(v + ops.shift, c.act)
    if ops.gate is not None:
        v = v * ops.gate[:, None, None, :]
    if ops.res is not None:
        v = v + ops.res
    v = act64(v, c.post)
    assert v.dtype == torch.float32
    if mutant == "chtile_prev":
        last0 = (c.Cout - 1) // 64 * 64
        v = v.clone()
        v[..., last0:] = v[..., last0 - 64:c.Cout - 64]
    y = round_to(v, "fp32" if c.out_f32 else dtype).double()
    if c.entry in ("pool", "nchw_pool"):
        if mutant == "pool_shift":
            y = torch.cat((y[:, 1:], torch.full_like(y[:, :1], float("-inf"))), dim=1)
        y = pool_values(y)
    return y


def _distinct():
    """(family, case, dtype) of the sweep, the tuning-switch variants of one geometry once"""
    seen, out = set(), []
    for fam, (cases, dts) in FAMILIES.items():
        for c in cases:
            if base_of(c) not in seen:
                seen.add(base_of(c))
                out += [(fam, c, dt) for dt in dts]
    return out


@functools.lru_cache(maxsize=8)
def _reference(base, dtype):
    return case_reference(base, dtype)


_RATIOS = {}


@pytest.mark.parametrize("fam,c,dtype", [pytest.param(f, c, dt, id="{}-{}-{}".format(f, case_id(c), dt)) for f, c, dt in _distinct()])
def test_emulated_kernel_inside_and_bug_models_outside_the_bound(fam, c, dtype):
    ops, ref, bound = _reference(base_of(c), dtype)
    y = emulate(c, ops, dtype)
    assert y.shape == ref.shape
    ratio = float(((y - ref).abs() / bound).max())
    _RATIOS[(fam, dtype)] = max(_RATIOS.get((fam, dtype), 0.0), ratio)
    assert ratio <= 1.0, "the correct kernel leaves the bound (error / bound = {:.3f}): the derivation is wrong".format(ratio)
    for m in relevant_mutants(c, dtype):
        bug = emulate(c, ops, dtype, m)
        assert bool(((bug - ref).abs() > bound).any()), "{} is not told from the correct kernel".format(m)


def test_every_bug_model_is_relevant_somewhere_in_every_dtype():
    names = {"drop_col", "drop_tap", "row_wrap", "dil_swap", "pad_swap", "stride_swap", "group_shift", "cpitch_leak", "chtile_prev",
             "pool_shift", "stem_origin"}
    for dt in DTYPES:
        seen = set()
        for fam, c, d in _distinct():
            if d == dt:
                seen |= set(relevant_mutants(c, dt))
        assert seen == (names if dt != "fp32" else names - {"pool_shift", "stem_origin"}), (dt, names - seen)


# ---- 3. the lists ----------------------------------------------------------------------------------------------------------------------------
def test_families_run_where_they_claim():
    for c in F1:
        for dt in DTYPES:
            P = plan(c, dt)
            assert P.ok and not P.pair and not P.stem and not P.gconv and P.ngb == 1, case_id(c)
            assert P.khw == (c.khw32 if dt == "fp32" else c.khw) and P.special == c.special, (case_id(c), dt, P)
    assert {plan(c, "bf16").khw for c in F1} == {0, 1, 9}
    for c in F2:
        for dt in DTYPES:
            assert plan(c, dt).ngb > 1 and not plan(c, dt).gconv, case_id(c)
    for c in F4:
        for dt in DTYPES16:
            assert plan(c, dt).pair and not plan(c, dt).stem, case_id(c)
    for c in F5:
        for dt in DTYPES16:
            assert plan(c, dt).stem, case_id(c)
    for c in F6 + F6_GENERIC + F7 + F7_GENERIC:
        assert c.Cin == c.Cout and c.Cin % 64 == 0 and not c.res and c.post == 0 and not c.gate and not c.yslice and not c.tune, case_id(c)
        for dt in DTYPES16:
            assert plan(c, dt).gconv and plan(c, dt).ngb > 1, case_id(c)
        assert not plan(c, "fp32").gconv and plan(c, "fp32").gkernel == "generic"                      # 16 bit only
    assert all(plan(c, dt).gkernel == "flat" for c in F6 for dt in DTYPES16) and all(plan(c, "bf16").gkernel == "generic" for c in F6_GENERIC)
    assert {(c.Cin // c.groups, (0 if c.W + 1 <= 16 else (1 if c.W + 1 <= 32 else 2))) for c in F6} == {(g, slot) for g in (4, 8, 16) for slot in (0, 1, 2)}   # gconv_slot
    assert {c.W for c in F6} == {5, 15, 16, 31, 32, 63} and {c.H for c in F6} == {1, 3, 9} and {c.W for c in F6_GENERIC} == {64}
    tiles = {(c.N * c.H * c.W + 127) // 128 * (c.Cin // 64) for c in F6}
    assert 1 in tiles and 9 in tiles and max(tiles) > 16 and any(c.Cin == 128 for c in F6)
    assert all((c.H * c.W) % 128 != 0 for c in F6 if c.N > 1)                                          # images end inside a 128-pixel tile
    assert {c.act for c in F6 if (c.N, c.H, c.W, c.groups) == (3, 3, 15, 8)} == set(range(7))
    assert all(plan(c, dt).gkernel == "rows" for c in F7 for dt in DTYPES16) and all(plan(c, "bf16").gkernel == "generic" for c in F7_GENERIC)
    assert {(c.sh, c.Cin // c.groups) for c in F7} == {(2, 4), (2, 8), (2, 16), (2, 32), (1, 32)}
    for s in (1, 2):
        assert {plan(c, "bf16").R for c in F7 if c.sh == s} == {64, 32, 9, 4, 3, 1}, s
    for c in F7:
        P = plan(c, "bf16")
        assert P.R == F7_R[P.Wo] and (P.R == 1 or c.N * P.Ho % P.R != 0), case_id(c)
        assert not (c.sh == 2 and (c.H | c.W) & 1)
    assert all(c.sh == 2 and (c.H | c.W) & 1 for c in F7_GENERIC)
    assert {c.act for c in F7 if (c.N, c.H, c.W, c.groups) == (2, 10, 14, 4)} == set(range(7)) and any(c.Cin == 128 for c in F7)
    big = [c for c in F1 if (c.N, c.Cin, c.Cout) == (9, 8, 200) and not c.tune][0]
    assert all(9 * 13 * 11 % bp for bp in (64, 128, 256)) and plan(big, "bf16").nPixTiles * plan(big, "bf16").nChTiles > 2 * 8


def test_stem_list_covers_every_value_with_every_entry_point():
    assert 40 <= len(_STEM) <= 60
    kernels = {(3, 3), (7, 7), (5, 5), (1, 1), (2, 2), (4, 4), (6, 6), (3, 7), (7, 3), (7, 1)}
    maps = {(2, 2), (1, 40), (5, 7), (31, 33), (32, 32), (33, 35), (20, 70)}
    for entry in ("conv", "pool", "nchw", "nchw_pool"):
        rows = [r for r in _STEM if r[0] == entry]
        nchw = entry.startswith("nchw")
        assert {r[1] for r in rows} == kernels, entry
        assert {r[2][1] for r in rows} == {0, 1, 2, 3, 5} and {r[2][0] for r in rows} == {0, 1, 3, 4}, entry
        assert any(r[2] == (0, 1, 0, 1) for r in rows) and any(r[2][0] != r[2][2] or r[2][1] != r[2][3] for r in rows), entry
        assert {r[3] for r in rows} == ({1, 2, 3} if nchw else {1, 2, 3, 4}), entry         # the NCHW forms take at most 3 planes
        assert {r[4] for r in rows} >= {8, 24, 32, 40, 64}, entry
        assert {r[6] for r in rows} == {1, 3}, entry
        if nchw:                                                                            # ... and W % 4 == 0
            assert all(r[5][1] % 4 == 0 for r in rows) and {r[5] for r in rows} >= {(1, 40), (32, 32), (5, 8), (33, 36)}, entry
        else:
            assert {r[5] for r in rows} == maps, entry
        assert all(r[1][1] + (r[2][1] & 1) <= 8 for r in rows)
    plain = [r for r in _STEM if r[0] == "conv"]
    assert {r[7] for r in plain if (r[1], r[4], r[5]) == ((3, 3), 24, (5, 7))} == set(range(7))      # all seven activations on one shape
    for entry in ("conv", "nchw"):
        assert {r[8] for r in _STEM if r[0] == entry and r[4] <= 32} == {0, 1}, entry


def test_tuning_defaults_the_sweep_restores_match_the_library():
    """util.tuning puts `tile`, `persist` and `wstat` back to util._TUNING_DEFAULTS after a forced-tile case: those must be pcv_ctx's own
    initial values, or every test after the sweep would run another launch form"""
    import os
    import re
    import util
    with open(os.path.join(os.path.dirname(util.HERE), "pytorchcv_amd", "csrc", "pcv_api.hip")) as f:
        src = f.read()
    for key, field in (("persist", "persist_mode"), ("tile", "force_tile"), ("wstat", "use_wstat"), ("stem32", "use_stem32"),
                       ("d3x3", "use_d3x3"), ("d1x1", "use_d1x1"), ("d1i", "use_d1i"), ("gconvr", "use_gconvr"), ("head", "use_head")):
        m = re.search(r"^\s*int {} = (-?\d+);".format(field), src, re.M)
        assert m and int(m.group(1)) == util._TUNING_DEFAULTS[key], (key, field)
        assert re.search(r'\{{"{}", &pcv_ctx::{}\}}'.format(key, field), src), (key, field)
    from test_gpu_conv_sweep import K_GCONVR_MAX_LDS
    m = re.search(r"kGconvRMaxLds = (\d+) \* 1024;", src)
    assert m and int(m.group(1)) * 1024 == K_GCONVR_MAX_LDS
