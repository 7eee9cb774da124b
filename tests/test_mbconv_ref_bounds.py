"""
CPU checks of the fused inverted-residual sweep in tests/test_gpu_mbconv_sweep.py:
  1. the float64 reference of tests/mbconv_ref.py, without its rounding points, equals a float64 F.conv2d composition;
  2. an emulated fp32 kernel - in the plain form and in mbr.hpp's fp16 + ReLU6 form, which keeps E / 6 and D / 6 - is bit-identical to
     the reference on every exact case and inside the derived bound on every bounded case (the largest error / bound ratio per dtype is
     collected in _RATIOS);
  3. every exact case passes the certificate (every fp32 partial sum exact in any order), none is dropped;
  4. kernel bug models, applied to the emulated kernel. Exact family - each must change the result in EVERY case whose geometry makes
     it relevant, in both dtypes:
       drop_tap        one depthwise tap of one channel is not multiplied          shift_row / shift_col   the window starts one row / column late
       pad_e           E at padded positions is act(shift_e), not 0                chunk_taps / chunk_bn   the ragged last 32-channel chunk takes the
       edge_neighbour  a tile's last column holds the neighbouring tile's first                            previous chunk's taps / BN constants
       edge_halo       a tile's last column is computed with a zero right neighbour (the halo lane of a 16-lane row is stored)
       row_repeat      the last row tile repeats the one before it                 swap_parity             stride 2: odd and even columns swapped
       res_neighbour   the residual of the neighbouring pixel                      noclamp_e / noclamp_d   ReLU6 without its upper clamp
     Bounded family - each must leave the bound somewhere in both dtypes:
       scale_swap (scale_e and scale_d swapped), skip_act_d, unfold_hd (shift_d / 6 used as shift_d), unfold_sp (scale_p without its 6),
       relu_for_relu6, hswish_as_swish
  5. the routing of pcv_mbconv_fused restated in the GPU file: its constants and the kMbr table against the source, the three LDS layout
     functions against a host program compiled from the headers (tests/tools/mb_lds_check.cpp);
  6. coverage: the case lists reach every row of kMbr and kMbw and every block-kernel variant the entry point can reach;
  7. a broken reference (one tap dropped in mbconv_ref) fails the exact comparison of the emulated kernel.
"""

import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
from conv_ref import round_to
from mbconv_ref import Ops, Unit, certified, exact_operands, out_hw, residual_of, taps_of, unit_ref
from test_gpu_dw_se import HSWISH, NONE, RELU, RELU6, SWISH, TDT, act64
import test_gpu_mbconv_sweep as S
from test_gpu_mbconv_sweep import BOUNDED, DTYPES16, EXACT, case_id, route, seed_of, unsupported

CSRC = os.path.join(os.path.dirname(util.HERE), "pytorchcv_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


# ---- 1. the reference against torch ---------------------------------------------------------------------------------------------------
_REF_UNITS = [Unit(2, 9, 11, 8, 24, 16, 1, True, RELU6, RELU, NONE, NONE, "own"), Unit(1, 10, 7, 16, 40, 8, 2, True, HSWISH, SWISH, RELU6, RELU, "own"),
              Unit(2, 7, 12, 24, 24, 24, 1, False, NONE, RELU6, NONE, HSWISH, "x"), Unit(3, 5, 5, 8, 8, 8, 2, True, NONE, NONE, NONE, NONE, None)]


@pytest.mark.parametrize("u", _REF_UNITS, ids=lambda u: "{}x{}_{}-{}-{}_s{}".format(u.H, u.W, u.Cin, u.Cmid, u.Cout, u.stride))
def test_unrounded_reference_equals_torch_float64_composition(u):
    gen = torch.Generator().manual_seed(u.H * u.W + u.Cmid)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)          # noqa: E731
    Ho, Wo = out_hw(u)
    ops = Ops(rnd(u.N, u.H, u.W, u.Cin), rnd(u.Cmid, u.Cin, 1, 1) if u.expand else None, rnd(u.Cmid) if u.expand else None,
              rnd(u.Cmid) if u.expand else None, rnd(u.Cmid, 1, 3, 3), rnd(u.Cmid), rnd(u.Cmid), rnd(u.Cout, u.Cmid, 1, 1),
              rnd(u.Cout), rnd(u.Cout), rnd(u.N, Ho, Wo, u.Cout) if u.res == "own" else None)
    y = unit_ref(u, ops, "bf16", rounded=False)[0]
    bn = lambda t, sc, sh: t * sc[:, None, None] + sh[:, None, None]             # noqa: E731
    t = ops.x.permute(0, 3, 1, 2)
    if u.expand:
        t = act64(bn(F.conv2d(t, ops.w_exp), ops.scale_e, ops.shift_e), u.act_e)
    t = act64(bn(F.conv2d(t, ops.w_dw, stride=u.stride, padding=1, groups=u.Cmid), ops.scale_d, ops.shift_d), u.act_d)
    t = act64(bn(F.conv2d(t, ops.w_proj), ops.scale_p, ops.shift_p), u.act_p)
    res = residual_of(u, ops)
    if res is not None:
        t = t + res.permute(0, 3, 1, 2)
    want = act64(t, u.post).permute(0, 2, 3, 1)
    assert y.shape == want.shape == (u.N, Ho, Wo, u.Cout)
    assert float((y - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- 2. the emulated kernel and its bug models ---------------------------------------------------------------------------------------------
SIXTH = torch.tensor(1.0 / 6.0, dtype=torch.float32)
EXACT_BUGS = ("drop_tap", "shift_row", "shift_col", "pad_e", "chunk_taps", "chunk_bn", "edge_neighbour", "edge_halo", "row_repeat", "swap_parity",
              "res_neighbour", "noclamp_e", "noclamp_d")
BOUNDED_BUGS = ("scale_swap", "skip_act_d", "unfold_hd", "unfold_sp", "relu_for_relu6", "hswish_as_swish")


def can_fold(u, dtype):
    """mbr.hpp's FAST form: fp16, both inner stages ReLU6"""
    return dtype == "fp16" and u.expand and u.act_e == RELU6 and u.act_d == RELU6


def relevant(c, bug):
    """the geometry of the case can tell this bug model from the correct kernel"""
    u, rt = c.u, route(c.u, c.k)
    Ho, Wo = out_hw(u)
    ragged = u.Cmid > 32 and u.Cmid % 32 != 0
    acts = (u.act_e if u.expand else NONE, u.act_d, u.act_p, u.post)
    return {"drop_tap": True, "shift_row": True, "shift_col": True, "pad_e": u.expand, "chunk_taps": ragged, "chunk_bn": ragged,
            "edge_neighbour": Wo > rt.OC, "edge_halo": Wo > rt.OC and u.stride == 1, "row_repeat": Ho > rt.RO, "swap_parity": u.stride == 2,
            "res_neighbour": u.res is not None, "noclamp_e": u.expand and u.act_e == RELU6, "noclamp_d": u.act_d == RELU6,
            "scale_swap": u.expand, "skip_act_d": u.act_d != NONE, "unfold_hd": True, "unfold_sp": True,
            "relu_for_relu6": RELU6 in acts[:2], "hswish_as_swish": HSWISH in acts}[bug]


def _act32(v, code, bug):
    if bug == "hswish_as_swish" and code == HSWISH:
        code = SWISH
    if bug == "relu_for_relu6" and code == RELU6:
        code = RELU
    out = act64(v, code)
    assert out.dtype == torch.float32
    return out


def _depthwise32(E, taps, stride, Ho, Wo, pad, oy=0, ox=0, skip_dx=None):
    """fp32 3x3 / pad 1 depthwise of NHWC E; `pad`: per-channel value of the padding; (oy, ox): origin of the window"""
    N, H, W, C = E.shape
    Ep = pad.expand(N, H + 3, W + 3, C).clone()
    Ep[:, 1:H + 1, 1:W + 1] = E
    if oy or ox:
        Ep[:, H + 1:, :] = 0
        Ep[:, :, W + 1:] = 0
    z = torch.zeros((N, Ho, Wo, C), dtype=torch.float32)
    for dy in range(3):
        for dx in range(3):
            if dx == skip_dx:
                continue
            z = z + Ep[:, oy + dy:oy + dy + stride * (Ho - 1) + 1:stride, ox + dx:ox + dx + stride * (Wo - 1) + 1:stride] * taps[3 * dy + dx]
    return z


def emulate(c, ops, dtype, folded=False, bug=None):
    """what an fp32 kernel with the three rounding points stores, as a tensor of the storage type"""
    u, rt = c.u, route(c.u, c.k)
    Ho, Wo = out_hw(u)
    r16 = lambda v: round_to(v, dtype)                                            # noqa: E731
    se, he = (ops.scale_e.clone(), ops.shift_e.clone()) if u.expand else (None, None)
    sd, hd, sp, hp = ops.scale_d.clone(), ops.shift_d.clone(), ops.scale_p.clone(), ops.shift_p.clone()
    taps = taps_of(ops.w_dw).clone()
    act_e, act_d = u.act_e, u.act_d
    c0 = u.Cmid // 32 * 32
    n = u.Cmid - c0
    if bug == "chunk_taps":
        taps[:, c0:] = taps[:, c0 - 32:c0 - 32 + n]
    elif bug == "chunk_bn":
        for t in (se, he, sd, hd):
            if t is not None:
                t[c0:] = t[c0 - 32:c0 - 32 + n].clone()
    elif bug == "scale_swap":
        se, sd = sd, se
    elif bug == "skip_act_d":
        act_d = NONE
    elif bug == "unfold_hd":
        hd = hd * SIXTH
    elif bug == "unfold_sp":
        sp = sp * SIXTH
    elif bug == "noclamp_e":
        act_e = RELU
    elif bug == "noclamp_d":
        act_d = RELU
    assert not (folded and bug in ("noclamp_e", "noclamp_d", "skip_act_d", "relu_for_relu6"))
    zero = torch.zeros(u.Cmid)
    if u.expand:
        z = ops.x @ ops.w_exp[:, :, 0, 0].t()
        if folded:
            E = r16(z * (se * SIXTH) + he * SIXTH).clamp(0, 1)
            pad = r16(he * SIXTH).clamp(0, 1) if bug == "pad_e" else zero
        else:
            E = r16(_act32(z * se + he, act_e, bug))
            pad = r16(_act32(he, act_e, bug)) if bug == "pad_e" else zero
    else:
        E, pad = ops.x, zero
    if bug == "swap_parity":
        m = u.W // 2 * 2
        E = E.clone()
        E[:, :, 0:m:2], E[:, :, 1:m:2] = E[:, :, 1:m:2].clone(), E[:, :, 0:m:2].clone()
    z = _depthwise32(E, taps, u.stride, Ho, Wo, pad, oy=int(bug == "shift_row"), ox=int(bug == "shift_col"))
    if bug == "drop_tap":
        # the centre tap of one channel - the first one, from the middle channel on, in which that changes D and w_proj is not zero (a
        # channel that sits on its clamp everywhere, or that the projection ignores, shows nothing whatever the kernel does with it)
        zc = z - E[:, 0:u.stride * (Ho - 1) + 1:u.stride, 0:u.stride * (Wo - 1) + 1:u.stride] * taps[4]
        if folded:
            live = (r16(zc * sd + hd * SIXTH).clamp(0, 1) != r16(z * sd + hd * SIXTH).clamp(0, 1)).any(dim=0).any(dim=0).any(dim=0)
        else:
            live = (r16(_act32(zc * sd + hd, act_d, bug)) != r16(_act32(z * sd + hd, act_d, bug))).any(dim=0).any(dim=0).any(dim=0)
        live &= ops.w_proj[:, :, 0, 0].abs().sum(dim=0) > 0
        order = torch.arange(u.Cmid).roll(-(u.Cmid // 2))
        ch = int(order[live[order]][0])
        z[..., ch] = zc[..., ch]
    if bug == "edge_halo":
        z[:, :, rt.OC - 1:Wo - 1:rt.OC] = _depthwise32(E, taps, u.stride, Ho, Wo, pad, skip_dx=2)[:, :, rt.OC - 1:Wo - 1:rt.OC]
    if folded:
        D = r16(z * sd + hd * SIXTH).clamp(0, 1)
        sp = sp * 6
    else:
        D = r16(_act32(z * sd + hd, act_d, bug))
    v = _act32((D @ ops.w_proj[:, :, 0, 0].t()) * sp + hp, u.act_p, bug)
    res = residual_of(u, ops)
    if res is not None:
        v = v + (res.roll(1, dims=2) if bug == "res_neighbour" else res)
    y = _act32(v, u.post, bug).to(TDT[dtype])
    if bug == "edge_neighbour":
        idx = torch.arange(rt.OC - 1, Wo - 1, rt.OC)
        y[:, :, idx] = y[:, :, idx + 1]
    elif bug == "row_repeat":
        t0 = (Ho - 1) // rt.RO * rt.RO
        y[:, t0:] = y[:, t0 - rt.RO:t0 - rt.RO + Ho - t0].clone()
    return y


def _distinct(cases):
    """the cases of a list with distinct (unit, tile geometry): the switches of two cases may route one unit to the same tiles"""
    seen, out = set(), []
    for c in cases:
        rt = route(c.u, c.k)
        key = (c.u, rt.RO, rt.OC)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@functools.lru_cache(maxsize=4)
def _exact_ref(u, dtype):
    return S.exact_reference(u, dtype)


_RATIOS, _DETECTED = {}, {}


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("c", _distinct(EXACT), ids=case_id)
def test_exact_family_emulated_kernel_is_bit_identical_and_every_relevant_bug_is_not(c, dtype):
    ops, want = _exact_ref(c.u, dtype)
    ok, worst = certified(c.u, ops, dtype)
    assert ok, "certificate: sum |term| / g = 2^{:.1f} is not below 2^24".format(np.log2(worst))                         # (3.)
    assert torch.equal(emulate(c, ops, dtype), want)
    if can_fold(c.u, dtype):
        assert torch.equal(emulate(c, ops, dtype, folded=True), want), "the /6-folded form is not exact on these operands"
    for bug in EXACT_BUGS:
        if relevant(c, bug):
            assert not torch.equal(emulate(c, ops, dtype, bug=bug), want), "{} is not told from the correct kernel".format(bug)
            if can_fold(c.u, dtype) and bug not in ("noclamp_e", "noclamp_d"):
                assert not torch.equal(emulate(c, ops, dtype, folded=True, bug=bug), want), "{} (folded form) is not told".format(bug)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("c", _distinct(BOUNDED), ids=case_id)
def test_bounded_family_emulated_kernel_inside_the_bound(c, dtype):
    ops, ref, bound = S.bounded_reference(c.u, dtype)
    for folded in ([False, True] if can_fold(c.u, dtype) else [False]):
        y = emulate(c, ops, dtype, folded=folded).double()
        ratio = float(((y - ref).abs() / bound).max())
        _RATIOS[dtype] = max(_RATIOS.get(dtype, 0.0), ratio)
        assert ratio <= 1.0, "the correct kernel leaves the bound (error / bound = {:.3f}): the derivation is wrong".format(ratio)
    _walk_bounded(c, dtype, _DETECTED)


def test_every_bounded_bug_model_leaves_the_bound_in_both_dtypes():
    hits = {}
    for dt in DTYPES16:
        for c in _distinct(BOUNDED):
            _walk_bounded(c, dt, hits)
    for bug in BOUNDED_BUGS:
        for dt in DTYPES16:
            assert (bug, dt) in hits, (bug, dt, "relevant nowhere")
            assert hits[(bug, dt)][0] >= 1, (bug, dt, hits[(bug, dt)])


def _walk_bounded(c, dtype, hits):
    """per (bug model, dtype): [cases in which it leaves the bound, cases in which it is relevant]"""
    ops, ref, bound = S.bounded_reference(c.u, dtype)
    for bug in BOUNDED_BUGS:
        if relevant(c, bug):
            out = bool(((emulate(c, ops, dtype, bug=bug).double() - ref).abs() > bound).any())
            hit = hits.setdefault((bug, dtype), [0, 0])
            hit[0] += int(out)
            hit[1] += 1


def test_every_exact_bug_model_is_relevant_somewhere_in_each_dtype():
    for dt in DTYPES16:
        seen = {b for c in _distinct(EXACT) for b in EXACT_BUGS if relevant(c, b)}
        assert seen == set(EXACT_BUGS), (dt, set(EXACT_BUGS) - seen)
        folded = {b for c in _distinct(EXACT) if can_fold(c.u, dt) for b in EXACT_BUGS if relevant(c, b)}
        if dt == "fp16":
            assert folded >= set(EXACT_BUGS) - {"noclamp_e", "noclamp_d"}, set(EXACT_BUGS) - folded
    for c in EXACT:                                                 # the recipe's operands: each value exact in both storage types
        ops = exact_operands(c.u, seed_of(c.u))
        for t in ops:
            if t is not None:
                assert torch.equal(t, round_to(t, "bf16")) and torch.equal(t, round_to(t, "fp16"))
        break


# ---- 7. a broken reference fails --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES16)
def test_a_reference_with_one_tap_dropped_fails_the_exact_comparison(dtype):
    c = [c for c in EXACT if (c.u.Cin, c.u.Cmid, c.u.Cout, c.u.stride) == (24, 40, 24, 1)][0]
    ops, want = _exact_ref(c.u, dtype)
    broken = unit_ref(c.u, ops, dtype, drop_tap=(4, 17))[0].float().to(TDT[dtype])
    y = emulate(c, ops, dtype)
    assert torch.equal(y, want) and not torch.equal(y, broken)
    diff = (y.float() != broken.float())
    assert int(diff.sum()) < diff.numel()                  # one tap of one channel: not everything moves


# ---- 5. routing -----------------------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_routing_constants_and_instance_tables_match_the_source():
    api = _src("pcv_api.hip")
    m = re.search(r"kMbMaxLds = (\d+) \* 1024, kMbwMaxLds = (\d+) \* 1024;", api)
    assert m and (int(m.group(1)) * 1024, int(m.group(2)) * 1024) == (S.K_MB_MAX_LDS, S.K_MBW_MAX_LDS)
    for key, field in (("mbw", "use_mbw"), ("mbr", "use_mbr"), ("mbr_xl", "use_mbr_xl")):
        m = re.search(r"^\s*int {} = (-?\d+);".format(field), api, re.M)
        assert m and int(m.group(1)) == util._TUNING_DEFAULTS[key], key
    tf = {"true": True, "false": False}
    rows = re.findall(r"MBR_SHAPES2\(X, DT, (\d), (\d), (\d), (\d), (true|false), (\d), (true|false), (true|false)\)", _src("mbr_inst.hpp"))
    assert [(int(a), int(b), int(c), int(d), tf[e], int(f), tf[g], tf[h]) for a, b, c, d, e, f, g, h in rows] == S.MBR_ROWS
    inst = _src("mbw_inst.hpp")
    assert re.search(r"MBW_SHAPES3\(X, DT, 1, 2\) MBW_SHAPES3\(X, DT, 1, 4\) MBW_SHAPES3\(X, DT, 2, 2\) MBW_SHAPES3\(X, DT, 2, 4\)", inst)
    assert len(re.findall(r"X\(DT, S, NRT, (?:-1|PCV_ACT_RELU6?), (?:16|8)\)", inst)) == 6
    assert len(re.findall(r"X\(DT, 1, 4, (?:-1|PCV_ACT_RELU6?), (?:16|8), 2\)", inst)) == 6
    assert len(re.findall(r"X\(DT, 1, 6, (?:-1|PCV_ACT_RELU6?), 16, [23], 2\)", inst)) == 6
    assert len(S.MBR_ROWS) * 2 == 16 and len(S.MBW_ROWS) * 3 == 36


def _lds_grid():
    """the layout arguments the routing of every case evaluates, and a few beyond"""
    rows = set()
    for nChunks in sorted({(c.u.Cmid + 31) // 32 for c in EXACT + BOUNDED} | {19, 24}):
        for (nrt, ro, s, ka, afl, waves, wel, xl) in S.MBR_ROWS:
            rows.add(("mbr", nrt, nChunks, ka, int(afl), int(wel), (ro + 2 if s == 1 else 2 * ro + 1) if xl else 0, waves))
        for (s, nrt, tw, ka, rb) in S.MBW_ROWS:
            for nw in (8, 6, 4):
                rows.add(("mbw", s, nrt, nChunks, nw, tw, ka, rb))
        for s in (1, 2):
            for expand, ka in ((0, 0), (1, 1), (1, 2), (1, 3)):
                for nbuf in (1, 2):
                    rows.add(("mb", s, expand, ka, nChunks, 2, nbuf))               # the block kernel's row tiles: the constant kMbRowT
    return sorted(rows)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_lds_layout_restatement_equals_the_compiled_headers(tmp_path):
    exe, grid = str(tmp_path / "mb_lds_check"), str(tmp_path / "grid.txt")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-I", CSRC, os.path.join(util.HERE, "tools", "mb_lds_check.cpp"),
                           "-o", exe])
    rows = _lds_grid()
    with open(grid, "w") as f:
        f.write("".join(" ".join(str(v) for v in r) + "\n" for r in rows))
    got = [int(v) for v in subprocess.check_output([exe, grid]).split()]
    fn = {"mbr": S.mbr_lds_total, "mbw": S.mbw_lds_total, "mb": S.mb_lds_total}
    want = [fn[r[0]](*r[1:]) for r in rows]
    assert len(got) == len(rows) > 300 and got == want, [(r, g, w) for r, g, w in zip(rows, got, want) if g != w][:5]


def test_routing_of_known_units():
    """MobileNetV2's units land where csrc/mbr_inst.hpp says they do, and the switches move them as the GPU file relies on"""
    U = S.U
    assert route(U(32, 32, 16, 1, 2, 112, 112), "mbr").inst[1:] == S.MBR_ROWS[0]                   # one chunk: x through LDS
    assert route(U(32, 32, 16, 1, 2, 112, 112), "mbr_nx").inst[1:] == S.MBR_ROWS[1]
    assert route(U(24, 144, 24, 1, 2, 56, 56), "mbr").inst[1:] == S.MBR_ROWS[1]                    # its two x buffers per wave do not fit
    assert route(U(96, 576, 96, 1, 2, 14, 14), "mbr").inst[1:] == S.MBR_ROWS[7] and route(U(96, 576, 96, 1, 2, 14, 14), "mbr").waves == 4
    assert route(U(96, 576, 96, 1, 2, 14, 14), "blk").kernel == "mbw"                               # no block shape: the wave kernel whatever the switch
    assert route(U(24, 144, 32, 2, 2, 56, 56), "mbr").OC == 15 and route(U(32, 192, 64, 2, 2, 28, 28), "mbr").OC == 7
    assert route(U(24, 144, 24, 1, 2, 56, 56, acts=(RELU, RELU6)), "mbr").kernel == "mbw"           # launch-time codes: no mbr instance
    assert route(U(24, 144, 24, 1, 2, 56, 56), "mbw").tw == 8 and route(U(24, 144, 24, 1, 2, 48, 48), "mbw").tw == 16
    assert route(U(24, 144, 24, 1, 2, 56, 56), "blk").kernel == "blk"
    assert unsupported(U(96, 576, 32, 1, 1, 28, 28)) is not None                                    # 576 x 96 on block tiles: over the LDS budget
    assert unsupported(U(64, 144, 32, 1, 2, 8, 23)) is not None and unsupported(U(64, 144, 32, 1, 2, 8, 24)) is None
    assert unsupported(U(24, 40, 24, 1, 2, 8, 13)) is not None and unsupported(U(24, 40, 24, 1, 2, 8, 14)) is None
    for name, bad in S.REFUSED.items():
        assert unsupported(bad) is not None, name


# ---- 6. coverage -------------------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_reachable_instance():
    """every instance of the three kernels: since the block kernel lost its six-row-tile variants, none is unreachable"""
    reached = {(route(c.u, c.k).kernel, route(c.u, c.k).inst) for c in EXACT + BOUNDED}
    for c in EXACT + BOUNDED:
        assert unsupported(c.u) is None and route(c.u, c.k).kernel == c.want, case_id(c)
    mbr = {("mbr", (a,) + row) for a in (RELU, RELU6) for row in S.MBR_ROWS}
    mbw = {("mbw", (a,) + row) for a in (-1, RELU, RELU6) for row in S.MBW_ROWS}
    # block tiles: mbconv_kernel<DT, S, EXPAND> is compiled for two projection row tiles (Cout <= 32) and nothing else, so these four
    # per dtype are EVERY instance of it
    blk = {("blk", (s, e)) for s in (1, 2) for e in (True, False)}
    assert re.search(r"^constexpr int kMbRowT = 2;", _src("mbconv.hpp"), re.M) and "MAXRT" not in _src("mbconv.hpp")
    assert len(re.findall(r"mbconv_kernel<DT, [12], (?:true|false)>", _src("pcv_api.hip"))) == 4
    missing = (mbr | mbw | blk) - reached
    assert not missing, sorted(missing, key=repr)
    assert reached <= (mbr | mbw | blk)
    # the exact family alone carries the geometry: every instance but the launch-time-activation ones with general codes is in it too
    exact = {(route(c.u, c.k).kernel, route(c.u, c.k).inst) for c in EXACT}
    assert (mbr | mbw | blk) - exact == set(), sorted((mbr | mbw | blk) - exact, key=repr)
    assert len(EXACT) * 2 + len(BOUNDED) * 2 <= 500
