"""
CPU checks of the fused 1x1 pair sweep in tests/test_gpu_pair_sweep.py, over the same case list (all_cases()): the reference composition
of tests/pair_ref.py equals a float64 F.conv2d chain; an emulated kernel (fp32 matmul, y1 rounded to the storage type, a second fp32
matmul from the rounded y1; the identity form's skip rounded to the storage type) stays at or below both bounds on EVERY case and dtype;
and the bounds are tight enough to fail: each kernel-bug model below leaves them on every case whose shape can tell it from the correct
kernel. The models are applied to the emulated kernel; "cannot tell" is stated per model (relevant_mutants restates it in code):
  drop_chunk        one 64-channel chunk of y1 (the second) is missing from GEMM2                          every case can tell
  chunk_xor         chunk c of y1 meets the K-slice of W2 that belongs to chunk c ^ 1                     every case can tell
  res_next_chunk    the residual (the computed skip of the identity form) of chunk c + 1 is added to chunk c     every case can tell
  gate_first_image  the gate row of a tile's first image is applied to the pixels of its second image: gated forms only; not where no tile
                    holds pixels of two images (N = 1; HW a multiple of the tile: (2, 4, 8) at 32 pixels, (5, 8, 16) at 128)
  gate_block_image  a 16-pixel block takes the gate row of its first pixel's image: gated forms only; not where HW is a multiple of 16 or N = 1
  gate_clamp_early  the gate image index is clamped to N - 2 instead of N - 1: gated forms only; not where N = 1.
                    (The opposite bug, the index of the last tile's second image NOT clamped, reads the row behind the last image into
                    LDS but no stored pixel belongs to that image: no value can tell it. The GPU file puts a NaN row there, which shows
                    it as soon as such a row reaches a pixel; the read itself is covered by reading the code only.)
  drop_wave_kslice  the narrow kernels' LDS reduction leaves out the last wave's K-slice (y1 channels 192 .. 255) for the second
                    16-pixel block of each tile: narrow forms only; not where M <= 16
  swap_halves       the two 128-channel halves of y2 are exchanged: the 256-channel forms only
  act_swap          act1 and post1 exchanged: not where act1 == post1
  tail_block        the last, partial 16-pixel block is not written (y1 and y2 keep their NaNs): not where M is a multiple of 16
  unrounded_y1      y2 computed from the fp32 y1 instead of the stored one. It moves the sum by about sqrt(C1) / 2 input ulps of |y1||w2|
                    (a random walk), while the accumulation allowance of the bound, (K + 3) 2^-23 S with K = C1, grows like C1.
                    bf16 (input ulp 2^-8), C1 <= 512: the deviation is several times the bound wherever |y2| is small and not
                    clamped: told on every such case, M = 1 included (asserted). C1 = 1024: the two are of one size (about 5e-4 |y1|
                    against 2^-13 S, S about 13); told on most cases, not on all, so not claimed.
                    fp16 (input ulp 2^-11): the deviation is at or below the allowance from K = 256 on. The bound cannot tell it
                    (measured on this list: told on the narrow cases, on half of the wide ones not), so it is not claimed.
The lists of the GPU file are also checked for what each shape is there for, and WPairCfg's LDS arithmetic (pair_ref.wpair_layout) for
the values the host routes by.
"""

import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import util
from conv_ref import round_to
from pair_ref import NARROW_TILE, WPAIR_CONFIGS, wpair_layout, y1_ref_bound, y2_ref_bound
from test_gpu_dw_se import NONE, RELU, act64
from test_gpu_pair_sweep import (DTYPES16, EPILOGUE_SHAPE, EPILOGUES, FORMS, GATE_GLOBAL_SHAPES, GATE_LDS_SHAPES, HW127, NARROW_SHAPES,
                                 RESNET, WIDE_SHAPES, Case, all_cases, case_id, case_operands, cases_of, route, route_case, shapes_of)

MUTANTS = ("drop_chunk", "chunk_xor", "res_next_chunk", "gate_first_image", "gate_block_image", "gate_clamp_early", "drop_wave_kslice",
           "swap_halves", "act_swap", "tail_block", "unrounded_y1")


# ---- 1. the reference against torch ----------------------------------------------------------------------------------------------------------
def _conv64(x, w):
    """float64 F.conv2d of NHWC x with OIHW w, NHWC"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double()).permute(0, 2, 3, 1)


@pytest.mark.parametrize("form", list(FORMS))
def test_reference_equals_a_float64_conv2d_chain(form):
    for epi in [RESNET] + EPILOGUES:
        c = Case(form, *EPILOGUE_SHAPE, *epi)
        ops = case_operands(c, "bf16")
        ref1, _ = y1_ref_bound(ops, c.act1, c.post1, "bf16")
        v = act64(_conv64(ops.x, ops.w1) * ops.scale1.double() + ops.shift1.double(), c.act1)
        if ops.gate is not None:
            v = v * ops.gate.double()[:, None, None, :]
        if ops.x0 is not None:
            v = v + (_conv64(ops.x0, ops.wid) * ops.scale_id.double() + ops.shift_id.double())
        else:
            v = v + ops.res.double()
        want1 = act64(v, c.post1)
        assert float((ref1 - want1).abs().max()) <= 1e-12 * float(want1.abs().max())
        y1 = round_to(want1, "bf16")
        ref2, _ = y2_ref_bound(y1, ops, c.act2, "bf16")
        want2 = act64(_conv64(y1, ops.w2) * ops.scale2.double() + ops.shift2.double(), c.act2)
        assert float((ref2 - want2).abs().max()) <= 1e-12 * float(want2.abs().max())


# ---- 2. the emulated kernel and its bug models ----------------------------------------------------------------------------------------------------
def image_index(c, tile, mutant=None):
    """per pixel: the image whose gate row the (mutated) kernel applies"""
    M, HW = c.N * c.H * c.W, c.H * c.W
    pix = torch.arange(M)
    img = pix // HW
    if mutant == "gate_first_image":
        first = (pix // tile * tile) // HW
        img = torch.where(img == first + 1, first, img)
    elif mutant == "gate_block_image":
        img = (pix // 16 * 16) // HW
    elif mutant == "gate_clamp_early":
        img = img.clamp(max=max(c.N - 2, 0))
    return img


def relevant_mutants(c, dtype):
    """the bug models the shape (and epilogue) of a case can tell from the correct kernel - the module docstring in code"""
    f = FORMS[c.form]
    M = c.N * c.H * c.W
    m = ["drop_chunk", "chunk_xor", "res_next_chunk"]
    if f.gated:
        m += [g for g in ("gate_first_image", "gate_block_image", "gate_clamp_early")
              if not torch.equal(image_index(c, f.tile, g), image_index(c, f.tile))]
    if f.CM == 64 and M > 16:
        m.append("drop_wave_kslice")
    if f.CM == 256:
        m.append("swap_halves")
    if c.act1 != c.post1:
        m.append("act_swap")
    if M % 16:
        m.append("tail_block")
    if dtype == "bf16" and f.C1 <= 512:
        m.append("unrounded_y1")
    return m


def emulate(c, ops, dtype, mutant=None):
    """(y1, y2) of an fp32 kernel on the case's operands, each rounded to the storage type; NHWC float32 (16-bit values, exact)"""
    f = FORMS[c.form]
    M, CM, C1 = c.N * c.H * c.W, f.CM, f.C1
    act1, post1 = (c.post1, c.act1) if mutant == "act_swap" else (c.act1, c.post1)
    v = act64((ops.x.reshape(M, CM) @ ops.w1.reshape(C1, CM).t()) * ops.scale1 + ops.shift1, act1)
    if ops.gate is not None:
        v = v * ops.gate[image_index(c, f.tile, mutant)]
    if ops.x0 is not None:
        res = round_to((ops.x0.reshape(M, CM) @ ops.wid.reshape(C1, CM).t()) * ops.scale_id + ops.shift_id, dtype)
    else:
        res = ops.res.reshape(M, C1)
    if mutant == "res_next_chunk":
        res = res.roll(-64, dims=1)
    v = act64(v + res, post1)
    assert v.dtype == torch.float32
    y1 = round_to(v, dtype)
    src = (v if mutant == "unrounded_y1" else y1).clone()
    w2 = ops.w2.reshape(CM, C1)
    if mutant == "drop_chunk":
        src[:, 64:128] = 0
    elif mutant == "chunk_xor":
        src = src.view(M, C1 // 128, 2, 64).flip(2).reshape(M, C1)
    z = src @ w2.t()
    if mutant == "drop_wave_kslice":
        rows = (torch.arange(M) % f.tile) // 16 == 1
        z[rows] = src[rows, :192] @ w2[:, :192].t()
    y2 = round_to(act64(z * ops.scale2 + ops.shift2, c.act2), dtype)
    assert z.dtype == torch.float32
    if mutant == "swap_halves":
        y2 = torch.cat((y2[:, 128:], y2[:, :128]), dim=1)
    elif mutant == "tail_block":
        y1[M // 16 * 16:] = float("nan")
        y2[M // 16 * 16:] = float("nan")
    return y1.view(c.N, c.H, c.W, C1), y2.view(c.N, c.H, c.W, CM)


_STATS = os.environ.get("PCV_PAIR_SWEEP_STATS")       # the GPU file's switch: here the emulation's error / bound, one JSON line per comparison


def _note(c, dtype, out, ratio):
    if _STATS:
        with open(_STATS, "a") as fh:
            fh.write(json.dumps(dict(form=c.form, dtype=dtype, grid="emulation", out=out, case=case_id(c), ratio=ratio)) + "\n")


@pytest.mark.parametrize("f,c,dtype", [pytest.param(f, c, dt, id=case_id(c) + "-" + dt) for f, c, dt in all_cases()])
def test_emulated_kernel_inside_and_bug_models_outside_the_bounds(f, c, dtype):
    ops = case_operands(c, dtype)
    ref1, bound1 = y1_ref_bound(ops, c.act1, c.post1, dtype)
    y1, y2 = emulate(c, ops, dtype)
    ref2, bound2 = y2_ref_bound(y1, ops, c.act2, dtype)
    for out, y, ref, bound in (("y1", y1, ref1, bound1), ("y2", y2, ref2, bound2)):
        assert y.shape == ref.shape
        ratio = float(((y.double() - ref).abs() / bound).max())
        _note(c, dtype, out, ratio)
        assert ratio <= 1.0, "the correct kernel leaves the {} bound (error / bound = {:.3f}): the derivation is wrong".format(out, ratio)
    for m in relevant_mutants(c, dtype):
        b1, b2 = emulate(c, ops, dtype, m)
        if not bool(((b1.double() - ref1).abs() <= bound1).all()):
            continue                                             # told by y1 (NaN included)
        r2, bd2 = (ref2, bound2) if torch.equal(b1, y1) else y2_ref_bound(b1, ops, c.act2, dtype)
        assert not bool(((b2.double() - r2).abs() <= bd2).all()), "{} is not told from the correct kernel".format(m)


def test_every_bug_model_is_relevant_somewhere_and_none_everywhere_excluded():
    for dt in DTYPES16:
        seen = set()
        for f, c, d in all_cases():
            if d == dt:
                seen |= set(relevant_mutants(c, dt))
        assert seen == set(MUTANTS) - ({"unrounded_y1"} if dt == "fp16" else set()), set(MUTANTS) - seen
    for f in FORMS.values():                                     # per form: everything that form can show is shown by some case of it
        seen = set().union(*[relevant_mutants(c, "bf16") for c in cases_of(f)])
        want = set(MUTANTS)
        if not f.gated:
            want -= {"gate_first_image", "gate_block_image", "gate_clamp_early"}
        if f.CM != 64:
            want -= {"drop_wave_kslice"}
        if f.CM != 256:
            want -= {"swap_halves"}
        if f.C1 > 512:
            want -= {"unrounded_y1"}
        assert seen == want, (f.name, want - seen)


# ---- 3. WPairCfg's LDS arithmetic (csrc/wpair1x1.hpp) ------------------------------------------------------------------------------------------------
def test_wpair_layout_restates_the_header():
    want = {(128, 512): (32768, 65536, 70656, True), (256, 1024): (65536, 147456, 157696, False),
            (128, 256): (32768, 65536, 68608, True), (256, 512): (65536, 147456, 153600, False)}
    assert set(WPAIR_CONFIGS) == set(want)
    for (cm, c1), (slot, tab, lds, gate_lds) in want.items():
        G = wpair_layout(cm, c1)
        assert (G.SLOT, G.TAB, G.LDS, G.GATE_LDS) == (slot, tab, lds, gate_lds), G
        assert G.P == 128 and G.NCH == c1 // 64 and G.NCH % 2 == 0 and G.NW == (8 if cm > 128 else 4)
        assert G.LDS_GATED == lds + (16 * c1 if gate_lds else 0) <= 160 * 1024
        assert G.TAB == 2 * G.SLOT + G.XCH and G.LDS == G.TAB + 4 * (2 * c1 + 2 * cm)
    assert NARROW_TILE == {2: 32, 4: 64}
    assert {f.tile for f in FORMS.values() if f.CM >= 128} == {128}
    assert {f.name: f.tile for f in FORMS.values() if f.CM == 64} == {"pb4": 64, "pb2": 32, "gated": 32, "idconv": 32}
    assert {f.name for f in FORMS.values() if f.gate_in_lds} == {"w128x512g", "w128x256g"}
    # the expressions restated are still the header's
    with open(os.path.join(os.path.dirname(util.HERE), "pytorchcv_amd", "csrc", "wpair1x1.hpp")) as fh:
        src = fh.read()
    for text in ("A1B = (CM / 64) * 64 * 128;", "A2B = CM * 128;", "SLOT = A1B + A2B;", "XCH = PAIRW ? NWP * 2 * PBW * 1024 : 0;",
                 "TAB = 2 * SLOT + XCH;", "LDS = TAB + (2 * C1 + 2 * CM) * 4;", "GATE_LDS = LDS + 4 * C1 * 4 <= 80 * 1024;",
                 "PAIRW = CM > 128;", "NWP = 4;", "PBW = 2;", "P = 16 * PBW * NWP;"):
        assert text in src, text
    with open(os.path.join(os.path.dirname(util.HERE), "pytorchcv_amd", "csrc", "pair1x1.hpp")) as fh:
        assert "P = 16 * PB;" in fh.read()
    with open(os.path.join(os.path.dirname(util.HERE), "pytorchcv_amd", "csrc", "pcv_api.hip")) as fh:
        api = fh.read()
    for i, (cm, c1) in enumerate(WPAIR_CONFIGS):
        assert re.search(r"if \(cm == {} && c1 == {}\) return {};".format(cm, c1, i), api), (cm, c1)


# ---- 4. the lists: each shape has the property it is there for ------------------------------------------------------------------------------------------
def _tiles(shape, tile):
    M = shape[0] * shape[1] * shape[2]
    return -(-M // tile)


def _straddling(shape, tile):
    """tiles that hold pixels of more than one image, as (tile, first pixel of the second image inside it)"""
    N, HW = shape[0], shape[1] * shape[2]
    out = []
    for t in range(_tiles(shape, tile)):
        lo, hi = t * tile, min((t + 1) * tile, N * HW) - 1
        if lo // HW != hi // HW:
            out.append((t, (lo // HW + 1) * HW - lo))
    return out


def test_every_form_is_listed_in_both_types_with_every_epilogue():
    assert len(FORMS) == 12 and len({f.kernel for f in FORMS.values()}) == 12
    assert {f.kernel for f in FORMS.values() if f.CM == 64} == {("pair1x1", 4, False, False), ("pair1x1", 2, False, False),
                                                                ("pair1x1", 2, False, True), ("pair1x1", 2, True, False)}
    assert {f.kernel for f in FORMS.values() if f.CM >= 128} == {("wpair1x1", cm, c1, g) for cm, c1 in WPAIR_CONFIGS for g in (False, True)}
    got = {}
    for f, c, dt in all_cases():
        got.setdefault((f.name, dt), []).append(c)
    assert set(got) == {(n, dt) for n in FORMS for dt in DTYPES16}
    for (name, dt), cs in got.items():
        f = FORMS[name]
        assert all(route_case(c).ok and route_case(c).kernel == f.kernel and route_case(c).gate_in_lds == f.gate_in_lds for c in cs), name
        epi = [(c.act1, c.post1, c.act2) for c in cs if (c.N, c.H, c.W) == EPILOGUE_SHAPE]
        assert set(epi) == set(EPILOGUES) | {RESNET}, name
        assert all((c.act1, c.post1, c.act2) == RESNET for c in cs if (c.N, c.H, c.W) != EPILOGUE_SHAPE), name
    assert EPILOGUES[:7] == [(1, 0, 0), (2, 2, 2), (0, 0, 6), (6, 1, 4), (4, 6, 3), (3, 0, 5), (5, 2, 1)]      # the list asked for, in act codes
    for site in range(3):                                        # all seven codes at each of the three sites
        assert {e[site] for e in EPILOGUES} == set(range(7)), site


def test_shapes_have_the_properties_they_are_listed_for():
    def M(s):
        return s[0] * s[1] * s[2]
    # narrow forms: tiles of 32 and 64 pixels
    assert NARROW_SHAPES[:5] == [(1, 1, 1), (1, 5, 7), (2, 4, 8), (3, 13, 11), (9, 14, 14)]
    assert M((1, 5, 7)) == 35 and M((2, 4, 8)) == 64 and M((3, 13, 11)) % 16 != 0
    for tile in (32, 64):
        n = _tiles((9, 14, 14), tile)
        assert n >= 3 * 8 and M((9, 14, 14)) % tile != 0, (tile, n)       # at least three rounds on the capped grid (the x ring wraps), a partial last tile
    assert _tiles((9, 14, 14), 64) % 8 != 0                               # ... and a ragged last round for the 64-pixel tiles
    assert _tiles((7, 9, 9), 32) > 16 and _tiles((7, 9, 9), 32) % 8 != 0  # ... which (7, 9, 9) gives the 32-pixel tiles
    for f in FORMS.values():
        if f.CM == 64:
            assert shapes_of(f)[:6] == NARROW_SHAPES
    # gate from global memory: gated narrow and the gated 256-channel wide forms
    assert GATE_GLOBAL_SHAPES == [(40, 1, 1), (5, 1, 13)]
    assert (40, 1, 1)[1] * (40, 1, 1)[2] == 1                              # every pixel is another image
    assert len(_straddling((5, 1, 13), 16)) >= 3                           # image boundaries inside 16-pixel blocks
    for name in ("gated", "w256x1024g", "w256x512g"):
        f = FORMS[name]
        assert not f.gate_in_lds and set(NARROW_SHAPES[:5] + GATE_GLOBAL_SHAPES + [HW127]) <= set(shapes_of(f)), name
        assert any(_straddling((c.N, c.H, c.W), 16) for c in cases_of(f))  # several images inside one 16-pixel block
    # wide forms: tiles of 128 pixels
    assert M((1, 8, 16)) == 128 and M((1, 3, 43)) == 129
    n = _tiles((17, 12, 11), 128)
    assert n >= 17 and -(-n // 8) == 3 and n % 8 != 0 and M((17, 12, 11)) % 128 != 0        # three rounds on the capped grid, the last ragged, a partial last tile
    for f in FORMS.values():
        if f.CM >= 128 and not f.gate_in_lds:
            assert shapes_of(f)[:6] == WIDE_SHAPES, f.name
    # gate rows in LDS: the gated 128-channel wide forms
    for name in ("w128x512g", "w128x256g"):
        assert FORMS[name].gate_in_lds and shapes_of(FORMS[name]) == GATE_LDS_SHAPES == [(5, 8, 16), (5, 3, 43), (3, 13, 11), (17, 12, 11)]
    assert all(s[1] * s[2] >= 128 for s in GATE_LDS_SHAPES)
    assert 8 * 16 == 128 and _straddling((5, 8, 16), 128) == []            # a tile is an image ...
    assert _tiles((5, 8, 16), 128) == 5                                    # ... so the last tile's second image (index 5) does not exist: the nimg - 1 clamp
    st = _straddling((5, 3, 43), 128)
    assert 3 * 43 == 129 and [t for t, _ in st] == [1, 2, 3, 4] and len({o for _, o in st}) == 4       # every tile behind the first straddles, the offset drifts
    assert _tiles((5, 3, 43), 128) == 6 and st[-1][0] < 5                  # ... and the last tile again has no second image
    assert len(_straddling((17, 12, 11), 128)) >= 12 and _tiles((17, 12, 11), 128) >= 2 * 8 + 1      # both parities of the double buffer in one block
    # HW = 127
    assert HW127[1] * HW127[2] == 127 and HW127[0] >= 3 and len(_straddling(HW127, 128)) >= 2
    for cm, c1 in WPAIR_CONFIGS:
        assert route(cm, c1, cm, *HW127, gated=True).ok == (cm == 256)
    assert route(64, 256, 64, *HW127, gated=True).ok
    # the refusals of the GPU file, restated
    assert not route(128, 512, 128, 3, 13, 11, wpair=0).ok and not route(256, 512, 256, 3, 13, 11, wpair=0).ok
    assert route(128, 512, 128, 3, 13, 11, wpair=1).ok and not route(256, 512, 256, 3, 13, 11, wpair=1).ok
    assert route(64, 256, 64, 3, 13, 11, wpair=0).ok
    assert not route(64, 256, 64, 3, 13, 11, res2=True).ok and not route(64, 256, 64, 3, 13, 11, res1=False).ok
    assert not route(64, 256, 64, 3, 13, 11, y1_cpitch=320).ok and not route(128, 512, 128, 3, 13, 11, idconv=True).ok
    assert route(64, 256, 64, 3, 13, 11, pair_pb=4).kernel == ("pair1x1", 4, False, False)
    assert route(64, 256, 64, 3, 13, 11, pair_pb=4, gated=True).kernel == ("pair1x1", 2, False, True)
    assert RESNET == (NONE, RELU, RELU)
