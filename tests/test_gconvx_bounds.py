"""
CPU checks of the any-width grouped 3x3 sweep in tests/test_gpu_gconvx_sweep.py: an fp32 emulation of csrc/gconvx.hpp that follows
the kernel's own tiles, window, K order and zero padding (tests/gconvx_ref.py) stays inside the derived bound of tests/conv_ref.py for
EVERY case the GPU sweep launches, and the bound is tight enough to fail: on every case each bug model its geometry can tell from the
correct kernel leaves the bound somewhere, in both storage types. The case list is also checked for what the sweep promises: the
required shapes, one case on each side of every boundary of the planner, and the routing of today's sweep families left where it was.
"""

import functools
import os
import re

import pytest

import gconvx_ref as gx
from gconvx_ref import CASES, CLASS_DECLINED, DECLINED, DTYPES16, MUTANTS, case_id, plan_gconvx, route


@functools.lru_cache(maxsize=4)
def _reference(c, dtype):
    return gx.case_reference(c, dtype)


@pytest.mark.parametrize("c,dtype", [pytest.param(c, dt, id=case_id(c) + "-" + dt) for c in CASES for dt in DTYPES16])
def test_emulated_kernel_inside_and_bug_models_outside_the_bound(c, dtype):
    ops, ref, bound = _reference(c, dtype)
    y = gx.emulate(c, ops, dtype)
    assert y.shape == ref.shape
    ratio = float(((y - ref).abs() / bound).max())
    assert ratio <= 1.0, "the correct kernel leaves the bound (error / bound = {:.3f})".format(ratio)
    for m in gx.relevant_mutants(c, dtype):
        bug = gx.emulate(c, ops, dtype, m)
        assert bool(((bug - ref).abs() > bound).any()), "{} is not told from the correct kernel".format(m)


def test_every_bug_model_is_relevant_somewhere():
    seen = set()
    for c in CASES:
        seen |= set(gx.relevant_mutants(c, "bf16"))
    assert seen == set(MUTANTS)


def test_case_list_is_the_required_one_with_both_sides_of_every_planner_boundary():
    shapes = {(c.N, c.Cin, c.Cin // c.groups, c.H, c.W, c.sh) for c in CASES}
    required = {(2, 24, 8, 6, 10, 2), (2, 56, 8, 5, 7, 1), (3, 152, 8, 4, 6, 1), (2, 72, 24, 6, 8, 2), (3, 120, 24, 7, 5, 1),
                (2, 80, 40, 5, 9, 1), (2, 240, 40, 8, 8, 2), (2, 96, 48, 7, 7, 1), (2, 168, 56, 6, 6, 2),
                (2, 48, 16, 9, 11, 1), (1, 24, 8, 4, 112, 2), (1, 48, 24, 4, 112, 2)}
    assert required <= shapes
    # (the two 64-per-group shapes of the required list went back to the generic kernel with their class: CLASS_DECLINED runs them there)
    assert {(2, 128, 64, 14, 14, 2), (1, 192, 64, 7, 7, 1)} <= {(c.N, c.Cin, c.Cin // c.groups, c.H, c.W, c.sh) for c in CLASS_DECLINED}
    plans = {(c.N, c.Cin, c.Cin // c.groups, c.H, c.W, c.sh): route(c, "bf16") for c in CASES}
    assert all(p is not None for p in plans.values())
    assert {c.Cin // c.groups for c in CASES} == set(gx.WIDTHS) - {64}
    assert {c.groups for c in CASES} >= {2, 3, 5, 7, 19}
    # tile size: 64 pixels run the 4-block instantiation, 65 the 7-block one
    assert plans[(1, 16, 8, 3, 64, 1)][:3] == (1, 2, 0) and plans[(1, 16, 8, 3, 65, 1)][:3] == (1, 2, 1)
    # row count: 112 / Wo rows
    assert plans[(1, 16, 8, 4, 56, 1)].R == 2 and plans[(1, 16, 8, 3, 57, 1)].R == 1
    # LDS budget: the 112-wide stride-2 window holds two rows of three 8-wide groups, but two 24-wide groups only at one row ...
    assert plans[(1, 24, 8, 4, 112, 2)][:2] == (2, 3) and plans[(1, 48, 24, 4, 112, 2)][:2] == (1, 2)
    # ... and five of seven 8-wide groups at two rows: two channel blocks
    p = plans[(1, 56, 8, 2, 112, 2)]
    assert (p.R, p.GB, p.nCB) == (2, 4, 2) and p.lds <= gx.MAX_LDS
    # channel block: 128 / Cg groups, evened out over the blocks; 19 groups run as 10 + 9
    assert (plans[(3, 120, 24, 7, 5, 1)].GB, plans[(3, 120, 24, 7, 5, 1)].nCB) == (5, 1)
    assert (plans[(2, 144, 24, 5, 5, 1)].GB, plans[(2, 144, 24, 5, 5, 1)].nCB) == (3, 2)
    assert (plans[(3, 152, 8, 4, 6, 1)].GB, plans[(3, 152, 8, 4, 6, 1)].nCB) == (10, 2)
    assert (3 * 4) % plans[(3, 152, 8, 4, 6, 1)].R != 0                  # the tail tile is partial
    for c in CASES:
        p = route(c, "bf16")
        assert p.lds <= gx.MAX_LDS and p.R * ((c.W - 1) // c.sh + 1) <= 16 * gx.PB[p.pbi] and p.pitch // 16 % 2 == 1
        assert route(c, "fp16") == p and route(c, "fp32") is None
    assert {c.act for c in CASES if (c.N, c.Cin, c.H, c.W) == (2, 56, 5, 7)} == {0, 1, 2}
    assert all(route(c, dt) is None and gx.gconvx_static(c, dt) for c in DECLINED + CLASS_DECLINED for dt in DTYPES16)
    # the measured classes: one case on each side of every edge of gconvx_pays
    assert not gx.gconvx_pays(48, 2, 28) and not gx.gconvx_pays(48, 2, 56) and gx.gconvx_pays(48, 2, 26) and gx.gconvx_pays(48, 2, 58)
    assert not gx.gconvx_pays(56, 2, 58) and gx.gconvx_pays(56, 2, 56) and not gx.gconvx_pays(56, 1, 30) and gx.gconvx_pays(56, 1, 28)
    assert all(gx.gconvx_pays(cg, s, W) for cg in (8, 16, 24) for s in (1, 2) for W in (7, 28, 56, 112))
    assert not any(gx.gconvx_pays(64, s, W) for s in (1, 2) for W in (7, 14, 28, 56, 112))
    assert {(1, 96, 48, 4, 26, 2), (1, 112, 56, 2, 56, 2), (1, 112, 56, 3, 28, 1)} <= shapes


def test_planner_refuses_what_the_kernel_cannot_tile():
    assert plan_gconvx(2, 15, 15, 8, 8, 2, 16) is None and plan_gconvx(2, 14, 15, 7, 8, 2, 16) is None
    assert plan_gconvx(1, 4, 113, 4, 113, 3, 8) is None and plan_gconvx(1, 4, 112, 4, 112, 3, 8) is not None
    # the widest group on the widest map still fits with one group per block
    p = plan_gconvx(2, 112, 112, 56, 56, 2, 64)                           # (the planner; the routing keeps 64 per group generic)
    assert (p.R, p.GB) == (1, 1) and p.lds <= gx.MAX_LDS


def test_existing_sweep_families_keep_their_route():
    """nothing of tests/test_gpu_conv_sweep.py moves to the new kernel: F6 / F7 (and their *_GENERIC rows) are P.gconv shapes, and F2's
    only Cin == Cout 3x3 layer with a width of the list (128 channels in 2 groups, stride 2) runs under gconvr = 0"""
    from test_gpu_conv_sweep import F2, F6_GENERIC, F7_GENERIC, FAMILIES, GENERIC
    for fam, (cases, dts) in FAMILIES.items():
        for c in cases:
            for dt in dts:
                tuned = c._replace(tune=tuple(sorted(dict(GENERIC if fam in ("F1", "F2", "F3", "F3f", "F4") else {}, **dict(c.tune)).items())))
                assert route(tuned, dt) is None, (fam, case_id(c), dt)
    assert any(gx.gconvx_static(c, "bf16") for c in F2)                   # ... which is why "gconvr" 0 switches the kernel off too
    assert not any(gx.gconvx_static(c, "bf16") for c in F6_GENERIC + F7_GENERIC)


def test_constants_match_the_library():
    import util
    root = os.path.dirname(util.HERE)
    with open(os.path.join(root, "pytorchcv_amd", "csrc", "gconvx.hpp")) as f:
        hdr = f.read()
    m = re.search(r"kGConvXMaxLds = (\d+) \* 1024;", hdr)
    assert m and int(m.group(1)) * 1024 == gx.MAX_LDS
    assert re.search(r"kGConvXPB\[2\] = \{4, 7\};", hdr)
    widths = re.search(r"#define GCONVX_WIDTHS\(X, DT, S, PB\) \\\n(.*)\n", hdr).group(1)
    assert tuple(int(v) for v in re.findall(r"S, (\d+), PB", widths)) == gx.WIDTHS
    with open(os.path.join(root, "pytorchcv_amd", "csrc", "pcv_api.hip")) as f:
        src = f.read()
    assert re.search(r"^\s*int use_gconvx = 1;", src, re.M) and '{"gconvx", &pcv_ctx::use_gconvx}' in src
    assert "W > 112" in src and gx.MAX_W == 112
