"""
CPU proofs behind tests/test_gpu_bnu_sweep.py (the fused stage-1 bottleneck unit, csrc/bnu.hpp):
  * the reference of tests/bnu_ref.py, without its rounding points, equals torch's float64 composition of the three convolutions;
  * the exact family's certificate holds for every swept case;
  * an emulated fp32 kernel - the kernel's own row-streaming structure: (image, band) items, the 4-slot t1 ring with its zero columns,
    the t2 row buffer, conv1 recomputed on a band's halo rows, the skip taken two steps behind conv1 - equals the exact family bit for
    bit and stays inside the bounded family's bound, on every swept case and band split;
  * each of the kernel bugs below leaves the bound on at least one swept case (and breaks the exact comparison on one): the sweep can
    tell them from a correct kernel.
The correct emulation passing every case is also what shows that the operands keep the reference itself inside the bounds.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from bnu_ref import CM, CO, NONE, RESNET, W, Unit, bounded_operands, certified, cin_of, exact_operands, exact_result, unit_ref
from test_gpu_bnu_sweep import DTYPES16, SHAPES, bands_of, case_id, cases, route, seed_of
from test_gpu_dw_se import TDT, act64

BUGS = ("halo_top", "halo_bottom", "col_left", "col_right", "slot", "skip_row", "carry", "band_halo")


# ---- the reference against torch ----------------------------------------------------------------------------------------------------------
def _torch_unit(u, ops):
    def bn(t, s, h):
        return t * s.double()[None, :, None, None] + h.double()[None, :, None, None]
    x = ops.x.double().permute(0, 3, 1, 2)
    t1 = act64(bn(F.conv2d(x, ops.w1.double()), ops.scale1, ops.shift1), u.act1)
    t2 = act64(bn(F.conv2d(t1, ops.w2.double(), padding=1), ops.scale2, ops.shift2), u.act2)
    a = act64(bn(F.conv2d(t2, ops.w3.double()), ops.scale3, ops.shift3), u.act3)
    skip = bn(F.conv2d(x, ops.wid.double()), ops.scale_id, ops.shift_id) if u.idconv else x
    return act64(a + skip, u.post).permute(0, 2, 3, 1)


@pytest.mark.parametrize("u", [Unit(2, 3, False, *RESNET), Unit(1, 5, True, *RESNET), Unit(2, 2, True, 2, 0, 1, 2)], ids=case_id)
def test_unrounded_reference_equals_torch_float64_composition(u):
    ops = bounded_operands(u, "bf16", 77)
    y = unit_ref(u, ops, "bf16", rounded=False)[0]
    t = _torch_unit(u, ops)
    assert y.shape == t.shape == (u.N, u.H, W, CO)
    assert float((y - t).abs().max()) <= 1e-12 * max(1.0, float(t.abs().max()))


def test_rounding_points_move_the_reference():
    """the rounded reference is not the unrounded one (the three rounding points are really there), yet within its own bound of it"""
    u = Unit(1, 3, True, *RESNET)
    ops = bounded_operands(u, "bf16", 78)
    y, bound = unit_ref(u, ops, "bf16")[:2]
    y0 = unit_ref(u, ops, "bf16", rounded=False)[0]
    assert float((y - y0).abs().max()) > 0
    assert bool(((y - y0).abs() <= bound).all())


# ---- the emulated kernel ------------------------------------------------------------------------------------------------------------------
def _act32(v, code):
    return v if code == NONE else (v.clamp(min=0) if code == 1 else v.clamp(0, 6))


def emulate(u, ops, dtype, band=0, bug=None):
    """what an fp32 kernel with bnu.hpp's structure stores, as a tensor of the storage type; `bug`: one of BUGS"""
    t = TDT[dtype]

    def rnd(v):
        return v.to(t).float()
    N, H = u.N, u.H
    band = H if band <= 0 else min(band, H)
    x = ops.x.float()
    w1 = ops.w1.float().reshape(CM, -1).t().contiguous()
    w2 = ops.w2.float().permute(2, 3, 1, 0).contiguous()            # [r][q][in][out]
    w3 = ops.w3.float().reshape(CO, CM).t().contiguous()
    wid = ops.wid.float().reshape(CO, -1).t().contiguous() if u.idconv else None
    s1, h1, s2, h2, s3, h3 = [v.float() for v in (ops.scale1, ops.shift1, ops.scale2, ops.shift2, ops.scale3, ops.shift3)]
    y = torch.full((N, H, W, CO), float("nan"))
    ring = [torch.zeros(W + 2, CM) for _ in range(4)]                # position p holds pixel p - 1; positions 0 and 57 stay zero
    for slot in ring:
        if bug == "col_left":
            slot[0] = 1.0
        if bug == "col_right":
            slot[W + 1] = 1.0
    t2 = torch.zeros(W, CM)
    for n in range(N):
        for r0 in range(0, H, band):
            r1 = min(H, r0 + band)
            for s in range(r0 - 1, r1 + 2):
                # phase 1: conv1 on row s; conv3 + skip on row s - 2
                if s <= r1:
                    slot = ring[s % 4]
                    inside = 0 <= s < H
                    if inside and not (bug == "band_halo" and ((s == r0 - 1) or (s == r1))):
                        slot[1:W + 1] = rnd(_act32((x[n, s] @ w1) * s1 + h1, u.act1))
                    elif bug == "carry" and s < 0 and n > 0:
                        pass                                          # the previous image's row stays in the slot
                    elif (bug == "halo_top" and s < 0) or (bug == "halo_bottom" and s >= H):
                        slot[1:W + 1] = 1.0
                    else:
                        slot[1:W + 1] = 0.0
                if s >= r0 + 2:
                    row = s - 2
                    xs = x[n, min(row + 1, H - 1) if bug == "skip_row" else row]
                    skip = rnd((xs @ wid) * ops.scale_id.float() + ops.shift_id.float()) if u.idconv else xs
                    y[n, row] = rnd(_act32(_act32((t2 @ w3) * s3 + h3, u.act3) + skip, u.post))
                # phase 2: conv2 on t1 rows s - 2 .. s
                if r0 + 1 <= s <= r1:
                    acc = torch.zeros(W, CM)
                    for r in range(3):
                        src = ring[(s - 2 + r + (1 if bug == "slot" else 0)) % 4]
                        for q in range(3):
                            acc = acc + src[q:q + W] @ w2[r, q]
                    t2 = rnd(_act32(acc * s2 + h2, u.act2))
    return y.to(t)


@functools.lru_cache(maxsize=4)
def _exact(u, dtype):
    ops = exact_operands(u, seed_of(u, "exact"))
    return ops, exact_result(u, ops, dtype).float()


@functools.lru_cache(maxsize=4)
def _bounded(u, dtype):
    ops = bounded_operands(u, dtype, seed_of(u, "bounded"))
    y, bound = unit_ref(u, ops, dtype)[:2]
    return ops, y, bound


def _emulated_bands(u):
    return [b for b in bands_of(u.H) if b != 0]


def _inside(y, ref, bound):
    return bool(((y.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("u", cases(), ids=case_id)
def test_emulated_kernel_passes_both_families_on_every_band_split(u, dtype):
    ops, ref = _exact(u, dtype)
    ok, worst = certified(u, ops, dtype)
    assert ok, "certificate: {:.3e} >= 2^24".format(worst)
    bops, bref, bound = _bounded(u, dtype)
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    for band in _emulated_bands(u):
        y = emulate(u, ops, dtype, band).float()
        assert torch.equal(y, ref), "exact family, band {}: {} elements differ".format(band, int((y != ref).sum()))
        y = emulate(u, bops, dtype, band).float()
        assert _inside(y, bref, bound), "bounded family, band {}: worst ratio {:.3f}".format(
            band, float(((y.double() - bref).abs() / bound).max()))


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("bug", BUGS)
def test_every_bug_model_leaves_the_bound_and_the_exact_family_somewhere(bug, dtype):
    """walks the swept cases (ResNet epilogue) and their band splits until the bug shows in each family"""
    hit_bound = hit_exact = None
    for idconv in (False, True):
        for n, h in SHAPES:
            u = Unit(n, h, idconv, *RESNET)
            for band in _emulated_bands(u):
                if hit_bound is None:
                    bops, bref, bound = _bounded(u, dtype)
                    if not _inside(emulate(u, bops, dtype, band, bug).float(), bref, bound):
                        hit_bound = (case_id(u), band)
                if hit_exact is None:
                    ops, ref = _exact(u, dtype)
                    if not torch.equal(emulate(u, ops, dtype, band, bug).float(), ref):
                        hit_exact = (case_id(u), band)
            if hit_bound and hit_exact:
                break
        if hit_bound and hit_exact:
            break
    assert hit_bound is not None, "no swept case tells the bug `{}` from a correct kernel by the bound".format(bug)
    assert hit_exact is not None, "no swept case tells the bug `{}` from a correct kernel bit for bit".format(bug)


def test_band_splits_cover_what_the_issue_of_each_shape_is():
    """whole images, bands of 1 and 4, a ragged last band wherever the height allows one; the restated routing takes every split"""
    for n, h in SHAPES:
        bs = bands_of(h)
        assert h in bs and 0 in bs and 1 in bs and min(4, h) in bs
        if h > 2:
            assert any(0 < b < h and h % b for b in bs), (h, bs)
        for b in bs:
            R = route(n, h, W, 256, CM, CM, CO, "bf16", RESNET, False, bnu_band=b, max_blocks=2, num_cu=256)
            assert R.ok and R.nItems == n * R.nBands and R.grid == min(2, R.nItems) and (R.nBands - 1) * R.band < h <= R.nBands * R.band
    assert cin_of(Unit(1, 1, True, *RESNET)) == 64 and cin_of(Unit(1, 1, False, *RESNET)) == 256
