"""
CPU checks of the depthwise MixConv sweep in tests/test_gpu_mixconv.py: the float64 reference of tests/mixconv_ref.py agrees with
F.conv2d applied per channel group, its table holds the shapes the sweep promises, and its bound is tight enough to fail - on the
sweep's own inputs the float64 result of each plausible kernel bug violates the bound of the correct result somewhere:
  a group boundary moved by one chunk (channels 88-95 of the 90-wide case run with the 3x3 window), a small filter embedded at the
  corner of the larger window instead of its centre, the outer ring of the 9x9 / 11x11 filter dropped, group g's taps read at
  group g-1's offset, a row duplicated across a strip boundary, the stride-2 phase off by one on an odd map.
"""

import pytest
import torch
import torch.nn.functional as F

from test_gpu_dw_se import NONE, RELU, SWISH, bn_fold64, dw_ref
from test_gpu_mixconv import SHAPES, DTYPES, OTHER_CODES
from mixconv_ref import group_bounds, mix_operands, mix_plan, mix_ref, out_bound, split_channels, taps_of_group


def _inputs(shape, dtype):
    """the sweep's own operands of a shape (same seed rule as tests/test_gpu_mixconv.py), taps rounded to the storage type"""
    N, C, G, s, H, W = shape
    x, ws, bn = mix_operands(N, H, W, C, G, dtype, seed=100 * C + 10 * G + s)
    sc, sh = [t.float() for t in bn_fold64(bn)]
    return x, [taps_of_group(w, dtype) for w in ws], sc, sh


def test_table_holds_the_promised_shapes():
    assert (2, 360, 4, 1, 9, 11) in SHAPES and split_channels(360, 4) == [90, 90, 90, 90]
    assert [b for b, _ in group_bounds(360, 4)] == [0, 90, 180, 270]
    assert {(G, s) for (_, _, G, s, _, _) in SHAPES} >= {(2, 1), (3, 1), (3, 2), (4, 1), (4, 2), (5, 2)}
    assert any(H % 2 == 1 and W % 2 == 0 and s == 2 for (_, _, _, s, H, W) in SHAPES)
    assert any(H == 1 and W == 1 for (_, _, _, _, H, W) in SHAPES)
    assert any(H >= 40 for (_, _, _, _, H, _) in SHAPES)                 # more than one row strip per column
    assert set(OTHER_CODES) | {RELU, SWISH} == set(range(7))              # every activation code is run
    assert split_channels(40, 3) == [14, 13, 13]                          # the split the entry points refuse


def test_blob_plan_covers_every_channel_once():
    for (_, C, G, _, _, _) in SHAPES:
        for es in (2, 4):
            regions, total = mix_plan(C, G, es)
            assert regions[0][0] == 0 and sum(span for _, span, _ in regions) == C
            for (b, span, off), (b2, _, off2) in zip(regions, regions[1:]):
                assert b + span == b2 and off2 >= off and off % 16 == 0
            assert total % 16 == 0


@pytest.mark.parametrize("shape", [(2, 360, 4, 2, 7, 9), (2, 720, 5, 1, 6, 5), (1, 48, 3, 2, 8, 8), (2, 16, 2, 1, 5, 4), (1, 48, 3, 1, 4, 4)])
def test_float64_reference_matches_conv2d_per_group(shape):
    N, C, G, s, H, W = shape
    x, ws, bn = mix_operands(N, H, W, C, G, "fp32", seed=5)
    sc, sh = bn_fold64(bn)
    ref, _ = mix_ref(x, [taps_of_group(w, "fp32") for w in ws], sc, sh, s, NONE)
    parts = []
    for g, (b, e) in enumerate(group_bounds(C, G)):
        k = 3 + 2 * g
        parts.append(F.conv2d(x[..., b:e].permute(0, 3, 1, 2).double(), ws[g].double(), stride=s, padding=k // 2, groups=e - b))
    want = torch.cat(parts, dim=1) * sc[:, None, None] + sh[:, None, None]
    assert ref.shape == want.permute(0, 2, 3, 1).shape == (N, (H - 1) // s + 1, (W - 1) // s + 1, C)
    assert torch.allclose(ref, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def _embed(t, k, K, corner=False):
    """[k*k][C] taps zero-embedded into a K x K window: at the centre, or (the bug) at the top-left corner"""
    o = 0 if corner else (K - k) // 2
    out = torch.zeros((K, K, t.shape[1]), dtype=t.dtype)
    out[o:o + k, o:o + k] = t.view(k, k, -1)
    return out.view(K * K, -1)


def _ring_dropped(t, k):
    out = t.clone().view(k, k, -1)
    out[0], out[-1], out[:, 0], out[:, -1] = 0, 0, 0, 0
    return out.view(k * k, -1)


def _shift_rows(x):
    """x moved up by one row (the window reads one input row further on), zero filled"""
    return F.pad(x[:, 1:], (0, 0, 0, 0, 0, 1))


def test_zero_embedding_is_exact():
    """a k x k filter with pad k // 2 equals the K x K filter with pad K // 2 whose ring is zero - what a straddling chunk runs"""
    x, taps, sc, sh = _inputs((3, 144, 3, 2, 15, 16), "fp32")
    for s in (1, 2):
        small, _ = dw_ref(x[..., :48], taps[0], sc[:48], sh[:48], 3, s, (1,) * 4, NONE)
        for K in (5, 7, 11):
            big, _ = dw_ref(x[..., :48], _embed(taps[0], 3, K), sc[:48], sh[:48], K, s, (K // 2,) * 4, NONE)
            assert torch.equal(small, big), (s, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [RELU, SWISH])
def test_bug_models_violate_the_bound(dtype, act):
    def check(shape, bug, what):
        x, taps, sc, sh = _inputs(shape, dtype)
        s = shape[3]
        ref, err = mix_ref(x, taps, sc, sh, s, act)
        bound = out_bound(ref, err, dtype)
        got = bug(x, taps, sc, sh, s, ref)
        assert got.shape == ref.shape
        assert bool(((got - ref).abs() > bound).any()), "{} ({}, act {}) stays within the bound".format(what, dtype, act)

    w90 = (2, 360, 4, 1, 9, 11)

    def boundary_moved(x, taps, sc, sh, s, ref):               # channels 90..95 (with 88, 89: one 8-channel chunk) run as 3x3
        t = [v.clone() for v in taps]
        t[1][:, :6] = _ring_dropped(taps[1][:, :6], 5)          # (only the centre 3x3 of their 5x5 taps is applied)
        return mix_ref(x, t, sc, sh, s, act)[0]
    check(w90, boundary_moved, "group boundary moved by one chunk")

    def corner(x, taps, sc, sh, s, ref):                       # channels 88, 89 run the 5x5 class: their 3x3 filter at its corner
        out = ref.clone()
        out[..., 88:90] = dw_ref(x[..., 88:90], _embed(taps[0][:, 88:90], 3, 5, corner=True), sc[88:90], sh[88:90], 5, s, (2,) * 4,
                                 act)[0]
        return out
    check(w90, corner, "small filter embedded at the corner")

    for shape, g in ((w90, 3), ((2, 720, 5, 2, 14, 14), 4), ((2, 720, 5, 2, 9, 10), 4)):
        def ring(x, taps, sc, sh, s, ref, g=g):
            t = list(taps)
            t[g] = _ring_dropped(taps[g], 3 + 2 * g)
            return mix_ref(x, t, sc, sh, s, act)[0]
        check(shape, ring, "outer ring of the {0}x{0} filter dropped".format(3 + 2 * g))

    for shape in (w90, (2, 240, 2, 1, 12, 7), (2, 240, 4, 2, 5, 5)):
        for g in range(1, shape[2]):
            def neighbour(x, taps, sc, sh, s, ref, g=g):       # equal group widths: channel c of group g gets channel c of group g - 1
                t = list(taps)
                t[g] = _embed(taps[g - 1], 1 + 2 * g, 3 + 2 * g)
                return mix_ref(x, t, sc, sh, s, act)[0]
            check(shape, neighbour, "group {}'s taps read at group {}'s offset".format(g, g - 1))

    def strip(x, taps, sc, sh, s, ref):                        # strips of 4 rows: each strip's first row repeats the row before it
        dup = ref.clone()
        dup[:, 4::4] = ref[:, 3:ref.shape[1] - 1:4][:, :dup[:, 4::4].shape[1]]
        return dup
    check((2, 48, 3, 1, 40, 3), strip, "row duplicated across a strip boundary")

    def phase(x, taps, sc, sh, s, ref):
        return mix_ref(_shift_rows(x), taps, sc, sh, s, act)[0]
    check((3, 144, 3, 2, 15, 16), phase, "stride-2 phase off by one on an odd map")
    check((2, 720, 5, 2, 9, 10), phase, "stride-2 phase off by one on an odd map (11x11)")
