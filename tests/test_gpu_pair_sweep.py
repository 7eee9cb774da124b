"""
GPU sweep of the fused 1x1 pair kernels - csrc/pair1x1.hpp (64 -> 256 -> 64, weights in registers: PB4, PB2, GATED, IDCONV) and
csrc/wpair1x1.hpp (128 -> 512, 256 -> 1024, 128 -> 256, 256 -> 512, weights through an LDS ring, each plain and gated): twelve kernel
forms, each in bf16 and fp16 - against the float64 reference and the derived elementwise bounds of tests/pair_ref.py
(tests/test_pair_ref_bounds.py proves on the CPU that the reference equals torch's float64 composition, that an emulated fp32 kernel stays
inside the bounds on every case below and that the listed kernel bugs leave them).

The sweep drives the C ABI directly: its own pcv_conv_desc per convolution, pcv_conv_pack, then pcv_conv1x1_pair_fused / _gated_fused /
_idconv_fused. That reaches what the engine never sets: all seven activation codes at all three sites (act1, post1, act2). The first
assertion of every test is the library's routing restated (`route`: pair_unsupported, pcv_conv1x1_pair_gated_supported,
pair_idconv_unsupported and the form pair_impl launches - pair_pb, gate, wpair_cfg, gate_in_lds), and the library's own *_supported
answer: a routing change cannot silently move a case onto another kernel.

Every case runs on the resident grid and under max_blocks = 8 (several tiles per block: the x ring wraps, the wide kernels' tile parity
flips), into NaN-filled y1 and y2 with a guard tail of 128 pixels each: an element nobody wrote fails the comparison, a store outside
y1 / y2 fails the guard check. y1 is judged first; y2 is judged against the bound computed from the y1 just read back (tests/pair_ref.py).
The gate tensor has one more row than images, NaN-filled: a gate row index beyond the last image that reaches a stored pixel shows.
Tuples are (N, H, W); M = N H W pixels, HW pixels per image.
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
from pair_ref import NARROW_TILE, WPAIR_CONFIGS, pair_operands, wpair_layout, y1_ref_bound, y2_ref_bound
from test_gpu_dw_se import CODE, HSIGMOID, HSWISH, NONE, RELU, RELU6, SIGMOID, SWISH, TDT

pytestmark = pytest.mark.gpu

GRIDS = [0, 8]
DTYPES16 = ("bf16", "fp16")
PCV_ERR_INVALID = -1

# ---- the twelve forms --------------------------------------------------------------------------------------------------------------------
# kernel: the template arguments behind the storage type - ("pair1x1", PB, IDC, GATE) or ("wpair1x1", CM, C1, GATE)
Form = collections.namedtuple("Form", "name CM C1 gated idconv pb kernel tile gate_in_lds")


def _forms():
    out = [Form("pb4", 64, 256, False, False, 4, ("pair1x1", 4, False, False), NARROW_TILE[4], False),
           Form("pb2", 64, 256, False, False, 2, ("pair1x1", 2, False, False), NARROW_TILE[2], False),
           Form("gated", 64, 256, True, False, 2, ("pair1x1", 2, False, True), NARROW_TILE[2], False),
           Form("idconv", 64, 256, False, True, 2, ("pair1x1", 2, True, False), NARROW_TILE[2], False)]
    for cm, c1 in WPAIR_CONFIGS:
        G = wpair_layout(cm, c1)
        for gated in (False, True):
            out.append(Form("w{}x{}{}".format(cm, c1, "g" if gated else ""), cm, c1, gated, False, 2, ("wpair1x1", cm, c1, gated), G.P,
                            gated and G.GATE_LDS))
    return out


FORMS = collections.OrderedDict((f.name, f) for f in _forms())
Case = collections.namedtuple("Case", "form N H W act1 post1 act2")
RESNET = (NONE, RELU, RELU)

# ---- shapes: the smallest at which each tiling can go wrong (tests/test_pair_ref_bounds.py asserts what each one is there for) ---------------
NARROW_SHAPES = [(1, 1, 1), (1, 5, 7), (2, 4, 8), (3, 13, 11), (9, 14, 14),
                 (7, 9, 9)]        # (not asked for: 18 32-pixel tiles = three rounds with a ragged last ROUND on the capped grid; (9, 14, 14) gives 56 = 7 x 8)
GATE_GLOBAL_SHAPES = [(40, 1, 1), (5, 1, 13)]                  # every pixel another image; an image boundary inside a 16-pixel block
WIDE_SHAPES = [(1, 1, 1), (1, 5, 7), (1, 8, 16), (1, 3, 43), (3, 13, 11), (17, 12, 11)]
GATE_LDS_SHAPES = [(5, 8, 16), (5, 3, 43), (3, 13, 11), (17, 12, 11)]
HW127 = (3, 1, 127)                                           # one pixel short of a wide tile: refused where the gate rows live in LDS, swept elsewhere
EPILOGUE_SHAPE = (3, 13, 11)
# (act1, post1, act2). The first seven are the list this sweep was asked for; it leaves post1 without SIGMOID / SWISH / HSIGMOID, so three more
# rows put every one of the seven codes at every one of the three sites.
EPILOGUES = [(RELU, NONE, NONE), (RELU6, RELU6, RELU6), (NONE, NONE, HSWISH), (HSWISH, RELU, SWISH), (SWISH, HSWISH, SIGMOID),
             (SIGMOID, NONE, HSIGMOID), (HSIGMOID, RELU6, RELU),
             (NONE, SIGMOID, NONE), (RELU, SWISH, RELU6), (NONE, HSIGMOID, HSWISH)]


def shapes_of(f):
    if f.gate_in_lds:
        return list(GATE_LDS_SHAPES)
    if f.CM == 64:
        return NARROW_SHAPES + (GATE_GLOBAL_SHAPES + [HW127] if f.gated else [])
    return WIDE_SHAPES + ([s for s in NARROW_SHAPES + GATE_GLOBAL_SHAPES if s not in WIDE_SHAPES] + [HW127] if f.gated else [])


def cases_of(f):
    return [Case(f.name, *s, *RESNET) for s in shapes_of(f)] + [Case(f.name, *EPILOGUE_SHAPE, *e) for e in EPILOGUES]


def all_cases():
    """(form, case, dtype) of everything the sweep launches (tests/test_pair_ref_bounds.py walks the same list)"""
    return [(f, c, dt) for f in FORMS.values() for c in cases_of(f) for dt in DTYPES16]


def case_id(c):
    return "{}_n{}_{}x{}_a{}{}{}".format(c.form, c.N, c.H, c.W, c.act1, c.post1, c.act2)


# ---- pair_unsupported / pcv_conv1x1_pair_gated_supported / pair_idconv_unsupported / pair_impl restated (csrc/pcv_api.hip) ---------------------
Route = collections.namedtuple("Route", "ok kernel tile gate_in_lds nTiles")


def route(CM, C1, C2, N, H, W, gated=False, idconv=False, pair_pb=2, wpair=3, res1=True, res2=False, post2=NONE, y1_cpitch=0):
    M = N * H * W
    narrow = (CM, C1, C2) == (64, 256, 64)
    wide = ((CM == 128 and wpair & 1) or (CM == 256 and wpair & 2)) and (CM, C1) in WPAIR_CONFIGS and C2 == CM
    ok = bool(narrow or wide) and y1_cpitch in (0, C1) and res1 and not res2 and post2 == NONE and M * C1 * 2 < 1 << 31
    if idconv:
        ok = ok and CM == 64
    if not ok:
        return Route(False, None, 0, False, 0)
    if CM >= 128:
        G = wpair_layout(CM, C1)
        in_lds = gated and G.GATE_LDS
        if in_lds and H * W < G.P:
            return Route(False, None, 0, False, 0)
        return Route(True, ("wpair1x1", CM, C1, gated), G.P, in_lds, (M + G.P - 1) // G.P)
    pb = 2 if (gated or idconv or pair_pb != 4) else 4
    return Route(True, ("pair1x1", pb, idconv, gated), 16 * pb, False, (M + 16 * pb - 1) // (16 * pb))


def route_case(c):
    f = FORMS[c.form]
    return route(f.CM, f.C1, f.CM, c.N, c.H, c.W, f.gated, f.idconv, f.pb)


# ---- reference of y1, once per (operands, act1, post1, dtype) ----------------------------------------------------------------------------------
def seed_of(c):
    f = FORMS[c.form]
    return zlib.crc32(repr((f.CM, f.C1, f.gated, f.idconv, c.N, c.H, c.W)).encode()) & 0x3FFFFFFF


def case_operands(c, dtype):
    f = FORMS[c.form]
    return pair_operands(c.N, c.H, c.W, f.CM, f.C1, dtype, seed_of(c), gated=f.gated, idconv=f.idconv)


def case_reference(c, dtype):
    """(operands, reference of y1, bound of y1)"""
    ops = case_operands(c, dtype)
    return (ops,) + tuple(y1_ref_bound(ops, c.act1, c.post1, dtype))


@functools.lru_cache(maxsize=8)
def _cached_reference(seed, shape, act1, post1, form_key, dtype):
    f = [f for f in FORMS.values() if (f.CM, f.C1, f.gated, f.idconv) == form_key][0]
    return case_reference(Case(f.name, *shape, act1, post1, NONE), dtype)


def reference_of(c, dtype):
    f = FORMS[c.form]
    return _cached_reference(seed_of(c), (c.N, c.H, c.W), c.act1, c.post1, (f.CM, f.C1, f.gated, f.idconv), dtype)      # pb4 and pb2 share it


# ---- launching ----------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def make_desc(N, H, W, Cin, Cout, dtype, act=NONE, post=NONE, res=False, y_cpitch=0):
    from pytorchcv_amd._lib import ConvDesc
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw = N, H, W, Cin, Cout, 1, 1
    d.stride_h, d.stride_w, d.pad_t, d.pad_l, d.pad_b, d.pad_r, d.dil_h, d.dil_w = 1, 1, 0, 0, 0, 0, 1, 1
    d.groups, d.act, d.post_act, d.has_residual = 1, act, post, int(res)
    d.dtype = d.out_dtype = CODE[dtype]
    d.x_cpitch, d.x_wpitch, d.y_cpitch = Cin, W, y_cpitch
    return d


def pair_descs(c, dtype):
    """(d1, d2, d_id or None)"""
    f = FORMS[c.form]
    d1 = make_desc(c.N, c.H, c.W, f.CM, f.C1, dtype, c.act1, c.post1, res=True)
    d2 = make_desc(c.N, c.H, c.W, f.C1, f.CM, dtype, c.act2)
    return d1, d2, make_desc(c.N, c.H, c.W, f.CM, f.C1, dtype) if f.idconv else None


def _pack(d, w, dev):
    lb, L, ctx = _lib()
    n = ctypes.c_size_t(0)
    lb.check(L.pcv_conv_packed_bytes(ctypes.byref(d), ctypes.byref(n)), None)
    packed = torch.zeros(n.value + 16, dtype=torch.uint8, device=dev)
    wd = w.to(dev).contiguous()
    lb.check(L.pcv_conv_pack(ctx, ctypes.byref(d), _p(wd), _p(packed), _stream()), ctx)
    torch.cuda.synchronize()
    return packed


GUARD_PIXELS = 128


def nan_output(M, C, dtype, dev):
    """a NaN-filled buffer of M x C elements and a guard tail of one wide tile (128 pixels x C) behind it"""
    return torch.full((M * C + GUARD_PIXELS * C + 64,), float("nan"), dtype=TDT[dtype], device=dev)


class Launch(object):
    """one case on the device: packed weights, operands, and `run()` into fresh NaN-filled outputs with their guard tails"""
    def __init__(self, c, dtype, ops, dev):
        self.c, self.dtype, self.dev, self.f = c, dtype, dev, FORMS[c.form]
        self.d1, self.d2, self.di = pair_descs(c, dtype)
        t = TDT[dtype]
        self.p1, self.p2 = _pack(self.d1, ops.w1, dev), _pack(self.d2, ops.w2, dev)
        self.x = ops.x.to(dev, t).contiguous()
        self.res = ops.res.to(dev, t).contiguous() if ops.res is not None else None
        self.bn = [v.to(dev).contiguous() for v in (ops.scale1, ops.shift1, ops.scale2, ops.shift2)]
        self.gate = None
        if ops.gate is not None:             # [N + 1][C1]: the row behind the last image is NaN
            self.gate = torch.cat((ops.gate, torch.full((1, self.f.C1), float("nan")))).to(dev).contiguous()
        if self.f.idconv:
            self.pi = _pack(self.di, ops.wid, dev)
            self.x0 = ops.x0.to(dev, t).contiguous()
            self.bni = [v.to(dev).contiguous() for v in (ops.scale_id, ops.shift_id)]

    def run(self):
        """(y1 [N][H][W][C1], y2 [N][H][W][CM], guard tail of y1, guard tail of y2)"""
        lb, L, ctx = _lib()
        c, f = self.c, self.f
        M = c.N * c.H * c.W
        y1b, y2b = nan_output(M, f.C1, self.dtype, self.dev), nan_output(M, f.CM, self.dtype, self.dev)
        sc1, sh1, sc2, sh2 = [_p(v) for v in self.bn]
        d1, d2 = ctypes.byref(self.d1), ctypes.byref(self.d2)
        if f.idconv:
            rc = L.pcv_conv1x1_pair_idconv_fused(ctx, ctypes.byref(self.di), d1, d2, _p(self.x0), _p(self.pi), _p(self.bni[0]), _p(self.bni[1]),
                                                 _p(self.x), _p(self.p1), sc1, sh1, _p(y1b), _p(self.p2), sc2, sh2, _p(y2b), _stream())
        elif f.gated:
            rc = L.pcv_conv1x1_pair_gated_fused(ctx, d1, d2, _p(self.x), _p(self.p1), sc1, sh1, _p(self.gate), _p(self.res), _p(y1b),
                                                _p(self.p2), sc2, sh2, _p(y2b), _stream())
        else:
            rc = L.pcv_conv1x1_pair_fused(ctx, d1, d2, _p(self.x), _p(self.p1), sc1, sh1, _p(self.res), _p(y1b), _p(self.p2), sc2, sh2,
                                          _p(y2b), _stream())
        lb.check(rc, ctx)
        torch.cuda.synchronize()
        return (y1b[:M * f.C1].view(c.N, c.H, c.W, f.C1), y2b[:M * f.CM].view(c.N, c.H, c.W, f.CM), y1b[M * f.C1:], y2b[M * f.CM:])


_STATS = os.environ.get("PCV_PAIR_SWEEP_STATS")       # a file name: one JSON line per comparison (measurements, nothing is asserted from them)


def check(out, ref, bound, what, tile, stats=None):
    """|y - ref| <= bound elementwise (out, ref, bound: NHWC on the CPU); names pixel, channel, image and tile of the worst element"""
    err = (out.double() - ref).abs()
    ratio = err / bound
    if _STATS and stats is not None:
        with open(_STATS, "a") as f:
            f.write(json.dumps(dict(stats, case=what, ratio=float(ratio.nan_to_num(nan=1e30).max()))) + "\n")
    bad = ~(err <= bound)                         # NaN (an element nobody wrote) counts as a failure
    if bool(bad.any()):
        worst = int(torch.where(bad, ratio.nan_to_num(nan=float("inf")), torch.zeros_like(ratio)).argmax())
        n, h, w, ch = [int(v) for v in np.unravel_index(worst, tuple(ref.shape))]
        pix = (n * ref.shape[1] + h) * ref.shape[2] + w
        pytest.fail("{}: {} of {} elements out of bound ({} of them NaN); worst at pixel {} (image {}, h {}, w {}), channel {}, tile {} (pixel "
                    "{} of it) - got {:.6e}, ref {:.6e}, bound {:.3e}".format(
                        what, int(bad.sum()), bad.numel(), int(torch.isnan(out).sum()), pix, n, h, w, ch, pix // tile, pix % tile,
                        float(out.flatten()[worst]), float(ref.flatten()[worst]), float(bound.flatten()[worst])))


def sweep(c, dtype, dev, pair_pb=None):
    f = FORMS[c.form]
    ops, ref1, bound1 = reference_of(c, dtype)
    run = Launch(c, dtype, ops, dev)
    seen = None                                   # (y1, reference and bound of y2 from it, y2) of the resident grid
    for g in GRIDS:
        what = "{} {} grid {}".format(case_id(c), dtype, g)
        with util.tuning(max_blocks=g, pair_pb=pair_pb or f.pb):
            y1, y2, tail1, tail2 = run.run()
        assert bool(torch.isnan(tail1).all()), what + ": the guard tail behind y1 was written"
        assert bool(torch.isnan(tail2).all()), what + ": the guard tail behind y2 was written"
        y1, y2 = y1.float().cpu(), y2.float().cpu()
        stats = dict(form=f.name, dtype=dtype, grid=g)
        check(y1, ref1, bound1, what + " y1", f.tile, dict(stats, out="y1"))          # a NaN in y1 fails here, before y2 is judged
        if seen is None or not torch.equal(seen[0], y1):
            ref2, bound2 = y2_ref_bound(y1, ops, c.act2, dtype)
        check(y2, ref2, bound2, what + " y2", f.tile, dict(stats, out="y2"))
        # a tile's arithmetic does not depend on which block walks it (the narrow kernels reduce their K-slices in a fixed order): the
        # capped grid must reproduce the resident grid's bits
        if seen is not None:
            assert torch.equal(seen[0], y1) and torch.equal(seen[1], y2), what + ": differs from the resident grid's result"
        seen = (y1, y2)


def assert_routing(c, dtype):
    """the form this case is listed under is the one the library launches, and the library's own predicates agree"""
    lb, L, ctx = _lib()
    f = FORMS[c.form]
    R = route_case(c)
    assert R.ok and R.kernel == f.kernel and R.tile == f.tile and R.gate_in_lds == f.gate_in_lds, (c, R)
    d1, d2, di = pair_descs(c, dtype)
    assert L.pcv_conv1x1_pair_supported(ctypes.byref(d1), ctypes.byref(d2)) == 1
    if f.gated:
        assert L.pcv_conv1x1_pair_gated_supported(ctypes.byref(d1), ctypes.byref(d2)) == 1
    if f.idconv:
        assert L.pcv_conv1x1_pair_idconv_supported(ctypes.byref(di), ctypes.byref(d1), ctypes.byref(d2)) == 1
    return R


def _params(forms):
    return [pytest.param(c, dt, id=case_id(c) + "-" + dt) for f in forms for c in cases_of(f) for dt in DTYPES16]


NARROW_FORMS = [f for f in FORMS.values() if f.CM == 64]
WIDE_FORMS = [f for f in FORMS.values() if f.CM >= 128]


@pytest.mark.parametrize("c,dtype", _params(NARROW_FORMS))
def test_narrow_pair_vs_float64(c, dtype, cuda_device):
    R = assert_routing(c, dtype)
    f = FORMS[c.form]
    assert R.kernel == ("pair1x1", f.pb, f.idconv, f.gated) and R.nTiles == -(-c.N * c.H * c.W // (16 * f.pb))
    sweep(c, dtype, cuda_device)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("form", ["gated", "idconv"])
def test_gated_and_identity_forms_keep_their_32_pixel_tiles_under_pair_pb_4(form, dtype, cuda_device):
    """both are instantiated for PB = 2 only: with the pair_pb = 4 switch set the host must still count 32-pixel tiles (counting 64-pixel
    ones would leave every second tile unwritten)"""
    c = Case(form, *EPILOGUE_SHAPE, *RESNET)
    f = FORMS[form]
    R = route(f.CM, f.C1, f.CM, c.N, c.H, c.W, f.gated, f.idconv, pair_pb=4)
    assert R.ok and R.kernel == f.kernel and R.tile == 32 and R.nTiles == -(-c.N * c.H * c.W // 32)
    sweep(c, dtype, cuda_device, pair_pb=4)


@pytest.mark.parametrize("c,dtype", _params(WIDE_FORMS))
def test_wide_pair_vs_float64(c, dtype, cuda_device):
    R = assert_routing(c, dtype)
    f = FORMS[c.form]
    G = wpair_layout(f.CM, f.C1)
    assert R.kernel == ("wpair1x1", f.CM, f.C1, f.gated) and R.tile == G.P == 128 and R.gate_in_lds == (f.gated and f.CM == 128)
    assert not R.gate_in_lds or c.H * c.W >= G.P                 # the staged gate rows hold two images: a tile may not touch a third
    sweep(c, dtype, cuda_device)


# ---- refusals: PCV_ERR_INVALID, nothing launched (both outputs keep their NaNs) ----------------------------------------------------------------------
def _refused(dev, dtype, CM, C1, shape, gated=False, idconv=False, id_cm=None, mutate=None, tune=None, expect_route=None):
    lb, L, ctx = _lib()
    N, H, W = shape
    M = N * H * W
    d1 = make_desc(N, H, W, CM, C1, dtype, NONE, RELU, res=True)
    d2 = make_desc(N, H, W, C1, CM, dtype, RELU)
    di = make_desc(N, H, W, id_cm or CM, C1, dtype)
    if mutate:
        mutate(d1, d2)
    t = TDT[dtype]

    def z(*s):
        return torch.zeros(s, dtype=t, device=dev)

    def f32(n):
        return torch.ones(n, dtype=torch.float32, device=dev)
    x, x0, res = z(M, CM), z(M, id_cm or CM), z(M, C1)
    packed = [torch.zeros(C1 * CM * 2 + 4096, dtype=torch.uint8, device=dev) for _ in range(3)]
    gate = f32((N + 1) * C1)
    y1, y2 = nan_output(M, C1, dtype, dev), nan_output(M, CM, dtype, dev)
    a1, a2, ai = ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(di)
    with util.tuning(**(tune or {})):
        if idconv:
            sup = L.pcv_conv1x1_pair_idconv_supported(ai, a1, a2)
            rc = L.pcv_conv1x1_pair_idconv_fused(ctx, ai, a1, a2, _p(x0), _p(packed[2]), _p(f32(C1)), _p(f32(C1)), _p(x), _p(packed[0]),
                                                 _p(f32(C1)), _p(f32(C1)), _p(y1), _p(packed[1]), _p(f32(CM)), _p(f32(CM)), _p(y2), _stream())
        elif gated:
            sup = L.pcv_conv1x1_pair_gated_supported(a1, a2)
            rc = L.pcv_conv1x1_pair_gated_fused(ctx, a1, a2, _p(x), _p(packed[0]), _p(f32(C1)), _p(f32(C1)), _p(gate), _p(res), _p(y1),
                                                _p(packed[1]), _p(f32(CM)), _p(f32(CM)), _p(y2), _stream())
        else:
            sup = L.pcv_conv1x1_pair_supported(a1, a2)
            rc = L.pcv_conv1x1_pair_fused(ctx, a1, a2, _p(x), _p(packed[0]), _p(f32(C1)), _p(f32(C1)), _p(res), _p(y1), _p(packed[1]),
                                          _p(f32(CM)), _p(f32(CM)), _p(y2), _stream())
    torch.cuda.synchronize()
    assert expect_route is not None and not expect_route.ok, "the routing restated here accepts what this test expects to be refused"
    assert sup == 0 and rc == PCV_ERR_INVALID, (sup, rc)
    assert bool(torch.isnan(y1).all()) and bool(torch.isnan(y2).all()), "a refused pair wrote into its outputs"


def test_misaligned_pointers_are_refused(cuda_device):
    """every tensor is read and written in 16-byte pieces: a pointer that is not 16-byte aligned is PCV_ERR_INVALID, nothing launched"""
    lb, L, ctx = _lib()
    dev, dtype = cuda_device, "bf16"
    N, H, W = 3, 13, 11
    M = N * H * W
    for form in ("pb2", "gated", "idconv", "w128x512", "w256x512g"):
        f = FORMS[form]
        c = Case(form, N, H, W, *RESNET)
        assert route_case(c).ok
        d1, d2, di = pair_descs(c, dtype)
        buf = {k: torch.zeros(n + 64, dtype=torch.uint8, device=dev) for k, n in
               (("x", M * f.CM * 2), ("x0", M * f.CM * 2), ("res", M * f.C1 * 2), ("p1", f.C1 * f.CM * 2 + 4096), ("p2", f.C1 * f.CM * 2 + 4096),
                ("pi", f.C1 * f.CM * 2 + 4096), ("gate", (N + 1) * f.C1 * 4))}
        bn = torch.ones(f.C1, dtype=torch.float32, device=dev)
        names = ["x", "p1", "p2"] + (["x0", "pi"] if f.idconv else ["res"]) + (["gate"] if f.gated else []) + ["y1", "y2"]
        for bad in names:
            y1, y2 = nan_output(M, f.C1, dtype, dev), nan_output(M, f.CM, dtype, dev)
            ptr = {k: v.data_ptr() for k, v in buf.items()}
            ptr.update(y1=y1.data_ptr(), y2=y2.data_ptr())
            assert all(v % 16 == 0 for v in ptr.values())
            ptr[bad] += 4 if bad == "gate" else 2                 # element-aligned, not 16-byte aligned
            a = {k: ctypes.c_void_p(v) for k, v in ptr.items()}
            b1, b2 = ctypes.byref(d1), ctypes.byref(d2)
            if f.idconv:
                rc = L.pcv_conv1x1_pair_idconv_fused(ctx, ctypes.byref(di), b1, b2, a["x0"], a["pi"], _p(bn), _p(bn), a["x"], a["p1"], _p(bn),
                                                     _p(bn), a["y1"], a["p2"], _p(bn), _p(bn), a["y2"], _stream())
            elif f.gated:
                rc = L.pcv_conv1x1_pair_gated_fused(ctx, b1, b2, a["x"], a["p1"], _p(bn), _p(bn), a["gate"], a["res"], a["y1"], a["p2"], _p(bn),
                                                    _p(bn), a["y2"], _stream())
            else:
                rc = L.pcv_conv1x1_pair_fused(ctx, b1, b2, a["x"], a["p1"], _p(bn), _p(bn), a["res"], a["y1"], a["p2"], _p(bn), _p(bn), a["y2"],
                                              _stream())
            torch.cuda.synchronize()
            assert rc == PCV_ERR_INVALID, (form, bad, rc)
            assert bool(torch.isnan(y1).all()) and bool(torch.isnan(y2).all()), (form, bad)


@pytest.mark.parametrize("dtype", DTYPES16)
def test_unsupported_pairs_are_refused(dtype, cuda_device):
    dev = cuda_device
    N, H, W = HW127
    assert H * W == wpair_layout(128, 512).P - 1
    for cm, c1 in ((128, 512), (128, 256)):               # the gate rows of two images in LDS: a 127-pixel map could put three into a tile
        _refused(dev, dtype, cm, c1, HW127, gated=True, expect_route=route(cm, c1, cm, N, H, W, gated=True))
        assert route(cm, c1, cm, N, H, W).ok               # ... while the ungated form of the same shape is fine
    for cm, c1 in ((128, 512), (256, 1024), (128, 256), (256, 512)):
        _refused(dev, dtype, cm, c1, (3, 13, 11), tune=dict(wpair=0), expect_route=route(cm, c1, cm, 3, 13, 11, wpair=0))
    for cm, c1 in ((64, 256), (128, 512), (256, 512)):
        def res2(d1, d2):
            d2.has_residual = 1

        def nores1(d1, d2):
            d1.has_residual = 0

        def pitch(d1, d2):
            d1.y_cpitch = d1.Cout + 64
        _refused(dev, dtype, cm, c1, (3, 13, 11), mutate=res2, expect_route=route(cm, c1, cm, 3, 13, 11, res2=True))
        _refused(dev, dtype, cm, c1, (3, 13, 11), mutate=nores1, expect_route=route(cm, c1, cm, 3, 13, 11, res1=False))
        _refused(dev, dtype, cm, c1, (3, 13, 11), mutate=pitch, expect_route=route(cm, c1, cm, 3, 13, 11, y1_cpitch=c1 + 64))
    _refused(dev, dtype, 128, 512, (3, 13, 11), idconv=True, expect_route=route(128, 512, 128, 3, 13, 11, idconv=True))
    # y1 must fit the 2 GiB window its 32-bit byte offsets cover: the predicate alone (nothing is allocated or launched)
    lb, L, ctx = _lib()
    for cm, c1 in ((64, 256), (128, 512), (256, 1024), (128, 256), (256, 512)):
        rows = (1 << 31) // (2 * c1)                       # N = rows, H = W = 1: y1 takes exactly 2 GiB
        for n, ok in ((rows, False), (rows - 1, True)):
            d1, d2 = make_desc(n, 1, 1, cm, c1, dtype, NONE, RELU, res=True), make_desc(n, 1, 1, c1, cm, dtype, RELU)
            assert route(cm, c1, cm, n, 1, 1).ok == ok
            assert L.pcv_conv1x1_pair_supported(ctypes.byref(d1), ctypes.byref(d2)) == int(ok), (cm, c1, n)
