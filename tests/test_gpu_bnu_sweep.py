"""
GPU sweep of the fused stage-1 bottleneck unit - csrc/bnu.hpp, plain form (256 -> 64 -> 64 -> 256, skip = x) and identity-convolution
form (64 -> 64 -> 64 -> 256, skip = BN(conv_id(x))), each in bf16 and fp16 - against the float64 reference of tests/bnu_ref.py: the exact
family bit for bit, the bounded family inside the derived elementwise bound (tests/test_bnu_ref_bounds.py proves on the CPU that the
reference equals torch's float64 composition, that an emulated fp32 kernel passes both and that the listed kernel bugs do not).

The sweep drives the C ABI directly: its own pcv_conv_desc per convolution, pcv_conv_pack, then pcv_bottleneck_fused. The first assertion
of every test is the library's routing restated (`route`: bottleneck_unsupported and the item split of pcv_bottleneck_fused) next to the
library's own pcv_bottleneck_supported answer.

Shapes are (N, H) at W = 56: single-row images, the first wrap of the 4-slot rings (H = 3: steps -1 .. 4) and several wraps (H = 9),
image boundaries inside one block (N > 1 under the capped grid). Every case runs on the resident grid and under max_blocks = 2, as whole
images, with the automatic split, and with bands of 1, 4 and a ragged last band - into a NaN-filled y with a guard tail of 128 pixels: an
element nobody wrote fails the comparison, a store outside y fails the guard check. The value of an output element may not depend on the
split or the grid: every run of a case must reproduce the first one's bits.
"""

import collections
import contextlib
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from bnu_ref import CM, CO, NONE, RELU, RELU6, RESNET, W, Unit, bounded_operands, certified, cin_of, exact_operands, exact_result, unit_ref
from test_gpu_dw_se import CODE, TDT

pytestmark = pytest.mark.gpu

GRIDS = [0, 2]
DTYPES16 = ("bf16", "fp16")
PCV_ERR_INVALID = -1
SHAPES = [(1, 1), (1, 2), (1, 3), (1, 5), (1, 9), (3, 4), (2, 7), (5, 3)]
EPILOGUE_SHAPE = (2, 7)
# (act1, act2, act3, post): the clamp codes are all the epilogue helper (conv_device.hpp: make_epi_bounds / epi2) takes
EPILOGUES = [(RELU6, RELU6, RELU6, RELU6), (NONE, NONE, NONE, NONE), (RELU, RELU6, RELU, NONE)]


def cases():
    out = []
    for idconv in (False, True):
        out += [Unit(n, h, idconv, *RESNET) for n, h in SHAPES]
        out += [Unit(*EPILOGUE_SHAPE, idconv, *e) for e in EPILOGUES]
    return out


def case_id(u):
    return "{}_n{}_h{}_a{}{}{}{}".format("idc" if u.idconv else "plain", u.N, u.H, u.act1, u.act2, u.act3, u.post)


def bands_of(H):
    """band settings of one case: whole images (H), the automatic split (0), 1, 4 and sizes that leave a ragged last band"""
    out = [H, 0, 1, min(4, H)] + [b for b in (2, 3, 4, 5) if b < H and H % b != 0]
    return sorted(set(out), key=out.index)


# ---- bottleneck_unsupported and the item split of pcv_bottleneck_fused restated (csrc/pcv_api.hip) ------------------------------------------
Route = collections.namedtuple("Route", "ok form band nBands nItems grid")


def route(N, H, Wd, cin, cm, cm2, cout, dtype, acts, idconv, bnu_band=0, max_blocks=0, num_cu=256, bnu=-1, res3=True):
    ok = (bnu != 0 and dtype in DTYPES16 and Wd == 56 and N >= 1 and H >= 1 and (cin, cm, cm2, cout) == (64 if idconv else 256, 64, 64, 256) and
          res3 and all(0 <= a <= RELU6 for a in acts) and N * H * Wd * cout * 2 < 1 << 31)
    if not ok:
        return Route(False, None, 0, 0, 0, 0)
    band = H
    if bnu_band > 0:
        band = min(bnu_band, H)
    elif N < num_cu:
        nb = max(1, min((H + 3) // 4, (num_cu + N - 1) // N))
        band = (H + nb - 1) // nb
    nBands = (H + band - 1) // band
    items = N * nBands
    return Route(True, "idc" if idconv else "plain", band, nBands, items, min(items, max_blocks if max_blocks > 0 else num_cu))


# ---- launching ----------------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {"max_blocks": 0, "bnu_band": 0, "bnu": -1}


def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


@contextlib.contextmanager
def tuning(**switches):
    lb, L, ctx = _lib()
    try:
        for k, v in switches.items():
            lb.check(L.pcv_set_tuning(ctx, k.encode(), int(v)), ctx)
        yield
    finally:
        for k in switches:
            lb.check(L.pcv_set_tuning(ctx, k.encode(), _DEFAULTS[k]), ctx)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def make_desc(N, H, Wd, Cin, Cout, dtype, k=1, act=NONE, post=NONE, res=False):
    from pytorchcv_amd._lib import ConvDesc
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw = N, H, Wd, Cin, Cout, k, k
    p = k // 2
    d.stride_h, d.stride_w, d.pad_t, d.pad_l, d.pad_b, d.pad_r, d.dil_h, d.dil_w = 1, 1, p, p, p, p, 1, 1
    d.groups, d.act, d.post_act, d.has_residual = 1, act, post, int(res)
    d.dtype = d.out_dtype = CODE[dtype]
    d.x_cpitch, d.x_wpitch, d.y_cpitch = Cin, Wd, 0
    return d


def unit_descs(u, dtype, Wd=W):
    """(d1, d2, d3, d_id or None)"""
    ci = cin_of(u)
    return (make_desc(u.N, u.H, Wd, ci, CM, dtype, 1, u.act1), make_desc(u.N, u.H, Wd, CM, CM, dtype, 3, u.act2),
            make_desc(u.N, u.H, Wd, CM, CO, dtype, 1, u.act3, u.post, res=True), make_desc(u.N, u.H, Wd, ci, CO, dtype) if u.idconv else None)


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


class Launch(object):
    """one case on the device: packed weights, operands, and `run()` into a fresh NaN-filled output with its guard tail"""
    def __init__(self, u, dtype, ops, dev):
        self.u, self.dtype, self.dev = u, dtype, dev
        self.d = unit_descs(u, dtype)
        t = TDT[dtype]
        self.x = ops.x.to(dev, t).contiguous()
        self.p = [_pack(self.d[0], ops.w1, dev), _pack(self.d[1], ops.w2, dev), _pack(self.d[2], ops.w3, dev)]
        self.bn = [v.to(dev).contiguous() for v in (ops.scale1, ops.shift1, ops.scale2, ops.shift2, ops.scale3, ops.shift3)]
        self.pi, self.bni = None, [None, None]
        if u.idconv:
            self.pi = _pack(self.d[3], ops.wid, dev)
            self.bni = [v.to(dev).contiguous() for v in (ops.scale_id, ops.shift_id)]

    def run(self):
        """(y [N][H][56][256], guard tail)"""
        lb, L, ctx = _lib()
        u = self.u
        M = u.N * u.H * W
        yb = torch.full((M * CO + GUARD_PIXELS * CO + 64,), float("nan"), dtype=TDT[self.dtype], device=self.dev)
        d1, d2, d3, di = self.d
        b = [_p(v) for v in self.bn]
        rc = L.pcv_bottleneck_fused(ctx, ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3), ctypes.byref(di) if di is not None else None,
                                    _p(self.x), _p(self.p[0]), b[0], b[1], _p(self.p[1]), b[2], b[3], _p(self.p[2]), b[4], b[5],
                                    _p(self.pi), _p(self.bni[0]), _p(self.bni[1]), _p(yb), _stream())
        lb.check(rc, ctx)
        torch.cuda.synchronize()
        return yb[:M * CO].view(u.N, u.H, W, CO), yb[M * CO:]


def seed_of(u, family):
    return zlib.crc32(repr((family, u.idconv, u.N, u.H)).encode()) & 0x3FFFFFFF


@functools.lru_cache(maxsize=4)
def exact_reference(u, dtype):
    ops = exact_operands(u, seed_of(u, "exact"))
    return ops, exact_result(u, ops, dtype).float()


@functools.lru_cache(maxsize=4)
def bounded_reference(u, dtype):
    ops = bounded_operands(u, dtype, seed_of(u, "bounded"))
    y, bound = unit_ref(u, ops, dtype)[:2]
    return ops, y, bound


def describe_worst(out, ref, bad, ratio, u):
    worst = int(torch.where(bad, ratio.nan_to_num(nan=float("inf")), torch.zeros_like(ratio)).argmax())
    n, h, w, ch = [int(v) for v in np.unravel_index(worst, tuple(ref.shape))]
    return "{} of {} elements differ ({} of them NaN); worst at image {}, row {}, column {}, channel {} - got {:.6e}, ref {:.6e}".format(
        int(bad.sum()), bad.numel(), int(torch.isnan(out).sum()), n, h, w, ch, float(out.flatten()[worst]), float(ref.flatten()[worst]))


def assert_routing(u, dtype, num_cu):
    lb, L, ctx = _lib()
    acts = (u.act1, u.act2, u.act3, u.post)
    R = route(u.N, u.H, W, cin_of(u), CM, CM, CO, dtype, acts, u.idconv, num_cu=num_cu)
    assert R.ok and R.form == ("idc" if u.idconv else "plain") and R.nItems == u.N * R.nBands and R.band * R.nBands >= u.H, (u, R)
    d1, d2, d3, di = unit_descs(u, dtype)
    assert L.pcv_bottleneck_supported(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3), ctypes.byref(di) if di is not None else None) == 1
    return R


def sweep(u, dtype, dev, ops, judge):
    """every band split on both grids; `judge(y, what)` compares the first run with the reference, every later run must repeat its bits"""
    run = Launch(u, dtype, ops, dev)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    first = None
    for band in bands_of(u.H):
        for g in GRIDS:
            what = "{} {} band {} grid {}".format(case_id(u), dtype, band, g)
            R = route(u.N, u.H, W, cin_of(u), CM, CM, CO, dtype, (u.act1, u.act2, u.act3, u.post), u.idconv, band, g, num_cu)
            assert R.ok and (band == 0 or R.band == band) and R.grid >= 1
            with tuning(max_blocks=g, bnu_band=band):
                y, tail = run.run()
            assert bool(torch.isnan(tail).all()), what + ": the guard tail behind y was written"
            y = y.float().cpu()
            if first is None:
                judge(y, what)
                first = y
            else:
                assert torch.equal(first, y), what + ": differs from the first run's result (whole images, resident grid)"


def _params():
    return [pytest.param(u, dt, id=case_id(u) + "-" + dt) for u in cases() for dt in DTYPES16]


@pytest.mark.parametrize("u,dtype", _params())
def test_exact_family_bit_for_bit(u, dtype, cuda_device):
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert_routing(u, dtype, num_cu)
    ops, ref = exact_reference(u, dtype)
    ok, worst = certified(u, ops, dtype)
    assert ok, "the exact family's certificate fails for this case: {:.3e} >= 2^24".format(worst)

    def judge(y, what):
        bad = ~(y == ref)
        if bool(bad.any()):
            pytest.fail(what + ": " + describe_worst(y, ref, bad, (y - ref).abs(), u))
    sweep(u, dtype, cuda_device, ops, judge)


@pytest.mark.parametrize("u,dtype", _params())
def test_bounded_family_inside_the_bound(u, dtype, cuda_device):
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert_routing(u, dtype, num_cu)
    ops, ref, bound = bounded_reference(u, dtype)

    def judge(y, what):
        err = (y.double() - ref).abs()
        bad = ~(err <= bound)                         # NaN (an element nobody wrote) counts as a failure
        if bool(bad.any()):
            pytest.fail(what + ": out of bound: " + describe_worst(y, ref, bad, err / bound, u))
    sweep(u, dtype, cuda_device, ops, judge)


# ---- refusals: PCV_ERR_INVALID, nothing launched (the output keeps its NaNs) ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES16)
def test_unsupported_units_are_refused(dtype, cuda_device):
    lb, L, ctx = _lib()
    dev = cuda_device
    t = TDT[dtype]
    N, H = 2, 3

    def attempt(Wd=W, cin=256, cm=CM, acts=RESNET, idconv=False, tune=None, res3=True, expect=None):
        u = Unit(N, H, idconv, *acts)
        ci = 64 if idconv else cin
        d1 = make_desc(N, H, Wd, ci, cm, dtype, 1, u.act1)
        d2 = make_desc(N, H, Wd, cm, cm, dtype, 3, u.act2)
        d3 = make_desc(N, H, Wd, cm, CO, dtype, 1, u.act3, u.post, res=res3)
        di = make_desc(N, H, Wd, ci, CO, dtype) if idconv else None
        M = N * H * Wd
        x = torch.zeros(M * ci, dtype=t, device=dev)
        y = torch.full((M * CO + 64,), float("nan"), dtype=t, device=dev)
        packed = [torch.zeros(64 * 9 * 256 * 2 + 8192, dtype=torch.uint8, device=dev) for _ in range(4)]
        bn = torch.ones(CO, dtype=torch.float32, device=dev)
        a = [ctypes.byref(d) for d in (d1, d2, d3)] + [ctypes.byref(di) if di is not None else None]
        with tuning(**(tune or {})):
            sup = L.pcv_bottleneck_supported(*a)
            rc = L.pcv_bottleneck_fused(ctx, *a, _p(x), _p(packed[0]), _p(bn), _p(bn), _p(packed[1]), _p(bn), _p(bn), _p(packed[2]), _p(bn),
                                        _p(bn), _p(packed[3]) if idconv else None, _p(bn) if idconv else None, _p(bn) if idconv else None,
                                        _p(y), _stream())
        torch.cuda.synchronize()
        assert expect is not None and not expect.ok, "the routing restated here accepts what this test expects to be refused"
        assert sup == 0 and rc == PCV_ERR_INVALID, (sup, rc)
        assert bool(torch.isnan(y).all()), "a refused unit wrote into its output"

    def r(**kw):
        args = dict(N=N, H=H, Wd=W, cin=256, cm=CM, cm2=CM, cout=CO, dtype=dtype, acts=RESNET, idconv=False)
        args.update(kw)
        return route(**args)
    attempt(Wd=28, expect=r(Wd=28))
    attempt(cin=128, expect=r(cin=128))
    attempt(cm=128, expect=r(cm=128, cm2=128))
    attempt(acts=(4, RELU, NONE, RELU), expect=r(acts=(4, RELU, NONE, RELU)))
    attempt(res3=False, expect=r(res3=False))
    attempt(tune=dict(bnu=0), expect=r(bnu=0))
    attempt(idconv=True, tune=dict(bnu=0), expect=r(idconv=True, bnu=0))
    # y must fit the 2 GiB window its 32-bit byte offsets cover: the predicate alone (nothing is allocated or launched)
    rows = (1 << 31) // (2 * CO * W)
    for n, ok in ((rows + 1, False), (rows - 1, True)):
        u = Unit(n, 1, False, *RESNET)
        d1, d2, d3, _ = unit_descs(u, dtype)
        assert route(n, 1, W, 256, CM, CM, CO, dtype, RESNET, False).ok == ok
        assert L.pcv_bottleneck_supported(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3), None) == int(ok)
