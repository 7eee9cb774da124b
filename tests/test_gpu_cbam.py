"""
GPU tests of CBAM (CBAM-ResNet): the four C-ABI entry points, each alone, against the float64 restatement of tests/cbam_ref.py; the
reference block goldens of tests/golden/blocks_cbam.npz (+ blocks_cbam_wide.npz) with both stored gates; the two fixture nets end
to end; batch-position invariance, graph capture and run-to-run determinism.

Bounds (those of tests/test_gpu_splat.py, written here on purpose):
  kernels, fp32   : |y - exact| <= 1e-5 * cond, cond being the same sums over absolute values (relative to the sum's conditioning,
                    not to |y|). A maximum of fp32 values is exact. Behind a sigmoid (slope <= 1/4) the bound is 1e-5 * (cond / 4 + 1):
                    the + 1 is the sigmoid's own evaluation (v_exp_f32 and v_rcp_f32, 1 ulp each, on a result <= 1).
  kernels, 16 bit : one rounding of the exact result, |y - exact| <= 2^-8 (bf16) / 2^-11 (fp16) * |exact| + the fp32 term above
  blocks          : fp32 <= 1e-3 of the golden; 16 bit the golden bounds of tests/test_gpu_blocks.py (x3 for units); the gates,
                    fp32 in every mode but computed from 16-bit activations, within the same bounds
  nets            : fp32 <= 1e-3 of the reference's golden logits; default mode <= 1e-2, top-1 identical, no fp16 overflow
"""

import os
import ctypes
import pytest
import numpy as np
import torch
import util
import cbam_ref
from test_cbam_host import blocks_meta, build_cbam_block

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
ULP = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
FLOOR = {"fp32": 1e-30, "bf16": 1e-30, "fp16": 2.0 ** -25}        # half of fp16's subnormal spacing: tiny results round absolutely

# (N, C, H, W): the block fixtures' shapes - 8 lanes per pixel (sub-wave), the whole map one tile of the apply kernel; C not a power
# of two, H != W, every pixel a border pixel, N = 3; 256 chunks per pixel (more than a wave), HW = 49, a row split into two column
# tiles; interior and border pixels on an odd map, two rows per tile and a ragged last tile - plus the smallest legal map and a
# wide flat one (three 40-pixel rows in one tile)
SHAPES = [(2, 64, 9, 9), (3, 72, 5, 11), (2, 2048, 7, 7), (2, 256, 15, 15), (2, 8, 1, 1), (2, 64, 3, 40)]
IDS = ["n{}c{}_{}x{}".format(*s) for s in SHAPES]


def _representable(shape, seed, scale=1.0):
    """Values exactly representable in bf16 AND fp16 (bf16 rounding, magnitudes well inside fp16's range)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(torch.float16).float()


def _weights(C, seed):
    """(w1, b1, w2, b2, w7, scale, shift) of a CBAM block on C channels (reduction 16, at least one hidden unit)."""
    g = torch.Generator().manual_seed(seed)
    M = max(C // 16, 1) if C != 8 else 3
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    return (r(M, C) * (2.0 / C ** 0.5), r(M) * 0.1, r(C, M) * (1.0 / M ** 0.5), r(C) * 0.1, r(2, 7, 7) * 0.3,
            torch.tensor([1.3]), torch.tensor([-0.2]))


_cases = {}


def _case(shape):
    """Inputs and the float64 chain of one shape, computed once and shared (nobody writes into it). Each stage's input is the
    previous stage's exact result rounded to fp32 - what the kernel under test is handed."""
    if shape not in _cases:
        N, C, H, W = shape
        seed = 1000 * C + 10 * H + W
        x = _representable((N, H, W, C), seed)
        res = _representable((N, H, W, C), seed + 1)
        w = _weights(C, seed + 2)
        s, cond_s = cbam_ref.pool(x)
        s32 = s.float()
        gate, mid, cond_g = cbam_ref.excite(s32, *w[:4])
        g32 = gate.float()
        p, cond_p = cbam_ref.spatial_pool(x, g32)
        p32 = p.float()
        _cases[shape] = dict(x=x, res=res, w=w, s=s, cond_s=cond_s, s32=s32, gate=gate, mid=mid, cond_g=cond_g, g32=g32, p=p,
                             cond_p=cond_p, p32=p32)
    return _cases[shape]


def _lib_ctx():
    from pytorchcv_amd import _lib
    return _lib, _lib.lib(), _lib.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _worst(err, bound):
    i = int((err - bound).argmax())
    return "{} elements out of bound; worst |d| {:.3e} against {:.3e}".format(int((err > bound).sum()), float(err.flatten()[i]),
                                                                              float(bound.flatten()[i]))


def _run_pool(x, dtype, dev):
    _lib, L, ctx = _lib_ctx()
    N, H, W, C = x.shape
    xd = x.to(dev, TDT[dtype]).contiguous()
    s = torch.full((N, 2, C), 7.0, dtype=torch.float32, device=dev)
    _lib.check(L.pcv_cbam_pool(ctx, _p(xd), _p(s), N, H * W, C, CODE[dtype], _stream()), ctx)
    torch.cuda.synchronize()
    return s, xd


def _run_spatial_pool(x, gate, dtype, dev):
    _lib, L, ctx = _lib_ctx()
    N, H, W, C = x.shape
    xd, gd = x.to(dev, TDT[dtype]).contiguous(), gate.to(dev).contiguous()
    p = torch.full((N, H, W, 2), 7.0, dtype=torch.float32, device=dev)
    _lib.check(L.pcv_cbam_spatial_pool(ctx, _p(xd), _p(gd), _p(p), N, H * W, C, CODE[dtype], _stream()), ctx)
    torch.cuda.synchronize()
    return p


def _run_apply(x, gate, p, w7, scale, shift, res, relu, dtype, dev):
    _lib, L, ctx = _lib_ctx()
    N, H, W, C = x.shape
    xd = x.to(dev, TDT[dtype]).contiguous()
    rd = res.to(dev, TDT[dtype]).contiguous() if res is not None else None
    t = [v.to(dev).contiguous() for v in (gate, p, w7, scale, shift)]
    y = torch.full_like(xd, 7.0)
    _lib.check(L.pcv_cbam_apply(ctx, _p(xd), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), _p(rd), _p(y), N, H, W, C,
                                1 if relu else 0, CODE[dtype], _stream()), ctx)
    torch.cuda.synchronize()
    return y


# ---- each kernel alone against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pool_vs_float64(shape, dtype, cuda_device):
    _lib, L, ctx = _lib_ctx()
    c = _case(shape)
    s, xd = _run_pool(c["x"], dtype, cuda_device)
    out = s.double().cpu()
    err = (out[:, 0] - c["s"][:, 0]).abs()
    bound = 1e-5 * c["cond_s"] + 1e-30
    assert bool((err <= bound).all()), "mean: " + _worst(err, bound)
    assert torch.equal(out[:, 1], c["s"][:, 1]), "the maximum of representable values is exact"
    # the mean row has pcv_se_squeeze's bits (same operations in the same order)
    N, C, H, W = shape
    m = torch.empty((N, C), dtype=torch.float32, device=cuda_device)
    _lib.check(L.pcv_se_squeeze(ctx, _p(xd), _p(m), N, H * W, C, CODE[dtype], _stream()), ctx)
    torch.cuda.synchronize()
    assert torch.equal(m, s[:, 0])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_excite_vs_float64(shape, cuda_device):
    _lib, L, ctx = _lib_ctx()
    c = _case(shape)
    N, C, H, W = shape
    w1, b1, w2, b2 = (t.to(cuda_device).contiguous() for t in c["w"][:4])
    M = w1.shape[0]
    s = c["s32"].to(cuda_device).contiguous()
    mid = torch.full((N, 2, M), 7.0, dtype=torch.float32, device=cuda_device)
    gate = torch.full((N, C), 7.0, dtype=torch.float32, device=cuda_device)
    _lib.check(L.pcv_cbam_excite(ctx, _p(s), _p(w1), _p(b1), _p(w2), _p(b2), _p(mid), _p(gate), N, C, M, _stream()), ctx)
    torch.cuda.synchronize()
    cond_mid = c["s32"].double().abs() @ c["w"][0].double().abs().t() + c["w"][1].double().abs()
    err = (mid.double().cpu() - c["mid"]).abs()
    assert bool((err <= 1e-5 * cond_mid + 1e-30).all()), "hidden layer: " + _worst(err, 1e-5 * cond_mid)
    err = (gate.double().cpu() - c["gate"]).abs()
    bound = 1e-5 * (0.25 * c["cond_g"] + 1.0)
    assert bool((err <= bound).all()), "gate: " + _worst(err, bound)
    assert float(c["gate"].max() - c["gate"].min()) > 0.2, "a saturated gate would make this test blind"


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_spatial_pool_vs_float64(shape, dtype, cuda_device):
    c = _case(shape)
    p = _run_spatial_pool(c["x"], c["g32"], dtype, cuda_device).double().cpu()
    err = (p - c["p"]).abs()
    bound = 1e-5 * c["cond_p"] + 1e-30
    assert bool((err[..., 0] <= bound[..., 0]).all()), "max over channels: " + _worst(err[..., 0], bound[..., 0])
    assert bool((err[..., 1] <= bound[..., 1]).all()), "mean over channels: " + _worst(err[..., 1], bound[..., 1])


@pytest.mark.parametrize("with_res,relu", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "res", "relu", "res_relu"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_vs_float64(shape, dtype, with_res, relu, cuda_device):
    c = _case(shape)
    w7, scale, shift = c["w"][4:]
    res = c["res"] if with_res else None
    ref, sg, cond_sg, axg = cbam_ref.apply(c["x"], c["g32"], c["p32"], w7, scale, shift, res, relu)
    y = _run_apply(c["x"], c["g32"], c["p32"], w7, scale, shift, res, relu, dtype, cuda_device)
    assert y.dtype == TDT[dtype] and tuple(y.shape) == tuple(c["x"].shape)
    sg_tol = 1e-5 * (0.25 * cond_sg + 1.0)                               # the spatial gate: a sigmoid behind the 98-tap sum
    cond = axg * sg[..., None] + (res.double().abs() if with_res else 0.0)
    bound = ULP[dtype] * ref.abs() + (1e-5 * cond + axg * sg_tol[..., None]) * (1 + ULP[dtype]) + FLOOR[dtype]
    err = (y.double().cpu() - ref).abs()
    assert bool((err <= bound).all()), _worst(err, bound)
    assert float(sg.max() - sg.min()) > 0.2 or shape[2] * shape[3] == 1, "a saturated gate would make this test blind"


def test_apply_multi_round_launch_is_bit_identical(cuda_device):
    """With the grid capped at three blocks every block walks several tiles (the halo buffer is reused): same bits."""
    for dtype in ("bf16", "fp16", "fp32"):
        c = _case((2, 256, 15, 15))
        w7, scale, shift = c["w"][4:]
        y0 = _run_apply(c["x"], c["g32"], c["p32"], w7, scale, shift, c["res"], True, dtype, cuda_device)
        with util.tuning(max_blocks=3):
            y1 = _run_apply(c["x"], c["g32"], c["p32"], w7, scale, shift, c["res"], True, dtype, cuda_device)
        assert torch.equal(y0, y1), dtype


# ---- NaN ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(3, 72, 5, 11), (2, 2048, 7, 7)], ids=["n3c72_5x11", "n2c2048_7x7"])
def test_one_nan_reaches_its_own_maxima_only(shape, dtype, cuda_device):
    N, C, H, W = shape
    c = _case(shape)
    n0, h0, w0, c0 = 1, H // 2, W - 1, C - 3
    x = c["x"].clone()
    x[n0, h0, w0, c0] = float("nan")
    s_clean, _ = _run_pool(c["x"], dtype, cuda_device)
    s, _ = _run_pool(x, dtype, cuda_device)
    nan = torch.isnan(s[:, 1])
    want = torch.zeros_like(nan)
    want[n0, c0] = True
    assert torch.equal(nan, want), "max over the map: NaN at {}".format(nan.nonzero().tolist())
    assert torch.equal(torch.isnan(s[:, 0]), want)                          # (the mean of that channel is NaN as well)
    p_clean = _run_spatial_pool(c["x"], c["g32"], dtype, cuda_device)
    p = _run_spatial_pool(x, c["g32"], dtype, cuda_device)
    nan = torch.isnan(p[..., 0])
    want = torch.zeros_like(nan)
    want[n0, h0, w0] = True
    assert torch.equal(nan, want), "max over the channels: NaN at {}".format(nan.nonzero().tolist())
    assert torch.equal(torch.isnan(p[..., 1]), want)
    for n in range(N):
        if n != n0:
            assert torch.equal(s[n], s_clean[n]) and torch.equal(p[n], p_clean[n]), "image {} changed".format(n)
    assert torch.equal(p[n0][~want[n0]], p_clean[n0][~want[n0]])            # the other pixels of that image, bit for bit


# ---- fp16 range guard, refusals -------------------------------------------------------------------------------------------------
def test_fp16_range_guard_in_apply(cuda_device):
    from pytorchcv_amd import engine
    N, H, W, C = 1, 4, 4, 16
    x = torch.full((N, H, W, C), 60000.0)
    ones, p = torch.ones(N, C), torch.zeros(N, H, W, 2)
    w7, scale, shift = torch.zeros(2, 7, 7), torch.ones(1), torch.full((1,), 10.0)       # spatial gate = sigmoid(10)
    before = engine.fp16_overflow_count(cuda_device)
    y = _run_apply(x, ones, p, w7, scale, shift, x, False, "fp16", cuda_device)
    mid = engine.fp16_overflow_count(cuda_device)
    assert mid > before and bool(torch.isinf(y.float()).all())
    _run_apply(torch.ones_like(x), ones, p, w7, scale, shift, torch.ones_like(x), True, "fp16", cuda_device)
    assert engine.fp16_overflow_count(cuda_device) == mid                    # inside the range nothing is counted
    _run_apply(x, ones, p, w7, scale, shift, x, False, "bf16", cuda_device)
    assert engine.fp16_overflow_count(cuda_device) == mid                    # nor in another storage type


def test_refusals(cuda_device):
    _lib, L, ctx = _lib_ctx()
    st = _stream()
    x = torch.zeros(2 * 16 * 64, device=cuda_device)
    y = torch.zeros_like(x)
    m = torch.zeros(4096, device=cuda_device)

    def invalid(rc):
        with pytest.raises(_lib.PcvError) as e:
            _lib.check(rc, ctx)
        assert e.value.code == -1

    # pool: C % 8, C < 8, NULL, dtype, empty batch / map
    invalid(L.pcv_cbam_pool(ctx, _p(x), _p(m), 2, 16, 12, 0, st))
    invalid(L.pcv_cbam_pool(ctx, _p(x), _p(m), 2, 16, 0, 0, st))
    invalid(L.pcv_cbam_pool(ctx, None, _p(m), 2, 16, 64, 0, st))
    invalid(L.pcv_cbam_pool(ctx, _p(x), None, 2, 16, 64, 0, st))
    invalid(L.pcv_cbam_pool(ctx, _p(x), _p(m), 2, 16, 64, 7, st))
    invalid(L.pcv_cbam_pool(ctx, _p(x), _p(m), 0, 16, 64, 0, st))
    invalid(L.pcv_cbam_pool(ctx, _p(x), _p(m), 2, 0, 64, 0, st))
    # excite: C % 8, M < 1, NULL
    args = [_p(m)] * 7
    invalid(L.pcv_cbam_excite(ctx, *args, 2, 60, 4, st))
    invalid(L.pcv_cbam_excite(ctx, *args, 2, 64, 0, st))
    invalid(L.pcv_cbam_excite(ctx, *args, 0, 64, 4, st))
    for i in range(7):
        invalid(L.pcv_cbam_excite(ctx, *(args[:i] + [None] + args[i + 1:]), 2, 64, 4, st))
    # spatial pool: C % 8, NULL, dtype
    invalid(L.pcv_cbam_spatial_pool(ctx, _p(x), _p(m), _p(m), 2, 16, 20, 1, st))
    invalid(L.pcv_cbam_spatial_pool(ctx, _p(x), None, _p(m), 2, 16, 64, 1, st))
    invalid(L.pcv_cbam_spatial_pool(ctx, _p(x), _p(m), None, 2, 16, 64, 1, st))
    invalid(L.pcv_cbam_spatial_pool(ctx, _p(x), _p(m), _p(m), 2, 16, 64, 3, st))
    invalid(L.pcv_cbam_spatial_pool(ctx, _p(x), _p(m), _p(m), 2, -1, 64, 1, st))
    # apply: C % 8, NULL (every required pointer; the residual may be NULL), dtype, post_act, empty map
    ok = [_p(x), _p(m), _p(m), _p(m), _p(m), _p(m), None, _p(y)]
    invalid(L.pcv_cbam_apply(ctx, *ok, 2, 4, 4, 20, 0, 0, st))
    invalid(L.pcv_cbam_apply(ctx, *ok, 2, 4, 4, 64, 0, 3, st))
    invalid(L.pcv_cbam_apply(ctx, *ok, 2, 4, 4, 64, 99, 0, st))
    invalid(L.pcv_cbam_apply(ctx, *ok, 2, 4, 4, 64, -1, 0, st))
    invalid(L.pcv_cbam_apply(ctx, *ok, 2, 0, 4, 64, 0, 0, st))
    invalid(L.pcv_cbam_apply(ctx, *ok, 2, 4, 0, 64, 0, 0, st))
    for i in (0, 1, 2, 3, 4, 5, 7):
        invalid(L.pcv_cbam_apply(ctx, *(ok[:i] + [None] + ok[i + 1:]), 2, 4, 4, 64, 0, 0, st))
    _lib.check(L.pcv_cbam_apply(ctx, *ok, 2, 4, 4, 64, 0, 0, st), ctx)                 # and the call they all vary is accepted
    torch.cuda.synchronize()


# ---- reference block goldens ----------------------------------------------------------------------------------------------------
_npz = None


def _golden(key):
    global _npz
    if _npz is None:
        _npz = {}
        for f in ("blocks_cbam.npz", "blocks_cbam_wide.npz"):
            z = np.load(os.path.join(util.GOLDEN, f))
            _npz.update({k: z[k] for k in z.files})
    return torch.from_numpy(_npz[key])


_BLOCK_NAMES = sorted(blocks_meta())


def _run_block(name, dtype, dev):
    """(y, golden, kind, channel gate, spatial gate) - the gates for a CbamBlock case, recomputed by the two gate entry points from
    the same activation the block saw."""
    import pytorchcv_amd
    from pytorchcv_amd import engine
    m = blocks_meta()[name]
    blk = build_cbam_block(m["case"])
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)
    blk = pytorchcv_amd.set_compute_dtype(blk.to(dev), dtype)
    x = util.synth_input(*m["case"]["x"], seed=m["input_seed"]).to(dev)
    with torch.no_grad():
        y = blk(x)
    gates = (None, None)
    if m["case"]["kind"] == "CbamBlock":
        _lib, L, ctx = _lib_ctx()
        a = engine.from_nchw(x, dtype, stem=False)
        N, C, HW = a.N, a.C, a.H * a.W
        w1, b1, w2, b2 = blk.ch_gate.mlp.weights()
        w7, scale, shift = blk.sp_gate.stencil()
        f32 = dict(dtype=torch.float32, device=dev)
        s, mid, gate, p = (torch.empty(sh, **f32) for sh in ((N, 2, C), (N, 2, w1.shape[0]), (N, C), (N, HW, 2)))
        _lib.check(L.pcv_cbam_pool(ctx, _p(a.t), _p(s), N, HW, C, CODE[dtype], _stream()), ctx)
        _lib.check(L.pcv_cbam_excite(ctx, _p(s), _p(w1), _p(b1), _p(w2), _p(b2), _p(mid), _p(gate), N, C, w1.shape[0], _stream()), ctx)
        _lib.check(L.pcv_cbam_spatial_pool(ctx, _p(a.t), _p(gate), _p(p), N, HW, C, CODE[dtype], _stream()), ctx)
        # the spatial gate alone: apply on a one-channel-chunk tensor of ones with a unit channel gate gives sg itself
        one = torch.ones((N, a.H, a.W, 8), **f32)
        og = torch.ones((N, 8), **f32)
        sg = torch.empty_like(one)
        _lib.check(L.pcv_cbam_apply(ctx, _p(one), _p(og), _p(p), _p(w7), _p(scale), _p(shift), None, _p(sg), N, a.H, a.W, 8, 0, 0,
                                    _stream()), ctx)
        gates = (gate.cpu(), sg[..., 0].cpu())
    torch.cuda.synchronize()
    return y.float().cpu(), _golden(name), m["case"]["kind"], gates


@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_fp32_matches_reference_golden(name, cuda_device):
    y, g, kind, (cg, sg) = _run_block(name, "fp32", cuda_device)
    assert y.shape == g.shape
    assert float((y - g).abs().max()) <= 1e-3
    if kind == "CbamBlock":
        gc, gs = _golden(name + ".channel_gate"), _golden(name + ".spatial_gate")
        assert cg.shape == gc.shape and sg.shape == gs.shape
        assert float((cg - gc).abs().max()) <= 1e-3 and float((sg - gs).abs().max()) <= 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_16bit_matches_reference_golden(name, dtype, cuda_device):
    y, g, kind, (cg, sg) = _run_block(name, dtype, cuda_device)
    assert y.shape == g.shape
    mult = 3.0 if kind == "CbamResUnit" else 1.0
    rtol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * mult
    atol = (4e-2 if dtype == "bf16" else 1e-2) * mult
    dg = (y - g).abs()
    assert bool((dg <= atol + rtol * g.abs()).all()), "vs fp32 golden: max |d| {:.3e}".format(float(dg.max()))
    if kind == "CbamBlock":
        for got, want in ((cg, _golden(name + ".channel_gate")), (sg, _golden(name + ".spatial_gate"))):
            d = (got - want).abs()
            assert bool((d <= atol + rtol * want.abs()).all()), "gate vs golden: max |d| {:.3e}".format(float(d.max()))


# ---- whole nets -----------------------------------------------------------------------------------------------------------------
NETS = ["cbam_resnet18", "cbam_resnet50"]


def _net(name, dtype, dev, fixture=True):
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name).eval()
    if fixture:
        net.load_state_dict(util.model_state(name, net.state_dict()), strict=True)
    net = net.to(dev)
    return net if dtype is None else pytorchcv_amd.set_compute_dtype(net, dtype)


@pytest.mark.parametrize("name", NETS)
def test_net_fp32_matches_reference_golden(name, cuda_device):
    logits, ids = util.model_golden(name)
    net = _net(name, "fp32", cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    err = float((y - logits).abs().max())
    print("{} fp32: vs golden {:.3e}".format(name, err))
    assert err <= 1e-3 and torch.equal(y.argmax(1), logits.argmax(1))


@pytest.mark.parametrize("name", NETS)
def test_net_default_mode_within_north_star_bound(name, cuda_device, monkeypatch):
    from pytorchcv_amd import engine
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    logits, ids = util.model_golden(name)
    net = _net(name, None, cuda_device)
    before = engine.fp16_overflow_count(cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device))
    torch.cuda.synchronize()
    assert engine.fp16_overflow_count(cuda_device) == before
    y = y.cpu()
    err = float((y - logits).abs().max())
    print("{} default ({}): vs golden {:.3e}".format(name, engine.compute_dtype_of(net), err))
    assert bool(torch.isfinite(y).all()) and torch.equal(y.argmax(1), logits.argmax(1))
    assert err <= 1e-2


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", NETS)
def test_net_16bit_distance_is_reported(name, dtype, cuda_device):
    """Both 16-bit modes of both fixture nets: finite logits, the reference's top-1; the distance is printed (DESIGN.md's table)."""
    logits, ids = util.model_golden(name)
    net = _net(name, dtype, cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    print("{} {}: vs golden {:.3e}".format(name, dtype, float((y - logits).abs().max())))
    assert bool(torch.isfinite(y).all()) and torch.equal(y.argmax(1), logits.argmax(1))


@pytest.mark.parametrize("name", NETS)
def test_batch_position_invariance(name, cuda_device, monkeypatch):
    """net(x)[1] == net(x[1:2]) bit for bit at N = 3, in the default mode."""
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    _, ids = util.model_golden(name)
    net = _net(name, None, cuda_device)
    x = util.images(ids[:3]).to(cuda_device)
    with torch.no_grad():
        y3 = net(x).clone()
        y1 = net(x[1:2].contiguous()).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y3).all())
    assert torch.equal(y3[1:2], y1)


@pytest.mark.parametrize("name", ["cbam_resnet34", "cbam_resnet101", "cbam_resnet152"])
def test_other_depths_run(name, cuda_device, monkeypatch):
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    torch.manual_seed(0)
    net = _net(name, None, cuda_device, fixture=False)
    with torch.no_grad():
        y = net(util.synth_input(1, seed=3).to(cuda_device))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (1, 1000) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())


def test_cbam_resnet50_batch8_eager_and_graph_are_bit_identical(cuda_device, monkeypatch):
    from pytorchcv_amd.graph import capture
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    name = "cbam_resnet50"
    logits, ids = util.model_golden(name)
    net = _net(name, None, cuda_device)
    x = util.images(ids).to(cuda_device).repeat(2, 1, 1, 1).contiguous()
    with torch.no_grad():
        y_eager = net(x).clone()
        y_again = net(x).clone()
        g = capture(net, x)
        y_graph = g(x, clone=True)
    torch.cuda.synchronize()
    assert torch.equal(y_eager, y_again)
    assert torch.equal(y_graph, y_eager), "graph differs in {} rows".format(int((y_graph != y_eager).any(1).sum()))
    assert torch.equal(y_eager[:4], y_eager[4:])
    assert torch.equal(y_eager.argmax(1).cpu(), logits.argmax(1).repeat(2))
    del g
    torch.cuda.empty_cache()
