"""
GPU tests of split attention (ResNeSt-A, SKNet) and the padded average pool: the four new C-ABI entry points against a float64
restatement of the reference's SABlock.forward (pytorchcv/models/common/att.py:172-189) and against torch's avg_pool2d, the
reference block goldens of tests/golden/blocks_splat.npz, and the three fixture nets end to end.

Bounds (written here on purpose):
  kernels, fp32   : |y - exact| <= 1e-5 * (sum_r a_r |x_r| + |residual|) - relative to the sum's conditioning, not to |y|
  kernels, 16 bit : one rounding of the exact result, |y - exact| <= 2^-8 (bf16) / 2^-11 (fp16) * |exact| + the fp32 term above
  blocks          : fp32 <= 1e-3 of the golden; 16 bit the golden bounds of tests/test_gpu_blocks.py (x3 for units)
  nets            : fp32 <= 1e-3 of the reference's golden logits; default mode <= 1e-2, top-1 identical, no fp16 overflow;
                    bf16 and fp16 top-1 identical
"""

import os
import json
import ctypes
import pytest
import numpy as np
import torch
import torch.nn.functional as F
import util

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
FLOOR = {"fp32": 1e-30, "bf16": 1e-30, "fp16": 2.0 ** -25}        # half of fp16's subnormal spacing: tiny results round absolutely


def _nhwc(t):
    from pytorchcv_amd import engine
    N, H, W, C = t.shape
    return engine.NHWC(t.contiguous(), N, H, W, C)


def _representable(shape, seed, dtype, scale=1.0):
    """Values exactly representable in bf16 AND fp16 (bf16 rounding, magnitudes well inside fp16's range)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(torch.float16).float()
    return v


def _mlp(C, R, seed):
    g = torch.Generator().manual_seed(seed)
    M = max(R * C // 4, 32)
    return (torch.randn(M, C, generator=g) * 0.2, torch.randn(M, generator=g) * 0.1, torch.randn(R * C, M, generator=g) * 0.2,
            torch.randn(R * C, generator=g) * 0.1)


def _splat_ref(x, R, groups, w1, b1, w2, b2, res=None, relu=False):
    """float64 restatement of SABlock.forward on NHWC x [N, H, W, R*C]; returns (y, sum_r a_r |x_r| + |res|)."""
    x = x.double()
    N, H, W, RC = x.shape
    C = RC // R
    xs = x.view(N, H, W, R, C)
    s = xs.sum(dim=3).mean(dim=(1, 2))
    mid = torch.relu(s @ w1.double().t() + b1.double())
    lg = (mid @ w2.double().t() + b2.double()).view(N, groups, R, C // groups).transpose(1, 2).contiguous()
    a = torch.softmax(lg, dim=1).view(N, 1, 1, R, C)
    y = (xs * a).sum(dim=3)
    cond = (xs.abs() * a).sum(dim=3)
    if res is not None:
        y = y + res.double()
        cond = cond + res.double().abs()
    if relu:
        y = torch.relu(y)
    return y, cond


_KSHAPES = [(hw, C, R) for hw in (7, 15, 56) for C in (32, 64, 1024) for R in (1, 2, 3, 4)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("hw,C,R", _KSHAPES, ids=["{}x{}_c{}_r{}".format(h, h, c, r) for h, c, r in _KSHAPES])
def test_split_attention_kernels_vs_float64(hw, C, R, dtype, cuda_device):
    from pytorchcv_amd import engine
    groups = (1, 2, 4)[(hw + C + R) % 3]
    with_res = (R + C // 32) % 2 == 0
    seed = hw * 1000 + C + R
    x = _representable((3, hw, hw, R * C), seed, dtype)
    res = _representable((3, hw, hw, C), seed + 1, dtype) if with_res else None
    w1, b1, w2, b2 = _mlp(C, R, seed + 2)
    ref, cond = _splat_ref(x, R, groups, w1, b1, w2, b2, res, relu=with_res)
    dev = cuda_device
    d = [t.to(dev).contiguous() for t in (w1, b1, w2, b2)]
    y = engine.splat_forward(_nhwc(x.to(dev, TDT[dtype])), R, groups, *d,
                             residual=_nhwc(res.to(dev, TDT[dtype])) if res is not None else None, post_act=1 if with_res else 0)
    torch.cuda.synchronize()
    assert y.C == C and tuple(y.t.shape) == (3, hw, hw, C) and y.dtype == TDT[dtype]
    out = y.t.double().cpu()
    err = (out - ref).abs()
    bound = ULP[dtype] * ref.abs() + 1e-5 * cond * (1 + ULP[dtype]) + FLOOR[dtype]
    bad = err > bound
    i = int((err - bound).argmax())
    assert not bool(bad.any()), "{} elements out of bound; worst excess at |d| {:.3e}, ref {:.4e}, cond {:.3e}".format(
        int(bad.sum()), float(err.flatten()[i]), float(ref.flatten()[i]), float(cond.flatten()[i]))


def _ctx():
    from pytorchcv_amd import _lib
    return _lib.lib(), _lib.ctx_for(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_radix_one_squeeze_and_unpadded_pool_keep_their_bits(dtype, cuda_device):
    """pcv_se_squeeze is the radix-1 squeeze and pcv_avgpool2d the unpadded pool: same kernels, same bits."""
    from pytorchcv_amd import _lib
    L, ctx = _ctx()
    code = {"fp32": 0, "bf16": 1, "fp16": 2}[dtype]
    for (N, H, W, C) in [(3, 7, 7, 64), (2, 56, 56, 256), (4, 14, 14, 1024)]:
        x = _representable((N, H, W, C), H + C, dtype).to(cuda_device, TDT[dtype])
        a = torch.empty((N, C), dtype=torch.float32, device=cuda_device)
        b = torch.empty_like(a)
        _lib.check(L.pcv_se_squeeze(ctx, _p(x), _p(a), N, H * W, C, code, _stream()), ctx)
        _lib.check(L.pcv_splat_squeeze(ctx, _p(x), _p(b), N, H * W, C, 1, code, _stream()), ctx)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert torch.allclose(a.cpu().double(), x.double().cpu().mean(dim=(1, 2)), rtol=1e-5, atol=1e-6)
        for k, s in ((2, 2), (3, 1), (3, 2), (7, 1)):
            if k > H:
                continue
            Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
            p1 = torch.empty((N, Ho, Wo, C), dtype=TDT[dtype], device=cuda_device)
            p2 = torch.empty_like(p1)
            _lib.check(L.pcv_avgpool2d(ctx, _p(x), _p(p1), N, H, W, C, k, s, code, code, _stream()), ctx)
            for cip in (0, 1):
                _lib.check(L.pcv_avgpool2d_pad(ctx, _p(x), _p(p2), N, H, W, C, k, s, 0, 0, cip, code, code, _stream()), ctx)
                torch.cuda.synchronize()
                assert torch.equal(p1, p2), (k, s, cip)


def _pool_configs():
    out = []
    for n in (7, 8, 15, 56):
        for k in (2, 3):
            for s in (1, 2):
                for p in (0, 1):
                    if 2 * p > k:
                        continue
                    for ceil in (0, 1):
                        for cip in (0, 1):
                            out.append((n, k, s, p, ceil, cip))
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_padded_avgpool_vs_torch(dtype, cuda_device):
    from pytorchcv_amd import engine
    ran = 0
    for (n, k, s, p, ceil, cip) in _pool_configs():
        C = 16 if n == 56 else 24
        x = _representable((2, n, n, C), n * 100 + k * 10 + s, dtype)
        ref = F.avg_pool2d(x.permute(0, 3, 1, 2), k, s, p, ceil_mode=bool(ceil), count_include_pad=bool(cip)).permute(0, 2, 3, 1)
        y = engine.avgpool2d_pad(_nhwc(x.to(cuda_device, TDT[dtype])), k, s, p, bool(ceil), bool(cip))
        torch.cuda.synchronize()
        assert tuple(y.t.shape) == tuple(ref.shape), (n, k, s, p, ceil, cip)
        err = (y.t.float().cpu() - ref).abs()
        bound = ULP[dtype] * ref.abs() + 2e-6 * (1 + x.abs().max())
        assert bool((err <= bound).all()), ((n, k, s, p, ceil, cip), float(err.max()))
        ran += 1
    assert ran == len(_pool_configs()) > 100


def test_multi_round_launches_are_bit_identical(cuda_device):
    """With every grid capped at a few blocks (several rounds per block) squeeze, combine and pool compute the same bits."""
    from pytorchcv_amd import engine
    for dtype in ("bf16", "fp16", "fp32"):
        x = _representable((3, 15, 15, 2 * 64), 77, dtype).to(cuda_device, TDT[dtype])
        res = _representable((3, 15, 15, 64), 78, dtype).to(cuda_device, TDT[dtype])
        w = [t.to(cuda_device) for t in _mlp(64, 2, 79)]
        y0 = engine.splat_forward(_nhwc(x), 2, 2, *w, residual=_nhwc(res), post_act=1).t.clone()
        p0 = engine.avgpool2d_pad(_nhwc(x), 3, 2, 1, False, True).t.clone()
        with util.tuning(max_blocks=3):
            y1 = engine.splat_forward(_nhwc(x), 2, 2, *w, residual=_nhwc(res), post_act=1).t.clone()
            p1 = engine.avgpool2d_pad(_nhwc(x), 3, 2, 1, False, True).t.clone()
        torch.cuda.synchronize()
        assert torch.equal(y0, y1) and torch.equal(p0, p1), dtype


def test_fp16_range_guard_on_combine_and_pool(cuda_device):
    from pytorchcv_amd import engine
    x = torch.full((1, 4, 4, 2 * 16), 60000.0, dtype=torch.float16, device=cuda_device)
    res = torch.full((1, 4, 4, 16), 60000.0, dtype=torch.float16, device=cuda_device)
    w = [t.to(cuda_device) for t in _mlp(16, 2, 5)]
    before = engine.fp16_overflow_count(cuda_device)
    y = engine.splat_forward(_nhwc(x), 2, 1, *w, residual=_nhwc(res))
    torch.cuda.synchronize()
    mid = engine.fp16_overflow_count(cuda_device)
    assert mid > before and bool(torch.isinf(y.t.float()).all())
    xp = torch.ones((1, 6, 6, 16), dtype=torch.float16, device=cuda_device)
    xp[0, 2, 2, :] = float("inf")
    xp[0, 3, 3, :8] = -float("inf")
    yp = engine.avgpool2d_pad(_nhwc(xp), 3, 2, 1, False, True)
    torch.cuda.synchronize()
    assert engine.fp16_overflow_count(cuda_device) > mid
    assert bool(torch.isinf(yp.t.float()).any())
    # inside the range nothing is counted
    quiet = engine.fp16_overflow_count(cuda_device)
    engine.splat_forward(_nhwc(torch.ones_like(x)), 2, 1, *w)
    engine.avgpool2d_pad(_nhwc(torch.ones_like(xp)), 3, 2, 1, False, True)
    assert engine.fp16_overflow_count(cuda_device) == quiet


def test_refusals(cuda_device):
    from pytorchcv_amd import _lib
    L, ctx = _ctx()
    st = _stream()
    x = torch.zeros(2 * 4 * 4 * 4 * 64, device=cuda_device)
    y = torch.zeros_like(x)
    s = torch.zeros(2 * 4 * 64, device=cuda_device)

    def invalid(rc):
        with pytest.raises(_lib.PcvError) as e:
            _lib.check(rc, ctx)
        assert e.value.code == -1

    # squeeze: C % 8, radix range, NULL, dtype
    invalid(L.pcv_splat_squeeze(ctx, _p(x), _p(s), 2, 16, 12, 2, 0, st))
    invalid(L.pcv_splat_squeeze(ctx, _p(x), _p(s), 2, 16, 64, 0, 0, st))
    invalid(L.pcv_splat_squeeze(ctx, _p(x), _p(s), 2, 16, 64, 5, 0, st))
    invalid(L.pcv_splat_squeeze(ctx, None, _p(s), 2, 16, 64, 2, 0, st))
    invalid(L.pcv_splat_squeeze(ctx, _p(x), _p(s), 2, 16, 64, 2, 7, st))
    # excite: groups not dividing C, radix, C % 8, NULL
    m = torch.zeros(4096, device=cuda_device)
    args = [_p(s), _p(m), _p(m), _p(m), _p(m), _p(m), _p(m), _p(m)]
    invalid(L.pcv_splat_excite(ctx, *args, 2, 64, 32, 2, 3, st))
    invalid(L.pcv_splat_excite(ctx, *args, 2, 64, 32, 5, 1, st))
    invalid(L.pcv_splat_excite(ctx, *args, 2, 60, 32, 2, 1, st))
    invalid(L.pcv_splat_excite(ctx, *args, 2, 64, 32, 2, 0, st))
    invalid(L.pcv_splat_excite(ctx, *(args[:-1] + [None]), 2, 64, 32, 2, 1, st))
    # combine: C % 8, radix, NULL, dtype, post_act
    invalid(L.pcv_splat_combine(ctx, _p(x), _p(m), None, _p(y), 2, 16, 20, 2, 0, 1, st))
    invalid(L.pcv_splat_combine(ctx, _p(x), _p(m), None, _p(y), 2, 16, 64, 0, 0, 1, st))
    invalid(L.pcv_splat_combine(ctx, _p(x), None, None, _p(y), 2, 16, 64, 2, 0, 1, st))
    invalid(L.pcv_splat_combine(ctx, _p(x), _p(m), None, None, 2, 16, 64, 2, 0, 1, st))
    invalid(L.pcv_splat_combine(ctx, _p(x), _p(m), None, _p(y), 2, 16, 64, 2, 0, 3, st))
    invalid(L.pcv_splat_combine(ctx, _p(x), _p(m), None, _p(y), 2, 16, 64, 2, 99, 1, st))
    # pool: C % 8, pad > k / 2, dtype / out_dtype mismatch, NULL, empty output
    invalid(L.pcv_avgpool2d_pad(ctx, _p(x), _p(y), 2, 8, 8, 12, 3, 2, 1, 0, 1, 1, 1, st))
    invalid(L.pcv_avgpool2d_pad(ctx, _p(x), _p(y), 2, 8, 8, 16, 2, 2, 2, 0, 1, 1, 1, st))
    invalid(L.pcv_avgpool2d_pad(ctx, _p(x), _p(y), 2, 8, 8, 16, 3, 2, 1, 0, 1, 1, 2, st))
    invalid(L.pcv_avgpool2d_pad(ctx, None, _p(y), 2, 8, 8, 16, 3, 2, 1, 0, 1, 1, 1, st))
    invalid(L.pcv_avgpool2d_pad(ctx, _p(x), _p(y), 2, 2, 2, 16, 7, 2, 2, 0, 1, 1, 1, st))     # window wider than the padded map
    torch.cuda.synchronize()


# ---- reference block goldens ---------------------------------------------------------------------------------------------------
def _blocks():
    with open(os.path.join(util.GOLDEN, "blocks_splat.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(util.GOLDEN, "blocks_splat.npz")), meta


_BLOCK_NAMES = sorted(_blocks()[1])


def _run_block(name, dtype, dev):
    import pytorchcv_amd
    from test_splat_host import build_splat_block
    npz, meta = _blocks()
    m = meta[name]
    blk = build_splat_block(m["case"])
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)
    blk = pytorchcv_amd.set_compute_dtype(blk.to(dev), dtype)
    x = util.synth_input(*m["case"]["x"], seed=m["input_seed"])
    with torch.no_grad():
        y = blk(x.to(dev))
    torch.cuda.synchronize()
    return y.float().cpu(), torch.from_numpy(npz[name]), m["case"]["kind"]


@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_fp32_matches_reference_golden(name, cuda_device):
    y, g, _ = _run_block(name, "fp32", cuda_device)
    assert y.shape == g.shape
    assert float((y - g).abs().max()) <= 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_16bit_matches_reference_golden(name, dtype, cuda_device):
    y, g, kind = _run_block(name, dtype, cuda_device)
    assert y.shape == g.shape
    mult = 3.0 if kind in ("ResNeStAUnit", "SEInitBlock") else 1.0
    rtol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * mult
    atol = (4e-2 if dtype == "bf16" else 1e-2) * mult
    dg = (y - g).abs()
    assert bool((dg <= atol + rtol * g.abs()).all()), "vs fp32 golden: max |d| {:.3e}".format(float(dg.max()))


# ---- whole nets ----------------------------------------------------------------------------------------------------------------
NETS = ["resnesta18", "resnesta50", "sknet50"]


def _net(name, dtype, dev):
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name).eval()
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
def test_net_16bit_top1_matches_reference(name, dtype, cuda_device):
    logits, ids = util.model_golden(name)
    net = _net(name, dtype, cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    print("{} {}: vs golden {:.3e}".format(name, dtype, float((y - logits).abs().max())))
    assert bool(torch.isfinite(y).all()) and torch.equal(y.argmax(1), logits.argmax(1))


def test_resnesta50_full_batch_eager_and_graph_match_fixture(cuda_device):
    """The 4 golden images tiled to batch 256: every row of the eager forward, of a second eager forward and of the 2-lane graph
    replay is bit-identical to the 4-image forward."""
    from pytorchcv_amd.graph import capture
    name, batch = "resnesta50", 256
    logits, ids = util.model_golden(name)
    net = _net(name, None, cuda_device)
    x4 = util.images(ids).to(cuda_device)
    with torch.no_grad():
        y4 = net(x4).clone()
        x = x4.repeat(batch // 4, 1, 1, 1).contiguous()
        y_eager = net(x).clone()
        y_again = net(x).clone()
        g = capture(net, x, lanes=2)
        assert g.lanes == 2
        y_graph = g(x, clone=True)
    torch.cuda.synchronize()
    want = y4.repeat(batch // 4, 1)
    assert torch.equal(y_eager, y_again)
    assert torch.equal(y_eager, want), "eager differs in {} rows".format(int((y_eager != want).any(1).sum()))
    assert torch.equal(y_graph, want), "graph differs in {} rows".format(int((y_graph != want).any(1).sum()))
    assert torch.equal(y_graph.argmax(1).cpu(), logits.argmax(1).repeat(batch // 4))
    del g, x, y_eager, y_graph
    torch.cuda.empty_cache()
