"""
GPU: HRNet on the hot path against the imported reference's fixtures (tests/golden/make_golden_hrnet.py) - the block cases of
blocks_hrnet.json (UpSamplingBlock at scales 2 and 8, a 2-branch and a 4-branch HRBlock, an HRStage that opens a branch and one that
narrows the init block's 256 channels, the init and the final block) and hrnet_w18_small_v1 / hrnetv2_w18 end to end at batch 4,
224x224. fp32 within 1e-3 of the golden; 16 bit within the golden bounds of tests/test_gpu_blocks.py (x 3 for multi-unit blocks, as
tests/test_gpu_ghostnet.py); the nets' default mode within the project's 1e-2 with the reference's top-1, finite logits and no fp16
overflow; both 16-bit distances are printed (DESIGN.md's parity table). In fp32 the fused exchange (one pcv_hr_fuse launch per
branch) equals the composed one (engine.interpolate + engine.add) bit for bit: same order, same adds. A captured forward equals the
eager one bit for bit; an image's logits do not depend on its place in the batch.
"""

import os
import numpy as np
import pytest
import torch
import util
from test_hrnet_host import blocks_meta, build_hr_block, case_input, FIXTURE_NETS

pytestmark = pytest.mark.gpu

_npz = None


def _golden(name):
    """the list of golden output maps of a block case"""
    global _npz
    if _npz is None:
        z = np.load(os.path.join(util.GOLDEN, "blocks_hrnet.npz"))
        _npz = {k: z[k] for k in z.files}
    n = len(blocks_meta()[name]["y_shapes"])
    return [torch.from_numpy(_npz["{}.{}".format(name, i)]) for i in range(n)]


_BLOCK_NAMES = sorted(blocks_meta())


def _run_block(name, dtype, dev, fused=True):
    import pytorchcv_amd
    from pytorchcv_amd.models import hrnet
    m = blocks_meta()[name]
    blk = build_hr_block(m["case"])
    blk.load_state_dict(util.synth_state_dict(blk.state_dict(), seed=m["weight_seed"]), strict=True)
    blk = pytorchcv_amd.set_compute_dtype(blk.to(dev), dtype)
    x = case_input(m["case"], m["input_seed"])
    x = [t.to(dev) for t in x] if isinstance(x, list) else x.to(dev)
    was = hrnet.FUSED
    hrnet.FUSED = fused
    try:
        with torch.no_grad():
            y = blk(x)
        torch.cuda.synchronize()
    finally:
        hrnet.FUSED = was
    assert isinstance(y, list) == m["y_is_list"]
    ys = y if isinstance(y, list) else [y]
    return [v.float().cpu() for v in ys], _golden(name), m["case"]["kind"]


@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_fp32_matches_reference_golden(name, cuda_device):
    ys, gs, _ = _run_block(name, "fp32", cuda_device)
    assert [y.shape for y in ys] == [g.shape for g in gs]
    err = max(float((y - g).abs().max()) for y, g in zip(ys, gs))
    print("{} fp32: vs golden {:.3e}".format(name, err))
    assert err <= 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_16bit_matches_reference_golden(name, dtype, cuda_device):
    ys, gs, kind = _run_block(name, dtype, cuda_device)
    assert [y.shape for y in ys] == [g.shape for g in gs]
    mult = 1.0 if kind == "UpSamplingBlock" else 3.0            # every other case chains several units
    rtol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * mult
    atol = (4e-2 if dtype == "bf16" else 1e-2) * mult
    for i, (y, g) in enumerate(zip(ys, gs)):
        dg = (y - g).abs()
        print("{}.{} {}: vs golden {:.3e}".format(name, i, dtype, float(dg.max())))
        assert bool((dg <= atol + rtol * g.abs()).all()), "map {} vs fp32 golden: max |d| {:.3e}".format(i, float(dg.max()))


@pytest.mark.parametrize("name", [n for n in _BLOCK_NAMES if blocks_meta()[n]["case"]["kind"] in ("UpSamplingBlock", "HRBlock", "HRStage")])
def test_block_fused_equals_composed_bit_for_bit_in_fp32(name, cuda_device):
    """one launch per branch against interpolate + add per term: fp32 partial sums are not rounded, the order is the same"""
    fused, _, _ = _run_block(name, "fp32", cuda_device, fused=True)
    composed, _, _ = _run_block(name, "fp32", cuda_device, fused=False)
    for i, (a, b) in enumerate(zip(fused, composed)):
        assert torch.equal(a, b), "map {}: {} elements differ".format(i, int((a != b).sum()))


def test_block_fused_path_really_is_one_launch_per_branch(cuda_device, monkeypatch):
    """the 4-branch block: four pcv_hr_fuse launches with the reference's term order, no interpolate, no add"""
    from pytorchcv_amd import engine
    calls = []
    real = engine.hr_fuse
    monkeypatch.setattr(engine, "hr_fuse", lambda s, k, a=0: calls.append((len(s), list(k), a)) or real(s, k, a))
    monkeypatch.setattr(engine, "interpolate", lambda *a, **k: pytest.fail("interpolate on the fused path"))
    monkeypatch.setattr(engine, "add", lambda *a, **k: pytest.fail("add on the fused path"))
    _run_block("block4_18_144", "bf16", cuda_device)
    assert calls == [(4, [0, 1, 2, 3], 1), (4, [0, 0, 1, 2], 1), (4, [0, 0, 0, 1], 1), (4, [0, 0, 0, 0], 1)]


# ---- the two nets ---------------------------------------------------------------------------------------------------------------
def _net(name, dtype, dev):
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name).eval()
    net.load_state_dict(util.model_state(name, net.state_dict()), strict=True)
    net = net.to(dev)
    return net if dtype is None else pytorchcv_amd.set_compute_dtype(net, dtype)


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_net_fp32_matches_reference_golden(name, cuda_device):
    logits, ids = util.model_golden(name)
    assert len(ids) == 4
    net = _net(name, "fp32", cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    err = float((y - logits).abs().max())
    print("{} fp32: vs golden {:.3e}".format(name, err))
    assert err <= 1e-3 and torch.equal(y.argmax(1), logits.argmax(1))


@pytest.mark.parametrize("name", FIXTURE_NETS)
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
@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_net_16bit_distance_is_reported(name, dtype, cuda_device):
    """Both 16-bit modes: finite logits; the distance is printed (DESIGN.md's parity table)."""
    logits, ids = util.model_golden(name)
    net = _net(name, dtype, cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    print("{} {}: vs golden {:.3e} top-1 equal {}".format(name, dtype, float((y - logits).abs().max()),
                                                         bool(torch.equal(y.argmax(1), logits.argmax(1)))))
    assert bool(torch.isfinite(y).all())


def test_net_fused_equals_composed_bit_for_bit_in_fp32(cuda_device):
    """hrnet_w18_small_v1 whole: 9 fuse launches against 9 chains of interpolate + add"""
    from pytorchcv_amd.models import hrnet
    name = FIXTURE_NETS[0]
    _, ids = util.model_golden(name)
    net = _net(name, "fp32", cuda_device)
    x = util.images(ids[:2]).to(cuda_device)
    try:
        with torch.no_grad():
            y_fused = net(x).clone()
            hrnet.FUSED = False
            y_composed = net(x).clone()
    finally:
        hrnet.FUSED = True
    torch.cuda.synchronize()
    assert torch.equal(y_fused, y_composed)


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_net_eager_and_graph_are_bit_identical(name, cuda_device, monkeypatch):
    from pytorchcv_amd.graph import capture
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    logits, ids = util.model_golden(name)
    net = _net(name, None, cuda_device)
    x = util.images(ids).to(cuda_device)
    with torch.no_grad():
        y_eager = net(x).clone()
        y_again = net(x).clone()
        g = capture(net, x)
        y_graph = g(x, clone=True)
    torch.cuda.synchronize()
    assert torch.equal(y_eager, y_again)
    assert torch.equal(y_graph, y_eager), "graph differs in {} rows".format(int((y_graph != y_eager).any(1).sum()))
    del g
    torch.cuda.empty_cache()


def test_net_batch_position_invariance(cuda_device, monkeypatch):
    """net(x)[1] == net(x[1:2]) bit for bit at N = 3, in the default mode."""
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    name = FIXTURE_NETS[1]
    _, ids = util.model_golden(name)
    net = _net(name, None, cuda_device)
    x = util.images(ids[:3]).to(cuda_device)
    with torch.no_grad():
        y3 = net(x).clone()
        y1 = net(x[1:2].contiguous()).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y3).all())
    assert torch.equal(y3[1:2], y1)
