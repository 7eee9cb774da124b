"""
GPU: GhostNet on the hot path against the imported reference's fixtures (tests/golden/make_golden_ghostnet.py) - the block cases of
blocks_ghostnet.json (ghost modules with half widths 8, 12, 92 and 60, on a 1x1 map too; units with the skip add in the ghost launch,
with `identity_conv`, the strided 5x5 and the clamp-gated SE; the classifier) and the net end to end at batch 4, 224x224. fp32
within 1e-3 of the golden; 16 bit within the golden bounds of tests/test_gpu_blocks.py (x 3 for units, as tests/test_gpu_ibn.py); the
net's default mode within the project's 1e-2 with the reference's top-1, finite logits and no fp16 overflow; both 16-bit distances
are printed (DESIGN.md's parity table); a captured forward equals the eager one bit for bit; an image's logits do not depend on its
place in the batch.
"""

import os
import numpy as np
import pytest
import torch
import util
from test_ghostnet_host import blocks_meta, build_ghost_block

pytestmark = pytest.mark.gpu

NAME = "ghostnet"

_npz = None


def _golden(key):
    global _npz
    if _npz is None:
        z = np.load(os.path.join(util.GOLDEN, "blocks_ghostnet.npz"))
        _npz = {k: z[k] for k in z.files}
    return torch.from_numpy(_npz[key])


_BLOCK_NAMES = sorted(blocks_meta())


def _run_block(name, dtype, dev):
    import pytorchcv_amd
    m = blocks_meta()[name]
    blk = build_ghost_block(m["case"])
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)
    blk = pytorchcv_amd.set_compute_dtype(blk.to(dev), dtype)
    x = util.synth_input(*m["case"]["x"], seed=m["input_seed"]).to(dev)
    with torch.no_grad():
        y = blk(x)
    torch.cuda.synchronize()
    return y.float().cpu(), _golden(name), m["case"]["kind"]


@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_fp32_matches_reference_golden(name, cuda_device):
    y, g, _ = _run_block(name, "fp32", cuda_device)
    assert y.shape == g.shape
    err = float((y - g).abs().max())
    print("{} fp32: vs golden {:.3e}".format(name, err))
    assert err <= 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", _BLOCK_NAMES)
def test_block_16bit_matches_reference_golden(name, dtype, cuda_device):
    y, g, kind = _run_block(name, dtype, cuda_device)
    assert y.shape == g.shape
    mult = 3.0 if kind.endswith("Unit") else 1.0
    rtol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * mult
    atol = (4e-2 if dtype == "bf16" else 1e-2) * mult
    dg = (y - g).abs()
    print("{} {}: vs golden {:.3e}".format(name, dtype, float(dg.max())))
    assert bool((dg <= atol + rtol * g.abs()).all()), "vs fp32 golden: max |d| {:.3e}".format(float(dg.max()))


# ---- the whole net --------------------------------------------------------------------------------------------------------------
def _net(dtype, dev):
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    net = get_model(NAME).eval()
    net.load_state_dict(util.model_state(NAME, net.state_dict()), strict=True)
    net = net.to(dev)
    return net if dtype is None else pytorchcv_amd.set_compute_dtype(net, dtype)


def test_net_fp32_matches_reference_golden(cuda_device):
    logits, ids = util.model_golden(NAME)
    assert len(ids) == 4
    net = _net("fp32", cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    err = float((y - logits).abs().max())
    print("{} fp32: vs golden {:.3e}".format(NAME, err))
    assert err <= 1e-3 and torch.equal(y.argmax(1), logits.argmax(1))


def test_net_default_mode_within_north_star_bound(cuda_device, monkeypatch):
    from pytorchcv_amd import engine
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    logits, ids = util.model_golden(NAME)
    net = _net(None, cuda_device)
    before = engine.fp16_overflow_count(cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device))
    torch.cuda.synchronize()
    assert engine.fp16_overflow_count(cuda_device) == before
    y = y.cpu()
    err = float((y - logits).abs().max())
    print("{} default ({}): vs golden {:.3e}".format(NAME, engine.compute_dtype_of(net), err))
    assert bool(torch.isfinite(y).all()) and torch.equal(y.argmax(1), logits.argmax(1))
    assert err <= 1e-2


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_net_16bit_distance_is_reported(dtype, cuda_device):
    """Both 16-bit modes: finite logits; the distance is printed (DESIGN.md's parity table)."""
    logits, ids = util.model_golden(NAME)
    net = _net(dtype, cuda_device)
    with torch.no_grad():
        y = net(util.images(ids).to(cuda_device)).cpu()
    print("{} {}: vs golden {:.3e} top-1 equal {}".format(NAME, dtype, float((y - logits).abs().max()),
                                                         bool(torch.equal(y.argmax(1), logits.argmax(1)))))
    assert bool(torch.isfinite(y).all())


def test_width_scale_with_an_odd_half_width_is_refused_at_the_first_forward(cuda_device):
    """width 0.5 gives stage 2 a 12-channel ghost module (Cm = 6): it builds, and the forward raises instead of computing something"""
    from pytorchcv_amd.models.ghostnet import get_ghostnet
    net = get_ghostnet(width_scale=0.5).eval().to(cuda_device)
    assert net.features.stage2.unit1.body.pw_conv.cheap_conv.conv.out_channels == 6
    with torch.no_grad(), pytest.raises(NotImplementedError, match="multiple of 4"):
        net(torch.zeros(1, 3, 64, 64, device=cuda_device))
    torch.cuda.synchronize()


def test_net_eager_and_graph_are_bit_identical(cuda_device, monkeypatch):
    from pytorchcv_amd.graph import capture
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    logits, ids = util.model_golden(NAME)
    net = _net(None, cuda_device)
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
    _, ids = util.model_golden(NAME)
    net = _net(None, cuda_device)
    x = util.images(ids[:3]).to(cuda_device)
    with torch.no_grad():
        y3 = net(x).clone()
        y1 = net(x[1:2].contiguous()).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y3).all())
    assert torch.equal(y3[1:2], y1)
