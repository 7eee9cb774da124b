"""
GPU: RegNetX / RegNetY on the hot path against the imported reference's fixtures (tests/golden/make_golden_regnet.py) - the
RegNetUnit cases of blocks_regnet.json (X and Y units, stride 1 and 2, with and without identity_conv, at 8 / 24 / 40 / 56 / 64
channels per group; the 64-wide units on the generic kernel) and regnetx002 / regnety016 end to end at batch 4, 224x224. fp32 within 1e-3 of the golden; 16 bit within the
golden bounds of tests/test_gpu_blocks.py x 3 (a unit chains three to four convolutions, as tests/test_gpu_ghostnet.py); the nets'
default mode within the project's 1e-2 with the reference's top-1, finite logits and no fp16 overflow; both 16-bit distances are
printed (DESIGN.md's parity table). A captured forward equals the eager one bit for bit; an image's logits do not depend on its place
in the batch; with "gconvx" 0 (every grouped layer on the generic kernel) a net stays within the same bounds.
"""

import os
import numpy as np
import pytest
import torch
import util
from test_regnet_host import blocks_meta, build_unit, FIXTURE_NETS
from test_gpu_gconvx_sweep import gconvx

pytestmark = pytest.mark.gpu

_npz = None


def _golden(name):
    global _npz
    if _npz is None:
        z = np.load(os.path.join(util.GOLDEN, "blocks_regnet.npz"))
        _npz = {k: z[k] for k in z.files}
    return torch.from_numpy(_npz[name])


_UNIT_NAMES = sorted(blocks_meta())


def _run_unit(name, dtype, dev):
    import pytorchcv_amd
    m = blocks_meta()[name]
    blk = build_unit(m["case"])
    blk.load_state_dict(util.synth_state_dict(blk.state_dict(), seed=m["weight_seed"]), strict=True)
    blk = pytorchcv_amd.set_compute_dtype(blk.to(dev), dtype)
    x = util.synth_input(*m["case"]["x"], seed=m["input_seed"]).to(dev)
    with torch.no_grad():
        y = blk(x)
    torch.cuda.synchronize()
    return y.float().cpu(), _golden(name)


@pytest.mark.parametrize("name", _UNIT_NAMES)
def test_unit_fp32_matches_reference_golden(name, cuda_device):
    y, g = _run_unit(name, "fp32", cuda_device)
    assert y.shape == g.shape
    err = float((y - g).abs().max())
    print("{} fp32: vs golden {:.3e}".format(name, err))
    assert err <= 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", _UNIT_NAMES)
def test_unit_16bit_matches_reference_golden(name, dtype, cuda_device):
    y, g = _run_unit(name, dtype, cuda_device)
    assert y.shape == g.shape
    rtol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * 3.0
    atol = (4e-2 if dtype == "bf16" else 1e-2) * 3.0
    dg = (y - g).abs()
    print("{} {}: vs golden {:.3e}".format(name, dtype, float(dg.max())))
    assert bool((dg <= atol + rtol * g.abs()).all()), "vs fp32 golden: max |d| {:.3e}".format(float(dg.max()))


def test_unit_conv2_runs_on_the_grouped_kernel_by_the_library_s_own_routing(cuda_device):
    """every 16-bit unit case: conv2's descriptor, as the engine builds it, is one pcv_gconvx_supported takes"""
    import ctypes
    from pytorchcv_amd import _lib
    from test_regnet_host import _desc
    L = _lib.lib()
    for name in _UNIT_NAMES:
        case = blocks_meta()[name]["case"]
        kw, (N, _, H, W) = case["kwargs"], case["x"]
        d = _desc(kw["out_channels"], kw["groups"], H, W, kw["stride"], N=N)
        want = int(kw["groups"] != 64)                 # (64 per group went back to the generic kernel: gconvx_pays)
        assert L.pcv_gconvx_supported(ctypes.byref(d)) == want, (name, L.pcv_last_error(None))


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


def _default_mode_check(name, dev):
    from pytorchcv_amd import engine
    logits, ids = util.model_golden(name)
    net = _net(name, None, dev)
    before = engine.fp16_overflow_count(dev)
    with torch.no_grad():
        y = net(util.images(ids).to(dev))
    torch.cuda.synchronize()
    assert engine.fp16_overflow_count(dev) == before
    y = y.cpu()
    err = float((y - logits).abs().max())
    print("{} default ({}): vs golden {:.3e}".format(name, engine.compute_dtype_of(net), err))
    assert bool(torch.isfinite(y).all()) and torch.equal(y.argmax(1), logits.argmax(1))
    assert err <= 1e-2
    return y


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_net_default_mode_within_north_star_bound(name, cuda_device, monkeypatch):
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    _default_mode_check(name, cuda_device)


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_net_on_the_generic_kernel_stays_within_the_same_bounds(name, cuda_device, monkeypatch):
    """pcv_set_tuning("gconvx", 0): the composed path of every grouped layer"""
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    with gconvx(0):
        _default_mode_check(name, cuda_device)


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
