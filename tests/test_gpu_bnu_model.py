"""
GPU: ResNet-50 with its stage-1 units on the fused bottleneck kernel (csrc/bnu.hpp). The value of an output row may depend on nothing
but the image: a 3-image batch tiled to 6 images must give the 3-image forward's logits twice, bit for bit, eager and from a captured
graph (the two batches are split into different row bands: 3 and 6 images do not fill the chip). The test first shows that the fused
launch is what runs: every stage-1 unit answers through conv_block_bottleneck.
"""

import pytest
import torch

import util

pytestmark = pytest.mark.gpu


def _net(dev):
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    net = get_model("resnet50").eval()
    net.load_state_dict(util.model_state("resnet50", net.state_dict()), strict=True)
    return pytorchcv_amd.set_compute_dtype(net.to(dev), "bf16")


def test_resnet50_rows_do_not_depend_on_the_batch_eager_and_graph(cuda_device, monkeypatch):
    from pytorchcv_amd import engine
    from pytorchcv_amd.graph import capture
    net = _net(cuda_device)
    _, ids = util.model_golden("resnet50")
    x3 = util.images(ids[:3]).to(cuda_device)
    x6 = torch.cat((x3, x3)).contiguous()

    calls = []
    fused = engine.bottleneck_fused

    def counted(*a, **kw):
        y = fused(*a, **kw)
        if not kw.get("probe"):
            calls.append(y is not None)
        return y
    monkeypatch.setattr(engine, "bottleneck_fused", counted)
    with torch.no_grad():
        y3 = net(x3).clone()
    assert calls[:3] == [True, True, True], "the three units of stage 1 must run as the fused launch: {}".format(calls)
    assert not any(calls[3:]), "only the 56 x 56 stage is covered"
    monkeypatch.setattr(engine, "bottleneck_fused", fused)

    with torch.no_grad():
        y6 = net(x6).clone()
        g3, g6 = capture(net, x3), capture(net, x6)
        z3, z6 = g3(x3, clone=True), g6(x6, clone=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y3).all())
    assert torch.equal(y6[:3], y3) and torch.equal(y6[3:], y3), "eager: rows of the 6-image forward differ from the 3-image forward"
    assert torch.equal(z3, y3), "graph (3 images) differs from eager"
    assert torch.equal(z6[:3], y3) and torch.equal(z6[3:], y3), "graph: rows of the 6-image forward differ from the 3-image forward"
    del g3, g6
    torch.cuda.empty_cache()
