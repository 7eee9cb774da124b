"""
Batch splitting at the 2 GiB window (engine._split_batch) at tiny shapes, for every launch that goes through it: a wrapper around
engine._call refuses any of those launches over more than two images as PCV_ERR_TOO_LARGE - where the caller accepts that code - so
a batch of 5 splits into [0, 2) + [2, 5) and the latter again into [2, 3) + [3, 5). What the split run slices - x, residual, gate, y -
must give the unsplit run's result bit for bit. (The real window is met by test_gpu_models.py::test_batch_split_beyond_2gib_window.)
"""

import pytest
import torch
import torch.nn as nn
from pytorchcv_amd import engine, _lib
from ghost_ref import SWEEP_SHAPES
from pytorchcv_amd.models.common.conv import conv1x1_block, dwconv3x3_block

pytestmark = pytest.mark.gpu

N, HW = 5, 6
SPLIT_ENTRIES = ("conv2d_fused", "dwconv2d_fused", "conv2d_gated_fused", "mixconv2d_fused", "ghost_dw_fused")


@pytest.fixture
def window(monkeypatch):
    """{"on": refuse or forward, "refused": [entry point, ...]} of the wrapper installed over engine._call."""
    state = {"on": False, "refused": []}
    real = engine._call

    def call(device, name, *args, accept=()):
        if state["on"] and name in SPLIT_ENTRIES and args[0]._obj.N > 2 and _lib.PCV_ERR_TOO_LARGE in accept:
            state["refused"].append(name)
            return _lib.PCV_ERR_TOO_LARGE
        return real(device, name, *args, accept=accept)
    monkeypatch.setattr(engine, "_call", call)
    return state


def _handle(C, dev, seed):
    x = torch.randn((N, C, HW, HW), generator=torch.Generator().manual_seed(seed))
    return engine.from_nchw(x.to(dev), "bf16", stem=False)


def _settle(module, dev, seed):
    """eval mode, on the device, BatchNorm statistics that are not the identity"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return module.eval().to(dev)


def _dw(C, k, dev, seed):
    torch.manual_seed(seed)
    return nn.Conv2d(C, C, k, padding=k // 2, groups=C, bias=False).to(dev)


def _cases(dev):
    x, res = _handle(16, dev, 1), _handle(16, dev, 2)
    gate = torch.rand((N, 16), generator=torch.Generator().manual_seed(3)).to(dev)
    torch.manual_seed(4)
    pw = _settle(conv1x1_block(in_channels=16, out_channels=16), dev, 5)
    dw = _settle(dwconv3x3_block(in_channels=16, out_channels=16), dev, 6)
    mix = engine.MixConvRunner([_dw(8, 3, dev, 7), _dw(8, 5, dev, 8)], _settle(nn.BatchNorm2d(16), dev, 9))
    Cm = min(s[1] for s in SWEEP_SHAPES)                # the smallest ghost width of tests/test_gpu_ghost.py's sweep
    cheap = engine.ConvRunner(_dw(Cm, 3, dev, 10), _settle(nn.BatchNorm2d(Cm), dev, 11))
    m, res2 = _handle(Cm, dev, 12), _handle(2 * Cm, dev, 13)
    return [("conv2d_fused", lambda: pw(x, residual=res, post_act=nn.ReLU())),
            ("conv2d_gated_fused", lambda: pw.runner().run(x, act=pw.act_code(), residual=res, post_act=1, gate=gate)),
            ("dwconv2d_fused", lambda: dw(x)),
            ("mixconv2d_fused", lambda: mix.run(x, act=1)),
            ("ghost_dw_fused", lambda: engine.ghost_dw(cheap, m, 1, res2))]


def test_split_launches_equal_the_unsplit_launch(window, cuda_device):
    for entry, run in _cases(cuda_device):
        whole = run()
        assert window["refused"] == [], entry
        window["on"] = True
        split = run()
        window["on"] = False
        torch.cuda.synchronize()
        assert window["refused"] == [entry, entry], (entry, window["refused"])      # [0, 5) and [2, 5)
        del window["refused"][:]
        assert whole.t.shape == split.t.shape and whole.t.dtype == torch.bfloat16
        assert not bool(torch.isnan(whole.t.float()).any()), entry
        assert torch.equal(whole.t, split.t), entry
