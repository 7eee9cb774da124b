"""
Host-side mechanisms of pytorchcv_amd/engine.py that need neither a GPU nor the library: the batch splitter (driven with a fake
launch), the pure-torch half of the BatchNorm fold, and ConvBlock's lazy runner.
"""

import pytest
import torch
import torch.nn as nn
from pytorchcv_amd import engine, parallel, _lib
from pytorchcv_amd.models.common.conv import ConvBlock, conv1x1_block

TOO_LARGE = _lib.PCV_ERR_TOO_LARGE


# ---- the batch splitter ---------------------------------------------------------------------------------------------------------
class FakeLaunch(object):
    """Refuses a range of more than `limit` images as too large when the caller accepts that code; records everything it is asked."""
    def __init__(self, limit):
        self.limit, self.asked, self.done = limit, [], []

    def __call__(self, n0, n1, accept):
        self.asked.append((n0, n1, tuple(accept)))
        if n1 - n0 > self.limit and TOO_LARGE in accept:
            return TOO_LARGE
        self.done.append((n0, n1))
        return 0


@pytest.mark.parametrize("limit", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 2, 3, 5, 8])
def test_split_batch_covers_the_batch_in_order(N, limit):
    f = FakeLaunch(limit)
    engine._split_batch(N, f)
    assert f.done[0][0] == 0 and f.done[-1][1] == N
    for (a0, a1), (b0, b1) in zip(f.done, f.done[1:]):
        assert a1 == b0                                         # ascending, disjoint, no gap: together exactly [0, N)
    assert all(0 < n1 - n0 <= limit for n0, n1 in f.done)
    assert f.asked[0][:2] == (0, N)
    for i, (n0, n1, accept) in enumerate(f.asked):
        assert accept == ((TOO_LARGE,) if n1 - n0 > 1 else ())  # a single image is launched with nothing accepted
        if (n0, n1) not in f.done:                              # refused: the left half is asked next, the right half later
            mid = (n0 + n1) // 2
            assert f.asked[i + 1][:2] == (n0, mid)
            assert (mid, n1) in [a[:2] for a in f.asked[i + 2:]]
    assert len(f.asked) == len(f.done) + (len(f.done) - 1)      # a binary tree: every refusal adds exactly two requests


def test_split_batch_single_image_refusal_is_not_retried():
    """What `_call` does with an empty `accept` is raise; a launch that returns the code all the same is not split into [n, n) + [n, n + 1)."""
    asked = []

    def stubborn(n0, n1, accept):
        asked.append((n0, n1))
        return TOO_LARGE
    engine._split_batch(2, stubborn)
    assert asked == [(0, 2), (0, 1), (1, 2)]


# ---- the pure-torch half of the BatchNorm fold ----------------------------------------------------------------------------------
def _random_bn(C, affine=True):
    g = torch.Generator().manual_seed(C)
    bn = nn.BatchNorm2d(C, affine=affine).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        if affine:
            bn.weight.copy_(torch.randn(C, generator=g))
            bn.bias.copy_(torch.randn(C, generator=g))
    return bn


def test_bn_fold_sources_pad_to_the_physical_width():
    bn = _random_bn(12)
    conv_bias = torch.randn(12)
    g, b, m, v, bias = engine._bn_fold_sources(bn, 16, conv_bias)
    for got, src, fill in ((g, bn.weight, 0.0), (b, bn.bias, 0.0), (m, bn.running_mean, 0.0), (v, bn.running_var, 1.0), (bias, conv_bias, 0.0)):
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (16,)
        assert torch.equal(got[:12], src.detach())              # the source values, bit for bit
        assert torch.equal(got[12:], torch.full((4,), fill))    # pad channels: gamma, beta, mean, bias 0 and var 1 -> scale 0, shift 0


def test_bn_fold_sources_defaults_without_affine_parameters():
    bn = _random_bn(16, affine=False)
    g, b, m, v, bias = engine._bn_fold_sources(bn, 16)
    assert torch.equal(g, torch.ones(16)) and torch.equal(b, torch.zeros(16)) and bias is None
    assert torch.equal(m, bn.running_mean) and torch.equal(v, bn.running_var)


def test_bn_fold_sources_without_bn_and_refusal():
    conv_bias = torch.randn(12)
    g, b, m, v, bias = engine._bn_fold_sources(None, 16, conv_bias)
    assert g is None and b is None and m is None and v is None                  # pcv_bn_fold's no-BN form: scale 1, shift bias
    assert torch.equal(bias[:12], conv_bias) and torch.equal(bias[12:], torch.zeros(4))
    assert engine._bn_fold_sources(None, 16) == (None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="only BatchNorm2d folds into the conv epilogue, got GroupNorm"):
        engine._bn_fold_sources(nn.GroupNorm(4, 16), 16)
    with pytest.raises(NotImplementedError, match="only BatchNorm2d folds to scale/shift, got GroupNorm"):
        engine._bn_fold_sources(nn.GroupNorm(4, 16), 16, what="to scale/shift")


# ---- ConvBlock.runner() ---------------------------------------------------------------------------------------------------------
def test_conv_block_runner_is_lazy_single_and_carries_pad4():
    blk = ConvBlock(in_channels=8, out_channels=16, kernel_size=3, padding=(0, 1, 0, 1))
    assert blk._pcv_runner is None and list(parallel._runners(blk)) == []      # built on first use, not in __init__
    r = blk.runner()
    assert isinstance(r, engine.ConvRunner) and blk.runner() is r and blk._pcv_runner is r
    assert r.pad4 == (0, 1, 0, 1) and r.conv is blk.conv and r.bn is blk.bn
    assert list(parallel._runners(blk)) == [r]
    plain = conv1x1_block(in_channels=8, out_channels=8, normalization=None, activation=None)
    assert plain.runner().pad4 is None and plain.runner().bn is None and plain.act_code() == 0
    assert blk.act_code() == engine.act_code(blk.activ) == 1
