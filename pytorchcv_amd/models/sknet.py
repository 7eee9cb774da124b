"""
    SKNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/sknet.py:15-300). Module tree, attribute names and
    factory signatures follow the reference so its state_dicts load strictly. The selective-kernel block's branches write their
    channel slices of one [N, H, W, M * C] buffer straight from the convolution epilogue (no stack, no copy, no NCHW), and the
    selection is the split-attention launches of common/att.py with groups = 1.
"""

__all__ = ['SKNet', 'sknet50', 'sknet101', 'sknet152', 'SKConvBlock', 'SKNetBottleneck', 'SKNetUnit', 'get_sknet']

import torch
import torch.nn as nn
from .common.conv import conv1x1, conv1x1_block, conv3x3_block
from .common.att import fold_bn_into_fc, _FoldedMlp
from .resnet import SkipUnit, ResInitBlock, resnet_channels
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class SKConvBlock(nn.Module):
    """M dilated grouped 3x3 branches + selection (reference sknet.py:15-83). `branches` is a plain container with the reference's
    child names (branch2, branch3, ...), so the state_dict keys match its `Concurrent(stack=True)`."""
    def __init__(self, in_channels, out_channels, stride, groups=32, num_branches=2, reduction=16, min_channels=32):
        super(SKConvBlock, self).__init__()
        self.num_branches = num_branches
        self.out_channels = out_channels
        mid_channels = max(in_channels // reduction, min_channels)
        self.branches = nn.Sequential()
        for i in range(num_branches):
            dilation = 1 + i
            self.branches.add_module("branch{}".format(i + 2), conv3x3_block(
                in_channels=in_channels, out_channels=out_channels, stride=stride, padding=dilation, dilation=dilation,
                groups=groups))
        self.pool = nn.AdaptiveAvgPool2d(output_size=1)       # marker only; the squeeze kernel computes it
        self.fc1 = conv1x1_block(in_channels=out_channels, out_channels=mid_channels)
        self.fc2 = conv1x1(in_channels=mid_channels, out_channels=(out_channels * num_branches))
        self.softmax = nn.Softmax(dim=1)
        self._pcv_mlp = _FoldedMlp()

    def _mlp(self):
        c1, bn, w2 = self.fc1.conv, self.fc1.bn, self.fc2.weight
        srcs = [c1.weight, c1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, w2]

        def build():
            w1, b1 = fold_bn_into_fc(c1.weight, c1.bias, bn)
            w2f = w2.detach().float().reshape(w2.shape[0], -1).contiguous()
            return w1, b1, w2f, torch.zeros(w2f.shape[0], dtype=torch.float32, device=w2f.device)
        return self._pcv_mlp.get(srcs, build)

    def _run(self, a):
        C, M = self.out_channels, self.num_branches
        if C % 8:
            raise NotImplementedError("SKConvBlock with {} channels: the MI355X path needs multiples of 8".format(C))
        c = self.branches.branch2.conv
        s, k = c.stride[0], c.kernel_size[0]
        Ho = (a.H + 2 * c.padding[0] - c.dilation[0] * (k - 1) - 1) // s + 1
        Wo = (a.W + 2 * c.padding[1] - c.dilation[1] * (k - 1) - 1) // c.stride[1] + 1
        buf = torch.empty((a.N, Ho, Wo, M * C), dtype=a.dtype, device=a.device)
        for i, branch in enumerate(self.branches.children()):
            branch(a, out=(buf, i * C))                       # the convolution writes its channel slice: no stack
        w1, b1, w2, b2 = self._mlp()
        return engine.splat_forward(engine.NHWC(buf, a.N, Ho, Wo, M * C), M, 1, w1, b1, w2, b2)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class SKNetBottleneck(nn.Module):
    """1x1 -> selective-kernel block -> 1x1 (reference sknet.py:86-130); `residual` / `post_act` ride in conv3's epilogue."""
    def __init__(self, in_channels, out_channels, stride, bottleneck_factor=2):
        super(SKNetBottleneck, self).__init__()
        mid_channels = out_channels // bottleneck_factor
        self.conv1 = conv1x1_block(in_channels=in_channels, out_channels=mid_channels)
        self.conv2 = SKConvBlock(in_channels=mid_channels, out_channels=mid_channels, stride=stride)
        self.conv3 = conv1x1_block(in_channels=mid_channels, out_channels=out_channels, activation=None)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self.conv3(self.conv2(self.conv1(a)), residual=residual, post_act=post_act))


class SKNetUnit(SkipUnit):
    """relu(body(x) + identity) (reference sknet.py:133-176)."""
    def __init__(self, in_channels, out_channels, stride):
        super(SKNetUnit, self).__init__()
        self.body = SKNetBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride)
        self.add_skip(in_channels, out_channels, stride)


class SKNet(ClassifierNet):
    """`features` (ResInitBlock, stage1..4, final_pool) + `output` Linear (reference sknet.py:179-245)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(SKNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        self.finish(add_stages(self.features, init_block_channels, channels,
                               make_unit=lambda cin, cout, stride, i, j: SKNetUnit(in_channels=cin, out_channels=cout, stride=stride)))


def get_sknet(blocks, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    net = SKNet(channels=resnet_channels(blocks, True, what="SKNet", depths=(50, 101, 152)), init_block_channels=64, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_sknet, {"sknet{}".format(n): dict(blocks=n) for n in (50, 101, 152)})
