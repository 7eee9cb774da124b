"""
    IBN-ResNet for ImageNet-1K on the MI355X hot path ('Two at Once: Enhancing Learning and Generalization Capacities via
    IBN-Net', https://arxiv.org/abs/1807.09441; reference pytorchcv/models/ibnresnet.py). Module tree, attribute names and
    factory signatures follow the reference so its state_dicts load strictly.

    A unit with IBN (stages 1-3: `out_channels < 2048`) runs as conv1 with the BatchNorm half folded and no activation, one
    pcv_instnorm_act (InstanceNorm half + ReLU; two launches), then conv2 and conv3 (+ skip add + ReLU) as ordinary fused
    convolutions: 5 launches, 6 with `identity_conv`. Its conv1 cannot be the tail of another unit's launch - the statistics
    need the whole map - so these stages are plain sequences. Units without IBN (stage 4) are `ResUnit(conv1_stride=False)`:
    same keys, same arithmetic, and ResNet's fused routes.
"""

__all__ = ['IBNResNet', 'ibn_resnet50', 'ibn_resnet101', 'ibn_resnet152', 'ibn_conv1x1_block', 'IBNConvBlock',
           'IBNResBottleneck', 'IBNResUnit', 'get_ibnresnet']

import torch.nn as nn
from .common.norm import IBN
from .common.conv import conv1x1_block, conv3x3_block
from .resnet import SkipUnit, ResInitBlock, ResStage, ResUnit, resnet_channels
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class IBNConvBlock(nn.Module):
    """Convolution + IBN or BatchNorm + ReLU (reference ibnresnet.py:16-83). With `use_ibn`: one convolution launch (BatchNorm
    half in the epilogue, act NONE) and pcv_instnorm_act over (C, Cn = C / 2) with the ReLU; without, the ordinary fused block."""
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False,
                 use_ibn=False, activate=True):
        super(IBNConvBlock, self).__init__()
        self.activate = activate
        self.use_ibn = use_ibn
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                              padding=padding, dilation=dilation, groups=groups, bias=bias)
        if self.use_ibn:
            self.ibn = IBN(channels=out_channels)
        else:
            self.bn = nn.BatchNorm2d(num_features=out_channels)
        if self.activate:
            self.activ = nn.ReLU(inplace=True)
        self._pcv_runner = None

    def _run(self, a):
        act = engine.act_code(self.activ if self.activate else None)
        if self._pcv_runner is None:
            self._pcv_runner = engine.IBNConvRunner(self.conv, self.ibn) if self.use_ibn else engine.ConvRunner(self.conv, self.bn)
        if not self.use_ibn:
            return self._pcv_runner.run(a, act=act)
        return self.ibn.run_inst(self._pcv_runner.run(a, act=0), act)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


def ibn_conv1x1_block(in_channels, out_channels, stride=1, groups=1, bias=False, use_ibn=False, activate=True):
    return IBNConvBlock(in_channels=in_channels, out_channels=out_channels, kernel_size=1, stride=stride, padding=0,
                        groups=groups, bias=bias, use_ibn=use_ibn, activate=activate)


class IBNResBottleneck(nn.Module):
    """1x1 (IBN) -> 3x3 (carries the stride) -> 1x1 (reference ibnresnet.py:125-165); `residual` / `post_act` ride on conv3."""
    def __init__(self, in_channels, out_channels, stride, conv1_ibn):
        super(IBNResBottleneck, self).__init__()
        mid_channels = out_channels // 4
        self.conv1 = ibn_conv1x1_block(in_channels=in_channels, out_channels=mid_channels, use_ibn=conv1_ibn)
        self.conv2 = conv3x3_block(in_channels=mid_channels, out_channels=mid_channels, stride=stride)
        self.conv3 = conv1x1_block(in_channels=mid_channels, out_channels=out_channels, activation=None)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self.conv3(self.conv2(self.conv1(a)), residual=residual, post_act=post_act))


class IBNResUnit(SkipUnit):
    """relu(body(x) + identity) (reference ibnresnet.py:168-212). Not chainable: see the module docstring."""
    def __init__(self, in_channels, out_channels, stride, conv1_ibn):
        super(IBNResUnit, self).__init__()
        self.body = IBNResBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride, conv1_ibn=conv1_ibn)
        self.add_skip(in_channels, out_channels, stride)


def ibn_unit(in_channels, out_channels, stride):
    """The unit of the net builders: IBN on conv1 while `out_channels < 2048` (reference ibnresnet.py:252), else ResNet's unit."""
    if out_channels < 2048:
        return IBNResUnit(in_channels=in_channels, out_channels=out_channels, stride=stride, conv1_ibn=True)
    return ResUnit(in_channels=in_channels, out_channels=out_channels, stride=stride, conv1_stride=False)


class IBNResNet(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` Linear (reference ibnresnet.py:215-281)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(IBNResNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        width = add_stages(self.features, init_block_channels, channels, container=ResStage,
                           make_unit=lambda cin, cout, stride, i, j: ibn_unit(cin, cout, stride))
        self.finish(width)


def get_ibnresnet(blocks, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    net = IBNResNet(channels=resnet_channels(blocks, True, what="IBN-ResNet", depths=(50, 101, 152)), init_block_channels=64, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_ibnresnet, {"ibn_resnet{}".format(n): dict(blocks=n) for n in (50, 101, 152)})
