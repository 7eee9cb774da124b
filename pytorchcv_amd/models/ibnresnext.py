"""
    IBN-ResNeXt for ImageNet-1K on the MI355X hot path (https://arxiv.org/abs/1807.09441; reference
    pytorchcv/models/ibnresnext.py): IBN-ResNet's unit with the grouped 3x3 of ResNeXt. conv1 of stages 1-3 goes through IBN
    (one convolution launch + pcv_instnorm_act), stage 4 is ResNeXt's own unit with its fused routes.
"""

__all__ = ['IBNResNeXt', 'ibn_resnext50_32x4d', 'ibn_resnext101_32x4d', 'ibn_resnext101_64x4d', 'IBNResNeXtBottleneck',
           'IBNResNeXtUnit', 'get_ibnresnext']

import math
import torch.nn as nn
from .common.conv import conv1x1_block, conv3x3_block
from .resnet import SkipUnit, ResInitBlock, ResStage, resnet_channels
from .resnext import ResNeXtUnit
from .ibnresnet import ibn_conv1x1_block
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class IBNResNeXtBottleneck(nn.Module):
    """1x1 (IBN) -> grouped 3x3 (carries the stride) -> 1x1 (reference ibnresnext.py:16-65)."""
    def __init__(self, in_channels, out_channels, stride, cardinality, bottleneck_width, conv1_ibn):
        super(IBNResNeXtBottleneck, self).__init__()
        mid_channels = out_channels // 4
        D = int(math.floor(mid_channels * (bottleneck_width / 64.0)))
        group_width = cardinality * D
        self.conv1 = ibn_conv1x1_block(in_channels=in_channels, out_channels=group_width, use_ibn=conv1_ibn)
        self.conv2 = conv3x3_block(in_channels=group_width, out_channels=group_width, stride=stride, groups=cardinality)
        self.conv3 = conv1x1_block(in_channels=group_width, out_channels=out_channels, activation=None)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self.conv3(self.conv2(self.conv1(a)), residual=residual, post_act=post_act))


class IBNResNeXtUnit(SkipUnit):
    """relu(body(x) + identity) (reference ibnresnext.py:68-120); not chainable, as IBNResUnit."""
    def __init__(self, in_channels, out_channels, stride, cardinality, bottleneck_width, conv1_ibn):
        super(IBNResNeXtUnit, self).__init__()
        self.body = IBNResNeXtBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride,
                                         cardinality=cardinality, bottleneck_width=bottleneck_width, conv1_ibn=conv1_ibn)
        self.add_skip(in_channels, out_channels, stride)


class IBNResNeXt(ClassifierNet):
    """`features` (init_block, stage1..4, final_pool) + `output` Linear (reference ibnresnext.py:123-197)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, cardinality, bottleneck_width, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(IBNResNeXt, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))

        def make_unit(cin, cout, stride, i, j):
            if cout < 2048:                 # (reference ibnresnext.py:166)
                return IBNResNeXtUnit(in_channels=cin, out_channels=cout, stride=stride, cardinality=cardinality,
                                      bottleneck_width=bottleneck_width, conv1_ibn=True)
            return ResNeXtUnit(in_channels=cin, out_channels=cout, stride=stride, cardinality=cardinality,
                               bottleneck_width=bottleneck_width)
        width = add_stages(self.features, init_block_channels, channels, container=ResStage, make_unit=make_unit)
        self.finish(width)


def get_ibnresnext(blocks, cardinality, bottleneck_width, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    net = IBNResNeXt(channels=resnet_channels(blocks, True, what="IBN-ResNeXt", depths=(50, 101)), init_block_channels=64,
                     cardinality=cardinality, bottleneck_width=bottleneck_width, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_ibnresnext, {
    "ibn_resnext50_32x4d": dict(blocks=50, cardinality=32, bottleneck_width=4),
    "ibn_resnext101_32x4d": dict(blocks=101, cardinality=32, bottleneck_width=4),
    "ibn_resnext101_64x4d": dict(blocks=101, cardinality=64, bottleneck_width=4)})
