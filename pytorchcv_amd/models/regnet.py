"""
    RegNetX / RegNetY for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/regnet.py:18-913). Module tree, attribute
    names and state_dict keys are the reference's (`features.stageN.unitM.body.conv2.conv.weight`, `...body.se.conv1.bias`,
    `...identity_conv.bn.weight`, `output.weight`), so its weights load with strict=True. A unit is three launches (four with
    `identity_conv`, seven for RegNetY): conv1 1x1, conv2 - the grouped 3x3 at 8 .. 232 channels per group and any channel count,
    which the library routes to csrc/gconvx.hpp up to 64 channels per group (pcv_gconvx_supported) - and conv3 1x1 with the skip
    add and the ReLU in its epilogue. RegNetY's SE block sits between conv2 and conv3 and gates conv3's INPUT (mid_channels = a
    quarter of the unit's input channels), so it runs composed: squeeze, excitation, channel scale (SEBlock.forward).
"""

__all__ = ['RegNet', 'regnetx002', 'regnetx004', 'regnetx006', 'regnetx008', 'regnetx016', 'regnetx032', 'regnetx040',
           'regnetx064', 'regnetx080', 'regnetx120', 'regnetx160', 'regnetx320', 'regnety002', 'regnety004',
           'regnety006', 'regnety008', 'regnety016', 'regnety032', 'regnety040', 'regnety064', 'regnety080',
           'regnety120', 'regnety160', 'regnety320', 'RegNetBottleneck', 'RegNetUnit', 'get_regnet']

import numpy as np
import torch.nn as nn
from .common.conv import conv1x1_block, conv3x3_block
from .common.att import SEBlock
from .resnet import SkipUnit
from ._build import ClassifierNet, add_stages, register_variants, stage_table
from ._tail import GlobalAvgPool2dNHWC, maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class RegNetBottleneck(nn.Module):
    """1x1 -> grouped 3x3 (`groups` = CHANNELS PER GROUP, as in the reference) -> [SE] -> 1x1 (reference regnet.py:18-72);
    `residual` / `post_act` ride on conv3."""
    def __init__(self, in_channels, out_channels, stride, groups, use_se, bottleneck_factor=1):
        super(RegNetBottleneck, self).__init__()
        self.use_se = use_se
        mid_channels = out_channels // bottleneck_factor
        mid_groups = mid_channels // groups
        self.conv1 = conv1x1_block(in_channels=in_channels, out_channels=mid_channels)
        self.conv2 = conv3x3_block(in_channels=mid_channels, out_channels=mid_channels, stride=stride, groups=mid_groups)
        if self.use_se:
            self.se = SEBlock(channels=mid_channels, mid_channels=(in_channels // 4))
        self.conv3 = conv1x1_block(in_channels=mid_channels, out_channels=out_channels, activation=None)

    def _run(self, a, residual, post_act):
        y = self.conv2(self.conv1(a))
        if self.use_se:
            y = self.se(y)
        return self.conv3(y, residual=residual, post_act=post_act)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual, post_act))


class RegNetUnit(SkipUnit):
    """relu(body(x) + identity) (reference regnet.py:75-123); the identity a strided 1x1 block where the shape changes."""
    def __init__(self, in_channels, out_channels, stride, groups, use_se):
        super(RegNetUnit, self).__init__()
        self.body = RegNetBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride, groups=groups, use_se=use_se)
        self.add_skip(in_channels, out_channels, stride)


class RegNet(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` Linear (reference regnet.py:126-197)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, groups, use_se, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(RegNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", conv3x3_block(in_channels=in_channels, out_channels=init_block_channels, stride=2,
                                                             padding=1))
        width = add_stages(
            self.features, init_block_channels, channels, downsample_first=True,
            make_unit=lambda cin, cout, stride, i, j: RegNetUnit(in_channels=cin, out_channels=cout, stride=stride,
                                                                 groups=groups[i], use_se=use_se))
        self.finish(width, pool=GlobalAvgPool2dNHWC(output_size=1, fp32_out=True))


def regnet_widths(channels_init, channels_slope, channels_mult, depth, groups):
    """(channels per stage, units per stage, channels per group per stage) of reference regnet.py:239-255: the linear width ramp
    quantised to powers of `channels_mult` and multiples of 8, then adjusted to whole groups."""
    divisor = 8
    assert (channels_slope >= 0) and (channels_init > 0) and (channels_mult > 1) and (channels_init % divisor == 0)
    channels_cont = np.arange(depth) * channels_slope + channels_init
    channels_exps = np.round(np.log(channels_cont / channels_init) / np.log(channels_mult))
    channels = channels_init * np.power(channels_mult, channels_exps)
    channels = (np.round(channels / divisor) * divisor).astype(int)
    channels_per_stage, layers = np.unique(channels, return_counts=True)
    groups_per_stage = [int(min(groups, c)) for c in channels_per_stage]
    channels_per_stage = [int(round(c / g) * g) for c, g in zip(channels_per_stage, groups_per_stage)]
    return channels_per_stage, [int(n) for n in layers], groups_per_stage


def get_regnet(channels_init, channels_slope, channels_mult, depth, groups, use_se=False, model_name=None, pretrained=False,
               root=DEFAULT_ROOT, **kwargs):
    channels_per_stage, layers, groups_per_stage = regnet_widths(channels_init, channels_slope, channels_mult, depth, groups)
    net = RegNet(channels=stage_table(channels_per_stage, layers), init_block_channels=32, groups=groups_per_stage, use_se=use_se, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


# name -> (channels_init, channels_slope, channels_mult, depth, channels per group) (reference regnet.py:296-913)
_X = {"002": (24, 36.44, 2.49, 13, 8), "004": (24, 24.48, 2.54, 22, 16), "006": (48, 36.97, 2.24, 16, 24), "008": (56, 35.73, 2.28, 16, 16),
      "016": (80, 34.01, 2.25, 18, 24), "032": (88, 26.31, 2.25, 25, 48), "040": (96, 38.65, 2.43, 23, 40), "064": (184, 60.83, 2.07, 17, 56),
      "080": (80, 49.56, 2.88, 23, 120), "120": (168, 73.36, 2.37, 19, 112), "160": (216, 55.59, 2.1, 22, 128),
      "320": (320, 69.86, 2.0, 23, 168)}
_Y = {"002": (24, 36.44, 2.49, 13, 8), "004": (48, 27.89, 2.09, 16, 8), "006": (48, 32.54, 2.32, 15, 16), "008": (56, 38.84, 2.4, 14, 16),
      "016": (48, 20.71, 2.65, 27, 24), "032": (80, 42.63, 2.66, 21, 24), "040": (96, 31.41, 2.24, 22, 64), "064": (112, 33.22, 2.27, 25, 72),
      "080": (192, 76.82, 2.19, 17, 56), "120": (168, 73.36, 2.37, 19, 112), "160": (200, 106.23, 2.48, 18, 112),
      "320": (232, 115.89, 2.53, 20, 232)}


_KEYS = ("channels_init", "channels_slope", "channels_mult", "depth", "groups")
register_variants(__name__, get_regnet, dict(
    [("regnetx" + k, dict(zip(_KEYS, cfg))) for k, cfg in _X.items()] +
    [("regnety" + k, dict(zip(_KEYS, cfg), use_se=True)) for k, cfg in _Y.items()]))
