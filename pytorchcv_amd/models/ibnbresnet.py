"""
    IBN(b)-ResNet for ImageNet-1K on the MI355X hot path (https://arxiv.org/abs/1807.09441; reference
    pytorchcv/models/ibnbresnet.py): ResNet-b (stride on the 3x3) with InstanceNorm2d in three places - after the stem
    convolution instead of its BatchNorm, and over the whole output of the last unit of stages 1 and 2, after the skip add and
    before the ReLU. Every other unit is `ResUnit(conv1_stride=False)` and runs ResNet's routes.
"""

__all__ = ['IBNbResNet', 'ibnb_resnet50', 'ibnb_resnet101', 'ibnb_resnet152', 'IBNbConvBlock', 'ibnb_conv7x7_block',
           'IBNbResUnit', 'IBNbResInitBlock', 'get_ibnbresnet']

import torch.nn as nn
from .resnet import ResStage, ResUnit, resnet_channels
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import MaxPool2dNHWC, maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class IBNbConvBlock(nn.Module):
    """Convolution -> InstanceNorm2d(affine) -> ReLU (reference ibnbresnet.py:15-74): the convolution runs bare (scale 1, shift 0,
    no activation), pcv_instnorm_act over all its channels carries the ReLU."""
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False, activate=True):
        super(IBNbConvBlock, self).__init__()
        self.activate = activate
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                              padding=padding, dilation=dilation, groups=groups, bias=bias)
        self.inst_norm = nn.InstanceNorm2d(num_features=out_channels, affine=True)
        if self.activate:
            self.activ = nn.ReLU(inplace=True)
        self._pcv_runner = None
        self._pcv_in = None

    def _run(self, a):
        if self._pcv_runner is None:
            self._pcv_runner = engine.ConvRunner(self.conv, None)
            self._pcv_in = engine.InstNormRunner(self.inst_norm)
        return self._pcv_in.run(self._pcv_runner.run(a, act=0), engine.act_code(self.activ if self.activate else None))

    def forward(self, x, stem=False):
        return engine.boundary(self, x, self._run, stem=stem)


def ibnb_conv7x7_block(in_channels, out_channels, stride=1, padding=3, bias=False, activate=True):
    return IBNbConvBlock(in_channels=in_channels, out_channels=out_channels, kernel_size=7, stride=stride, padding=padding,
                         bias=bias, activate=activate)


class IBNbResUnit(ResUnit):
    """ResNet-b bottleneck unit; with `use_inst_norm`, relu(inst_norm(body(x) + identity)) (reference ibnbresnet.py:111-162):
    conv3 takes the skip add with no activation behind it, pcv_instnorm_act over all channels carries the ReLU. Without it the
    unit IS ResUnit (keys, arithmetic, fused routes)."""
    def __init__(self, in_channels, out_channels, stride, use_inst_norm):
        super(IBNbResUnit, self).__init__(in_channels=in_channels, out_channels=out_channels, stride=stride, conv1_stride=False)
        self.use_inst_norm = use_inst_norm
        if self.use_inst_norm:
            self.inst_norm = nn.InstanceNorm2d(num_features=out_channels, affine=True)
        self._pcv_in = None

    def _norm_tail(self, a, y):
        z = self.body.conv3(y, residual=self._identity(a), post_act=None)
        if self._pcv_in is None:
            self._pcv_in = engine.InstNormRunner(self.inst_norm)
        return self._pcv_in.run(z, engine.act_code(self.activ))

    def _run(self, a):
        if not self.use_inst_norm:
            return super(IBNbResUnit, self)._run(a)
        return self._norm_tail(a, self.body.conv2(self.body.conv1(a)))

    def run_chained(self, a, conv1_out=None, next_unit=None):
        if not self.use_inst_norm:
            return super(IBNbResUnit, self).run_chained(a, conv1_out, next_unit)
        # the norm sits between this unit's conv3 and whatever follows: no whole-unit launch, nothing handed on
        y = self.body.conv2(conv1_out if conv1_out is not None else self.body.conv1(a))
        return self._norm_tail(a, y), None

    def fuses_whole(self, a_prev):
        return False if self.use_inst_norm else super(IBNbResUnit, self).fuses_whole(a_prev)


class IBNbResInitBlock(nn.Module):
    """7x7/2 convolution -> InstanceNorm2d -> ReLU -> MaxPool2d(3, 2, 1) (reference ibnbresnet.py:165-192)."""
    def __init__(self, in_channels, out_channels):
        super(IBNbResInitBlock, self).__init__()
        self.conv = ibnb_conv7x7_block(in_channels=in_channels, out_channels=out_channels, stride=2)
        self.pool = MaxPool2dNHWC(kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        return engine.boundary(self, x, lambda a: self.pool(self.conv(a)), stem=True)


class IBNbResNet(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` Linear (reference ibnbresnet.py:195-261)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(IBNbResNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", IBNbResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        width = add_stages(self.features, init_block_channels, channels, container=ResStage,
                           make_unit=lambda cin, cout, stride, i, j: IBNbResUnit(
                               in_channels=cin, out_channels=cout, stride=stride,
                               use_inst_norm=(i < 2) and (j == len(channels[i]) - 1)))
        self.finish(width)


def get_ibnbresnet(blocks, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    net = IBNbResNet(channels=resnet_channels(blocks, True, what="IBN(b)-ResNet", depths=(50, 101, 152)), init_block_channels=64,
                     **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_ibnbresnet, {"ibnb_resnet{}".format(n): dict(blocks=n) for n in (50, 101, 152)})
