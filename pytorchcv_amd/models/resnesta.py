"""
    ResNeSt(A) with average downsampling for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/resnesta.py:18-420,
    stem senet.py:127-163). Module tree, attribute names and factory signatures follow the reference so its state_dicts load
    strictly. A split-attention convolution is one fused grouped convolution + three split-attention launches (squeeze, excite,
    combine); in the basic block the unit's skip add and ReLU ride in the combine, in the bottleneck in conv3's epilogue.
"""

__all__ = ['ResNeStA', 'resnestabc14', 'resnesta18', 'resnestabc26', 'resnesta50', 'resnesta101', 'resnesta152',
           'resnesta200', 'resnesta269', 'ResNeStADownBlock', 'ResNeStABlock', 'ResNeStABottleneck', 'ResNeStAUnit', 'SEInitBlock',
           'get_resnesta']

import torch.nn as nn
from .common.norm import lambda_batchnorm2d
from .common.conv import conv1x1_block, conv3x3_block, conv_block_maxpool
from .common.att import saconv3x3_block
from .resnet import SkipUnit, resnet_channels, RESNET_DEPTHS
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import MaxPool2dNHWC, AvgPool2dPadNHWC, GlobalAvgPool2dNHWC, dropout_fc_head, maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class SEInitBlock(nn.Module):
    """Three 3x3 ConvBlocks (the first with stride 2) + MaxPool2d(3, 2, 1) (reference senet.py:127-163)."""
    def __init__(self, in_channels, out_channels):
        super(SEInitBlock, self).__init__()
        mid_channels = out_channels // 2
        self.conv1 = conv3x3_block(in_channels=in_channels, out_channels=mid_channels, stride=2)
        self.conv2 = conv3x3_block(in_channels=mid_channels, out_channels=mid_channels)
        self.conv3 = conv3x3_block(in_channels=mid_channels, out_channels=out_channels)
        self.pool = MaxPool2dNHWC(kernel_size=3, stride=2, padding=1)

    def _run(self, a):
        return conv_block_maxpool(self.conv3, self.conv2(self.conv1(a)), self.pool)

    def forward(self, x):
        return engine.boundary(self, x, self._run, stem=True)


class ResNeStABlock(nn.Module):
    """3x3 ConvBlock [-> AvgPool2d(3, stride, 1)] -> split-attention 3x3 block (reference resnesta.py:18-66); `residual` /
    `post_act` ride in the split-attention combine."""
    def __init__(self, in_channels, out_channels, stride, bias=False, normalization=lambda_batchnorm2d()):
        super(ResNeStABlock, self).__init__()
        self.resize = (stride > 1)
        self.conv1 = conv3x3_block(in_channels=in_channels, out_channels=out_channels, bias=bias, normalization=normalization)
        if self.resize:
            self.pool = AvgPool2dPadNHWC(kernel_size=3, stride=stride, padding=1)
        self.conv2 = saconv3x3_block(in_channels=out_channels, out_channels=out_channels, bias=bias, normalization=normalization,
                                     activation=None)

    def _run(self, a, residual=None, post_act=None):
        a = self.conv1(a)
        if self.resize:
            a = self.pool(a)
        return self.conv2(a, residual=residual, post_act=post_act)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual, post_act))


class ResNeStABottleneck(nn.Module):
    """1x1 -> split-attention 3x3 [-> AvgPool2d(3, stride, 1)] -> 1x1 (reference resnesta.py:69-115); `residual` / `post_act`
    ride in conv3's epilogue."""
    def __init__(self, in_channels, out_channels, stride, bottleneck_factor=4):
        super(ResNeStABottleneck, self).__init__()
        self.resize = (stride > 1)
        mid_channels = out_channels // bottleneck_factor
        self.conv1 = conv1x1_block(in_channels=in_channels, out_channels=mid_channels)
        self.conv2 = saconv3x3_block(in_channels=mid_channels, out_channels=mid_channels)
        if self.resize:
            self.pool = AvgPool2dPadNHWC(kernel_size=3, stride=stride, padding=1)
        self.conv3 = conv1x1_block(in_channels=mid_channels, out_channels=out_channels, activation=None)

    def _run(self, a, residual=None, post_act=None):
        a = self.conv2(self.conv1(a))
        if self.resize:
            a = self.pool(a)
        return self.conv3(a, residual=residual, post_act=post_act)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual, post_act))


class ResNeStADownBlock(nn.Module):
    """AvgPool2d(stride, stride, ceil_mode=True, count_include_pad=False) -> 1x1 ConvBlock without activation (reference
    resnesta.py:118-149). With stride 1 the pool is a 1x1 window, the identity: no launch."""
    def __init__(self, in_channels, out_channels, stride):
        super(ResNeStADownBlock, self).__init__()
        self.pool = AvgPool2dPadNHWC(kernel_size=stride, stride=stride, ceil_mode=True, count_include_pad=False)
        self.conv = conv1x1_block(in_channels=in_channels, out_channels=out_channels, activation=None)

    def _run(self, a):
        if self.pool.kernel_size != 1 or self.pool.stride != 1:
            a = self.pool(a)
        return self.conv(a)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class ResNeStAUnit(SkipUnit):
    """relu(body(x) + identity) (reference resnesta.py:152-200)."""
    def __init__(self, in_channels, out_channels, stride, bottleneck=True):
        super(ResNeStAUnit, self).__init__()
        body = ResNeStABottleneck if bottleneck else ResNeStABlock
        self.body = body(in_channels=in_channels, out_channels=out_channels, stride=stride)
        self.add_skip(in_channels, out_channels, stride, block=ResNeStADownBlock, name="identity_block")

    identity_conv = property(lambda self: self.identity_block)      # the reference's name here is `identity_block`


class ResNeStA(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` (dropout, fc) (reference resnesta.py:203-275)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, bottleneck, dropout_rate=0.0, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(ResNeStA, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", SEInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        width = add_stages(self.features, init_block_channels, channels,
                           make_unit=lambda cin, cout, stride, i, j: ResNeStAUnit(in_channels=cin, out_channels=cout, stride=stride,
                                                                                  bottleneck=bottleneck))
        self.finish(width, head=dropout_fc_head(width, num_classes, dropout_rate), pool=GlobalAvgPool2dNHWC(output_size=1, fp32_out=True))

    def _head(self, a):
        return self.output.fc(a)


def get_resnesta(blocks, bottleneck=None, width_scale=1.0, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    if bottleneck is None:
        bottleneck = (blocks >= 50)
    init_block_channels = 128 if blocks >= 101 else 64
    net = ResNeStA(channels=resnet_channels(blocks, bottleneck, "ResNeSt(A)", RESNET_DEPTHS + (269,), width_scale),
                   init_block_channels=(init_block_channels if width_scale == 1.0 else int(init_block_channels * width_scale)),
                   bottleneck=bottleneck, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_resnesta, {
    "resnestabc14": dict(blocks=14, bottleneck=True), "resnesta18": dict(blocks=18), "resnestabc26": dict(blocks=26, bottleneck=True),
    "resnesta50": dict(blocks=50), "resnesta101": dict(blocks=101), "resnesta152": dict(blocks=152),
    "resnesta200": dict(blocks=200, in_size=(256, 256)), "resnesta269": dict(blocks=269, in_size=(320, 320))})
