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
from ._tail import MaxPool2dNHWC, AvgPool2dPadNHWC, GlobalAvgPool2dNHWC, LinearHead, run_net, maybe_load_pretrained, \
    init_conv_params, DEFAULT_ROOT
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


class ResNeStAUnit(nn.Module):
    """relu(body(x) + identity) (reference resnesta.py:152-200)."""
    def __init__(self, in_channels, out_channels, stride, bottleneck=True):
        super(ResNeStAUnit, self).__init__()
        self.resize_identity = (in_channels != out_channels) or (stride != 1)
        if bottleneck:
            self.body = ResNeStABottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride)
        else:
            self.body = ResNeStABlock(in_channels=in_channels, out_channels=out_channels, stride=stride)
        if self.resize_identity:
            self.identity_block = ResNeStADownBlock(in_channels=in_channels, out_channels=out_channels, stride=stride)
        self.activ = nn.ReLU(inplace=True)

    def _run(self, a):
        identity = self.identity_block(a) if self.resize_identity else a
        return self.body(a, residual=identity, post_act=self.activ)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class ResNeStA(nn.Module):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` (dropout, fc) (reference resnesta.py:203-275)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)
    def __init__(self, channels, init_block_channels, bottleneck, dropout_rate=0.0, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(ResNeStA, self).__init__()
        self.in_size = in_size
        self.num_classes = num_classes
        self.features = nn.Sequential()
        self.features.add_module("init_block", SEInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        in_channels = init_block_channels
        for i, channels_per_stage in enumerate(channels):
            stage = nn.Sequential()
            for j, out_channels in enumerate(channels_per_stage):
                stride = 2 if (j == 0) and (i != 0) else 1
                stage.add_module("unit{}".format(j + 1), ResNeStAUnit(in_channels=in_channels, out_channels=out_channels, stride=stride,
                                                                      bottleneck=bottleneck))
                in_channels = out_channels
            self.features.add_module("stage{}".format(i + 1), stage)
        self.features.add_module("final_pool", GlobalAvgPool2dNHWC(output_size=1, fp32_out=True))
        self.output = nn.Sequential()
        if dropout_rate > 0.0:
            self.output.add_module("dropout", nn.Dropout(p=dropout_rate))       # identity in eval mode: not run on the hot path
        self.output.add_module("fc", LinearHead(in_features=in_channels, out_features=num_classes))
        init_conv_params(self)
        engine.stamp_family_dtype(self)                    # sub-modules called on their own resolve "auto" like the net

    def forward(self, x):
        return run_net(self, x, self.output.fc)


def get_resnesta(blocks, bottleneck=None, width_scale=1.0, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    if bottleneck is None:
        bottleneck = (blocks >= 50)
    layers = {10: [1, 1, 1, 1], 12: [2, 1, 1, 1], 16: [2, 2, 2, 1], 18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3],
              101: [3, 4, 23, 3], 152: [3, 8, 36, 3], 200: [3, 24, 36, 3], 269: [3, 30, 48, 8]}.get(blocks)
    if blocks == 14:
        layers = [1, 1, 1, 1] if bottleneck else [2, 2, 1, 1]
    elif blocks == 26:
        layers = [2, 2, 2, 2] if bottleneck else [3, 3, 3, 3]
    elif blocks == 38 and bottleneck:
        layers = [3, 3, 3, 3]
    if layers is None:
        raise ValueError("Unsupported ResNeSt(A) with number of blocks: {}".format(blocks))
    assert sum(layers) * (3 if bottleneck else 2) + 2 == blocks
    init_block_channels = 64
    channels_per_layers = [64, 128, 256, 512]
    if blocks >= 101:
        init_block_channels *= 2
    if bottleneck:
        channels_per_layers = [ci * 4 for ci in channels_per_layers]
    channels = [[ci] * li for (ci, li) in zip(channels_per_layers, layers)]
    if width_scale != 1.0:
        channels = [[int(cij * width_scale) if (i != len(channels) - 1) or (j != len(ci) - 1) else cij
                     for j, cij in enumerate(ci)] for i, ci in enumerate(channels)]
        init_block_channels = int(init_block_channels * width_scale)
    net = ResNeStA(channels=channels, init_block_channels=init_block_channels, bottleneck=bottleneck, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


def resnestabc14(**kwargs):
    return get_resnesta(blocks=14, bottleneck=True, model_name="resnestabc14", **kwargs)


def resnesta18(**kwargs):
    return get_resnesta(blocks=18, model_name="resnesta18", **kwargs)


def resnestabc26(**kwargs):
    return get_resnesta(blocks=26, bottleneck=True, model_name="resnestabc26", **kwargs)


def resnesta50(**kwargs):
    return get_resnesta(blocks=50, model_name="resnesta50", **kwargs)


def resnesta101(**kwargs):
    return get_resnesta(blocks=101, model_name="resnesta101", **kwargs)


def resnesta152(**kwargs):
    return get_resnesta(blocks=152, model_name="resnesta152", **kwargs)


def resnesta200(in_size=(256, 256), **kwargs):
    return get_resnesta(blocks=200, in_size=in_size, model_name="resnesta200", **kwargs)


def resnesta269(in_size=(320, 320), **kwargs):
    return get_resnesta(blocks=269, in_size=in_size, model_name="resnesta269", **kwargs)
