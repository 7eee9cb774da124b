"""
    PreResNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/preresnet.py:19-330): pre-activation units.
    Inside a unit every BatchNorm+ReLU that follows a convolution rides in that convolution's epilogue (conv1 carries
    conv2's pre-activation, conv2 carries conv3's); only the unit's first pre-activation, whose input the skip path needs
    raw, is its own elementwise launch. The skip add is the epilogue of the unit's last convolution.
"""

__all__ = ['PreResNet', 'preresnet10', 'preresnet12', 'preresnet14', 'preresnetbc14b', 'preresnet16', 'preresnet18_wd4',
           'preresnet18_wd2', 'preresnet18_w3d4', 'preresnet18', 'preresnet26', 'preresnetbc26b', 'preresnet34',
           'preresnetbc38b', 'preresnet50', 'preresnet50b', 'preresnet101', 'preresnet101b', 'preresnet152',
           'preresnet152b', 'preresnet200', 'preresnet200b', 'preresnet269b', 'PreResBlock', 'PreResBottleneck',
           'PreResUnit', 'PreResInitBlock', 'PreResActivation', 'get_preresnet']

import torch.nn as nn
from .common.norm import lambda_batchnorm2d
from .common.conv import pre_conv1x1_block, pre_conv3x3_block, conv1x1
from .resnet import SkipUnit, resnet_channels, RESNET_DEPTHS
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import MaxPool2dNHWC, maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class PreResBlock(nn.Module):
    """Two pre-activated 3x3 convolutions (reference preresnet.py:19-61); returns (x, x_pre_activ)."""
    def __init__(self, in_channels, out_channels, stride, bias=False, normalization=lambda_batchnorm2d()):
        super(PreResBlock, self).__init__()
        self.conv1 = pre_conv3x3_block(in_channels=in_channels, out_channels=out_channels, stride=stride, bias=bias,
                                       normalization=normalization, return_preact=True)
        self.conv2 = pre_conv3x3_block(in_channels=out_channels, out_channels=out_channels, bias=bias,
                                       normalization=normalization)

    def chain(self):
        return [self.conv1, self.conv2]

    def forward(self, x):
        return _run_body(self, x)


class PreResBottleneck(nn.Module):
    """1x1 -> 3x3 -> 1x1 pre-activated bottleneck (reference preresnet.py:64-106)."""
    def __init__(self, in_channels, out_channels, stride, conv1_stride):
        super(PreResBottleneck, self).__init__()
        mid_channels = out_channels // 4
        self.conv1 = pre_conv1x1_block(in_channels=in_channels, out_channels=mid_channels,
                                       stride=(stride if conv1_stride else 1), return_preact=True)
        self.conv2 = pre_conv3x3_block(in_channels=mid_channels, out_channels=mid_channels,
                                       stride=(1 if conv1_stride else stride))
        self.conv3 = pre_conv1x1_block(in_channels=mid_channels, out_channels=out_channels)

    def chain(self):
        return [self.conv1, self.conv2, self.conv3]

    def forward(self, x):
        return _run_body(self, x)


def _chain_forward(blocks, a, residual=None, se=None):
    """`a` is already pre-activated for blocks[0]; block i's convolution carries block i+1's BN+activation. `se`: the SEBlock
    that follows the body (SE-PreResNet): it runs inside the last convolution when that is a 1x1 (PreConvBlock.conv_then)."""
    for i, blk in enumerate(blocks):
        last = (i + 1 == len(blocks))
        a = blk.conv_then(a, next_block=(None if last else blocks[i + 1]), residual=(residual if last else None),
                          se=(se if last else None))
    return a


def _run_body(body, x):
    """Body used on its own (drop-in block): (x, x_pre_activ), NCHW in -> NCHW out."""
    def run(a):
        blocks = body.chain()
        pre = blocks[0].preact(a)
        return _chain_forward(blocks, pre), pre
    return engine.boundary(body, x, run)               # (tensor entry: the module's resolved type + the fp16 range guard)


class PreResUnit(SkipUnit):
    """Pre-activation residual unit (reference preresnet.py:109-164): the identity convolution, when present, reads the
    pre-activated input and has neither BN nor activation."""
    def __init__(self, in_channels, out_channels, stride, bias=False, normalization=lambda_batchnorm2d(), bottleneck=True,
                 conv1_stride=False):
        super(PreResUnit, self).__init__()
        if bottleneck:
            self.body = PreResBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride,
                                         conv1_stride=conv1_stride)
        else:
            self.body = PreResBlock(in_channels=in_channels, out_channels=out_channels, stride=stride, bias=bias,
                                    normalization=normalization)
        self.add_skip(in_channels, out_channels, stride, block=conv1x1, activation=None, bias=bias)

    def _run(self, a, se=None):
        """`se`: the SEBlock between the body and the add (SEPreResUnit runs this function with its own)."""
        blocks = self.body.chain()
        pre = blocks[0].preact(a)
        identity = self.identity_conv(pre) if self.resize_identity else a
        return _chain_forward(blocks, pre, residual=identity, se=se)


class PreResInitBlock(nn.Module):
    """7x7/2 conv + BN + ReLU + 3x3/2 max-pool with the parameters directly on the block (reference preresnet.py:167-196)."""
    def __init__(self, in_channels, out_channels):
        super(PreResInitBlock, self).__init__()
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=7, stride=2, padding=3,
                              bias=False)
        self.bn = nn.BatchNorm2d(num_features=out_channels)
        self.activ = nn.ReLU(inplace=True)
        self.pool = MaxPool2dNHWC(kernel_size=3, stride=2, padding=1)
        self._pcv_runner = None

    def _run(self, a):
        if self._pcv_runner is None:
            self._pcv_runner = engine.ConvRunner(self.conv, self.bn)
        y = self._pcv_runner.run_maxpool(a, engine.act_code(self.activ), self.pool.kernel_size, self.pool.stride, self.pool.padding,
                                         self.pool.ceil_mode)
        return y if y is not None else self.pool(self._pcv_runner.run(a, act=engine.act_code(self.activ)))

    def forward(self, x):
        return engine.boundary(self, x, self._run, stem=True)


class PreResActivation(nn.Module):
    """The BatchNorm + ReLU that closes the pre-activation trunk (reference preresnet.py:199-222)."""
    def __init__(self, in_channels):
        super(PreResActivation, self).__init__()
        self.bn = nn.BatchNorm2d(num_features=in_channels)
        self.activ = nn.ReLU(inplace=True)
        self._pcv_pre = None

    def _run(self, a):
        if self._pcv_pre is None:
            self._pcv_pre = engine.BnActRunner(self.bn)
        return self._pcv_pre.run(a, engine.act_code(self.activ))

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class PreResNet(ClassifierNet):
    unit = PreResUnit            # (SE-PreResNet is this net with its own unit)

    def __init__(self, channels, init_block_channels, bottleneck, conv1_stride, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(PreResNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", PreResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        width = add_stages(
            self.features, init_block_channels, channels,
            make_unit=lambda cin, cout, stride, i, j: self.unit(in_channels=cin, out_channels=cout, stride=stride,
                                                                bottleneck=bottleneck, conv1_stride=conv1_stride))
        self.features.add_module("post_activ", PreResActivation(in_channels=width))
        self.finish(width)


def get_preresnet(blocks, bottleneck=None, conv1_stride=True, width_scale=1.0, model_name=None, pretrained=False,
                  root=DEFAULT_ROOT, **kwargs):
    """Depth table and channel plan of reference preresnet.py:320-369 (same table as ResNet plus 269)."""
    if bottleneck is None:
        bottleneck = (blocks >= 50)
    net = PreResNet(channels=resnet_channels(blocks, bottleneck, "PreResNet", RESNET_DEPTHS + (269,), width_scale),
                    init_block_channels=(64 if width_scale == 1.0 else int(64 * width_scale)), bottleneck=bottleneck,
                    conv1_stride=conv1_stride, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


# name -> get_preresnet arguments (reference preresnet.py:372-878)
_B = dict(conv1_stride=False)
_BC = dict(bottleneck=True, conv1_stride=False)
register_variants(__name__, get_preresnet, {
    "preresnet10": dict(blocks=10), "preresnet12": dict(blocks=12), "preresnet14": dict(blocks=14),
    "preresnetbc14b": dict(blocks=14, **_BC), "preresnet16": dict(blocks=16),
    "preresnet18_wd4": dict(blocks=18, width_scale=0.25), "preresnet18_wd2": dict(blocks=18, width_scale=0.5),
    "preresnet18_w3d4": dict(blocks=18, width_scale=0.75), "preresnet18": dict(blocks=18),
    "preresnet26": dict(blocks=26, bottleneck=False), "preresnetbc26b": dict(blocks=26, **_BC),
    "preresnet34": dict(blocks=34), "preresnetbc38b": dict(blocks=38, **_BC),
    "preresnet50": dict(blocks=50), "preresnet50b": dict(blocks=50, **_B),
    "preresnet101": dict(blocks=101), "preresnet101b": dict(blocks=101, **_B),
    "preresnet152": dict(blocks=152), "preresnet152b": dict(blocks=152, **_B),
    "preresnet200": dict(blocks=200), "preresnet200b": dict(blocks=200, **_B),
    "preresnet269b": dict(blocks=269, **_B)})
