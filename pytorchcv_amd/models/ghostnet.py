"""
    GhostNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/ghostnet.py:18-385). Module tree, attribute names and
    state_dict keys are the reference's (`...body.exp_conv.main_conv.conv.weight`, `...body.pw_conv.cheap_conv.bn.weight`,
    `...identity_conv.dw_conv.conv.weight`, ...), so its weights load with strict=True. A ghost module runs as two launches: the main
    1x1 convolution (MFMA) and ONE launch for the cheap depthwise 3x3, the channel concatenation and - for the unit's last module -
    the skip add (pcv_ghost_dw_fused, csrc/ghost.hpp); the concatenation offset Cm (12, 20, 36, 60, 92, 100, ...) need not be a
    multiple of 8. Between them: the strided depthwise 3x3 / 5x5, SE with a clamp(x, 0, 1) gate through the three SE launches, the
    depthwise-separable `identity_conv` through the fused inverted-residual launch; the classifier is two 1x1 GEMMs with fp32 logits.
"""

__all__ = ['GhostNet', 'ghostnet', 'GhostHSigmoid', 'GhostConvBlock', 'GhostExpBlock', 'GhostUnit', 'GhostClassifier', 'get_ghostnet']

import math
import torch
import torch.nn as nn
from .common.activ import lambda_relu
from .common.conv import conv1x1, conv1x1_block, conv3x3_block, dwconv3x3_block, dwconv5x5_block, dwsconv3x3_block
from .common.att import round_channels, SEBlock
from .resnet import SkipUnit
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class GhostHSigmoid(nn.Module):
    """clamp(x, 0, 1), the gate activation of GhostNet's SE blocks (reference ghostnet.py:18-24). On the hot path it is the
    activation code PCV_ACT_CLAMP01 of the excitation launch (engine.act_code); called on a tensor it is the clamp itself."""
    def forward(self, x):
        return torch.clamp(x, min=0.0, max=1.0)


class GhostConvBlock(nn.Module):
    """Ghost module (reference ghostnet.py:27-60): `main_conv` 1x1 to half the channels, `cheap_conv` depthwise 3x3 on them, the two
    concatenated. `forward(x, residual=None)` also takes the unit's skip tensor: the concatenation and the add ride in the cheap
    convolution's launch."""
    def __init__(self, in_channels, out_channels, activation=lambda_relu()):
        super(GhostConvBlock, self).__init__()
        main_out_channels = math.ceil(0.5 * out_channels)
        cheap_out_channels = out_channels - main_out_channels
        self.main_conv = conv1x1_block(in_channels=in_channels, out_channels=main_out_channels, activation=activation)
        self.cheap_conv = dwconv3x3_block(in_channels=main_out_channels, out_channels=cheap_out_channels, activation=activation)

    def _run(self, a, residual):
        cheap = self.cheap_conv
        return engine.ghost_dw(cheap.runner(), self.main_conv(a), cheap.act_code(), residual)

    def forward(self, x, residual=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual))


class GhostExpBlock(nn.Module):
    """Body of a unit (reference ghostnet.py:63-121): expanding ghost module, strided depthwise convolution (stride 2 only), SE with the
    clamp gate, projecting ghost module without activation. `forward(x, residual=None)` hands the skip tensor to `pw_conv`."""
    def __init__(self, in_channels, out_channels, stride, use_kernel3, exp_factor, use_se):
        super(GhostExpBlock, self).__init__()
        self.use_dw_conv = (stride != 1)
        self.use_se = use_se
        mid_channels = int(math.ceil(exp_factor * in_channels))
        self.exp_conv = GhostConvBlock(in_channels=in_channels, out_channels=mid_channels)
        if self.use_dw_conv:
            dw_block = dwconv3x3_block if use_kernel3 else dwconv5x5_block
            self.dw_conv = dw_block(in_channels=mid_channels, out_channels=mid_channels, stride=stride, activation=None)
        if self.use_se:
            self.se = SEBlock(channels=mid_channels, reduction=4, out_activation=GhostHSigmoid())
        self.pw_conv = GhostConvBlock(in_channels=mid_channels, out_channels=out_channels, activation=None)

    def _run(self, a, residual):
        y = self.exp_conv(a)
        if self.use_dw_conv:
            y = self.dw_conv(y)
        if self.use_se:
            y = self.se(y)
        return self.pw_conv(y, residual=residual)

    def forward(self, x, residual=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual))


class GhostUnit(SkipUnit):
    """GhostNet unit (reference ghostnet.py:124-174): body + identity, the identity a depthwise-separable 3x3 block where the shape
    changes. The add is the epilogue of the body's last launch; there is no activation behind it."""
    def __init__(self, in_channels, out_channels, stride, use_kernel3, exp_factor, use_se):
        super(GhostUnit, self).__init__()
        self.body = GhostExpBlock(in_channels=in_channels, out_channels=out_channels, stride=stride, use_kernel3=use_kernel3,
                                  exp_factor=exp_factor, use_se=use_se)
        self.add_skip(in_channels, out_channels, stride, block=dwsconv3x3_block, activation=None, pw_activation=None)

    def _run(self, a):
        return self.body(a, residual=self._identity(a))


class GhostClassifier(nn.Module):
    """conv1x1 + BN + ReLU -> conv1x1 with bias (reference ghostnet.py:177-206): two 1x1 GEMMs on the pooled map, fp32 logits."""
    def __init__(self, in_channels, out_channels, mid_channels):
        super(GhostClassifier, self).__init__()
        self.conv1 = conv1x1_block(in_channels=in_channels, out_channels=mid_channels)
        self.conv2 = conv1x1(in_channels=mid_channels, out_channels=out_channels, bias=True)

    def _run(self, a):
        return self.conv2(self.conv1(a), out_fp32=True)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class GhostNet(ClassifierNet):
    """`features` (init_block, stage1..5 of unit1..n, final_block, final_pool) + `output` classifier (reference ghostnet.py:209-302)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, final_block_channels, classifier_mid_channels, kernels3, exp_factors, use_se,
                 first_stride, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(GhostNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", conv3x3_block(in_channels=in_channels, out_channels=init_block_channels, stride=2))
        width = add_stages(
            self.features, init_block_channels, channels, downsample_first=first_stride,
            make_unit=lambda cin, cout, stride, i, j: GhostUnit(
                in_channels=cin, out_channels=cout, stride=stride, use_kernel3=(kernels3[i][j] == 1),
                exp_factor=exp_factors[i][j], use_se=(use_se[i][j] == 1)))
        self.features.add_module("final_block", conv1x1_block(in_channels=width, out_channels=final_block_channels))
        self.finish(final_block_channels, head=GhostClassifier(in_channels=final_block_channels, out_channels=num_classes,
                                                               mid_channels=classifier_mid_channels))

    def _head(self, a):
        if a.H != 1 or a.W != 1:
            raise RuntimeError("classifier expects a 1x1 pooled map, got {}x{}".format(a.H, a.W))
        y = self.output(a)
        return y.t.view(y.N, -1)


def get_ghostnet(width_scale=1.0, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    """GhostNet with the reference's tables (ghostnet.py:329-353). A `width_scale` that gives a ghost module a half width that is
    no multiple of 4 builds, and raises NotImplementedError at the first forward."""
    init_block_channels = 16
    channels = [[16], [24, 24], [40, 40], [80, 80, 80, 80, 112, 112], [160, 160, 160, 160, 160]]
    kernels3 = [[1], [1, 1], [0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0]]
    exp_factors = [[1], [3, 3], [3, 3], [6, 2.5, 2.3, 2.3, 6, 6], [6, 6, 6, 6, 6]]
    use_se = [[0], [0, 0], [1, 1], [0, 0, 0, 0, 1, 1], [1, 0, 1, 0, 1]]
    final_block_channels = 960
    if width_scale != 1.0:
        channels = [[round_channels(cij * width_scale, divisor=4) for cij in ci] for ci in channels]
        init_block_channels = round_channels(init_block_channels * width_scale, divisor=4)
        if width_scale > 1.0:
            final_block_channels = round_channels(final_block_channels * width_scale, divisor=4)
    net = GhostNet(channels=channels, init_block_channels=init_block_channels, final_block_channels=final_block_channels,
                   classifier_mid_channels=1280, kernels3=kernels3, exp_factors=exp_factors, use_se=use_se, first_stride=False,
                   **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_ghostnet, {"ghostnet": {}})       # GhostNet 1.0x (reference ghostnet.py:367-385)
