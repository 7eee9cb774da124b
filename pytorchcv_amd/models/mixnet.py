"""
    MixNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/mixnet.py:18-573). Module tree, attribute names and
    state_dict keys are the reference's (`...conv1.conv.0.weight`, `...conv1.conv.1.weight`, `...exp_conv.conv.0.weight`, ...), so its
    weights load with strict=True. A unit runs as: expand (plain or 2-group 1x1) -> depthwise MixConv (ONE launch for all window
    sizes, pcv_mixconv2d_fused) or plain depthwise 3x3 -> SE through the three SE launches -> project (plain or 2-group 1x1) with
    the skip add in its epilogue. The 1x1 MixConv splits its channels evenly, which makes it exactly Conv2d(groups=kernel_count)
    with the groups' weights concatenated along dim 0: it runs on pcv_conv2d_fused's grouped path.
"""

__all__ = ['MixNet', 'mixnet_s', 'mixnet_m', 'mixnet_l', 'MixConv', 'MixConvBlock', 'mixconv1x1_block', 'MixUnit', 'MixInitBlock',
           'get_mixnet']

import torch
import torch.nn as nn
from .common.activ import lambda_relu, lambda_swish, create_activation_layer
from .common.norm import lambda_batchnorm2d, create_normalization_layer
from .common.conv import conv1x1_block, conv3x3_block, dwconv3x3_block, mbconv_chain
from .common.att import round_channels, SEBlock
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class _GroupedView(object):
    """The pointwise convolutions of a MixConv seen as ONE Conv2d(groups=G) for engine.ConvRunner: weight = the groups' weights
    concatenated along dim 0 (rebuilt when a source changes, so the runner's cache key follows load_state_dict / .to())."""
    def __init__(self, convs):
        self._convs = list(convs)
        c0 = self._convs[0]
        if any((c.in_channels, c.out_channels) != (c0.in_channels, c0.out_channels) for c in self._convs):
            raise NotImplementedError("1x1 MixConv with unequal channel splits ({}) has no grouped-convolution form on the MI355X "
                                      "path".format([(c.in_channels, c.out_channels) for c in self._convs]))
        self.groups = len(self._convs)
        self.in_channels, self.out_channels = c0.in_channels * self.groups, c0.out_channels * self.groups
        self.kernel_size, self.stride, self.padding, self.dilation = c0.kernel_size, c0.stride, c0.padding, c0.dilation
        self.padding_mode = c0.padding_mode
        self._key = self._w = self._b = None

    def _refresh(self):
        key = engine.source_key([c.weight for c in self._convs] + [c.bias for c in self._convs])
        if key != self._key:
            self._w = torch.cat([c.weight.detach() for c in self._convs], dim=0)
            self._b = torch.cat([c.bias.detach() for c in self._convs], dim=0) if self._convs[0].bias is not None else None
            self._key = key

    @property
    def weight(self):
        self._refresh()
        return self._w

    @property
    def bias(self):
        self._refresh()
        return self._b


class MixConv(nn.Module):
    """Mixed convolution layer (reference mixnet.py:18-86): children "0", "1", ... are the groups' nn.Conv2d parameter holders. They
    never run: `MixConvBlock` issues the fused launch."""
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False, axis=1):
        super(MixConv, self).__init__()
        kernel_size = kernel_size if isinstance(kernel_size, list) else [kernel_size]
        padding = padding if isinstance(padding, list) else [padding]
        kernel_count = len(kernel_size)
        self.splitted_in_channels = self.split_channels(in_channels, kernel_count)
        splitted_out_channels = self.split_channels(out_channels, kernel_count)
        for i, kernel_size_i in enumerate(kernel_size):
            in_channels_i = self.splitted_in_channels[i]
            out_channels_i = splitted_out_channels[i]
            self.add_module(name=str(i), module=nn.Conv2d(
                in_channels=in_channels_i, out_channels=out_channels_i, kernel_size=kernel_size_i, stride=stride,
                padding=padding[i], dilation=dilation, groups=(out_channels_i if out_channels == groups else groups), bias=bias))
        self.axis = axis
        self.depthwise = (out_channels == groups) and (in_channels == out_channels)
        if axis != 1:
            raise NotImplementedError("MixConv along axis {}".format(axis))

    def convs(self):
        return list(self._modules.values())

    def forward(self, x):
        raise RuntimeError("MixConv runs inside MixConvBlock's fused launch on MI355X and cannot be called on its own")

    @staticmethod
    def split_channels(channels, kernel_count):
        splitted_channels = [channels // kernel_count] * kernel_count
        splitted_channels[0] += channels - sum(splitted_channels)
        return splitted_channels


class MixConvBlock(nn.Module):
    """Mixed convolution + BatchNorm + activation as one launch (reference MixConvBlock, mixnet.py:89-157). `forward(x, residual)`
    takes the unit's skip tensor for the pointwise form (the depthwise form has none: MixUnit never adds behind conv1)."""
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False,
                 normalization=lambda_batchnorm2d(), activation=lambda_relu()):
        super(MixConvBlock, self).__init__()
        self.normalize = (normalization is not None)
        self.activate = (activation is not None)
        self.conv = MixConv(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                            padding=padding, dilation=dilation, groups=groups, bias=bias)
        if self.normalize:
            self.bn = create_normalization_layer(normalization=normalization, num_features=out_channels)
            assert isinstance(self.bn, nn.Module)
        if self.activate:
            self.activ = create_activation_layer(activation)
        self._pcv_runner = None

    def _run(self, a, residual):
        bn = self.bn if self.normalize else None
        act = engine.act_code(self.activ) if self.activate else 0
        if self._pcv_runner is None:
            convs = self.conv.convs()
            if self.conv.depthwise:
                self._pcv_runner = engine.MixConvRunner(convs, bn)
            elif all(tuple(c.kernel_size) == (1, 1) and c.groups == 1 for c in convs):
                self._pcv_runner = engine.ConvRunner(_GroupedView(convs), bn)
            else:
                raise NotImplementedError("MixConv on the MI355X path is depthwise (groups == channels) or pointwise (1x1)")
        if self.conv.depthwise:
            if residual is not None:
                raise RuntimeError("the depthwise MixConv launch has no residual input")
            return self._pcv_runner.run(a, act=act)
        return self._pcv_runner.run(a, act=act, residual=residual)

    def forward(self, x, residual=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual))


def mixconv1x1_block(kernel_count, stride=1, **kwargs):
    """1x1 version of the mixed convolution block (reference mixnet.py:160-189)."""
    return MixConvBlock(kernel_size=([1] * kernel_count), stride=stride, padding=([0] * kernel_count), **kwargs)


class MixUnit(nn.Module):
    """MixNet unit (reference mixnet.py:192-293)."""
    def __init__(self, in_channels, out_channels, stride, exp_kernel_count, conv1_kernel_count, conv2_kernel_count, exp_factor,
                 se_factor, activation):
        super(MixUnit, self).__init__()
        assert (exp_factor >= 1)
        assert (se_factor >= 0)
        self.residual = (in_channels == out_channels) and (stride == 1)
        self.use_se = se_factor > 0
        mid_channels = exp_factor * in_channels
        self.use_exp_conv = exp_factor > 1
        if self.use_exp_conv:
            if exp_kernel_count == 1:
                self.exp_conv = conv1x1_block(in_channels=in_channels, out_channels=mid_channels, activation=activation)
            else:
                self.exp_conv = mixconv1x1_block(in_channels=in_channels, out_channels=mid_channels,
                                                 kernel_count=exp_kernel_count, activation=activation)
        if conv1_kernel_count == 1:
            self.conv1 = dwconv3x3_block(in_channels=mid_channels, out_channels=mid_channels, stride=stride, activation=activation)
        else:
            self.conv1 = MixConvBlock(in_channels=mid_channels, out_channels=mid_channels,
                                      kernel_size=[3 + 2 * i for i in range(conv1_kernel_count)], stride=stride,
                                      padding=[1 + i for i in range(conv1_kernel_count)], groups=mid_channels, activation=activation)
        if self.use_se:
            self.se = SEBlock(channels=mid_channels, reduction=(exp_factor * se_factor), round_mid=False, mid_activation=activation)
        if conv2_kernel_count == 1:
            self.conv2 = conv1x1_block(in_channels=mid_channels, out_channels=out_channels, activation=None)
        else:
            self.conv2 = mixconv1x1_block(in_channels=mid_channels, out_channels=out_channels, kernel_count=conv2_kernel_count,
                                          activation=None)

    def _run(self, a):
        identity = a if self.residual else None
        if not self.use_se and not isinstance(self.conv1, MixConvBlock):
            # plain expand / depthwise 3x3 / project: the fused inverted-residual launch where it covers the shapes
            y = mbconv_chain(self.exp_conv if self.use_exp_conv else None, self.conv1, self.conv2, a, residual=identity)
            if y is not None:
                return y
        y = self.exp_conv(a) if self.use_exp_conv else a
        y = self.conv1(y)
        if self.use_se:
            y = self.se(y)
        return self.conv2(y, residual=identity)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class MixInitBlock(nn.Module):
    """MixNet specific initial block (reference mixnet.py:296-329)."""
    def __init__(self, in_channels, out_channels):
        super(MixInitBlock, self).__init__()
        self.conv1 = conv3x3_block(in_channels=in_channels, out_channels=out_channels, stride=2)
        self.conv2 = MixUnit(in_channels=out_channels, out_channels=out_channels, stride=1, exp_kernel_count=1, conv1_kernel_count=1,
                             conv2_kernel_count=1, exp_factor=1, se_factor=0, activation=lambda_relu())

    def _run(self, a):
        return self.conv2(self.conv1(a))

    def forward(self, x):
        return engine.boundary(self, x, self._run, stem=True)


class MixNet(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_block, final_pool) + `output` Linear (reference mixnet.py:332-429)."""
    pcv_16bit = "fp16"      # the 16-bit mode "auto" resolves to for this family (engine.compute_dtype_of)

    def __init__(self, channels, init_block_channels, final_block_channels, exp_kernel_counts, conv1_kernel_counts,
                 conv2_kernel_counts, exp_factors, se_factors, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(MixNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", MixInitBlock(in_channels=in_channels, out_channels=init_block_channels))

        def make_unit(cin, cout, _, i, j):
            # the family's own stride rule: every stage opens with stride 2, but the fourth has it in its middle
            stride = 2 if ((j == 0) and (i != 3)) or ((j == len(channels[i]) // 2) and (i == 3)) else 1
            return MixUnit(in_channels=cin, out_channels=cout, stride=stride, exp_kernel_count=exp_kernel_counts[i][j],
                           conv1_kernel_count=conv1_kernel_counts[i][j], conv2_kernel_count=conv2_kernel_counts[i][j],
                           exp_factor=exp_factors[i][j], se_factor=se_factors[i][j],
                           activation=(lambda_relu() if i == 0 else lambda_swish()))
        width = add_stages(self.features, init_block_channels, channels, make_unit)
        self.features.add_module("final_block", conv1x1_block(in_channels=width, out_channels=final_block_channels))
        self.finish(final_block_channels)


def get_mixnet(version, width_scale, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    """MixNet with the reference's tables (mixnet.py:432-504)."""
    if version == "s":
        init_block_channels = 16
        channels = [[24, 24], [40, 40, 40, 40], [80, 80, 80], [120, 120, 120, 200, 200, 200]]
        exp_kernel_counts = [[2, 2], [1, 2, 2, 2], [1, 1, 1], [2, 2, 2, 1, 1, 1]]
        conv1_kernel_counts = [[1, 1], [3, 2, 2, 2], [3, 2, 2], [3, 4, 4, 5, 4, 4]]
        conv2_kernel_counts = [[2, 2], [1, 2, 2, 2], [2, 2, 2], [2, 2, 2, 1, 2, 2]]
        exp_factors = [[6, 3], [6, 6, 6, 6], [6, 6, 6], [6, 3, 3, 6, 6, 6]]
        se_factors = [[0, 0], [2, 2, 2, 2], [4, 4, 4], [2, 2, 2, 2, 2, 2]]
    elif version == "m":
        init_block_channels = 24
        channels = [[32, 32], [40, 40, 40, 40], [80, 80, 80, 80], [120, 120, 120, 120, 200, 200, 200, 200]]
        exp_kernel_counts = [[2, 2], [1, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2, 1, 1, 1, 1]]
        conv1_kernel_counts = [[3, 1], [4, 2, 2, 2], [3, 4, 4, 4], [1, 4, 4, 4, 4, 4, 4, 4]]
        conv2_kernel_counts = [[2, 2], [1, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2, 1, 2, 2, 2]]
        exp_factors = [[6, 3], [6, 6, 6, 6], [6, 6, 6, 6], [6, 3, 3, 3, 6, 6, 6, 6]]
        se_factors = [[0, 0], [2, 2, 2, 2], [4, 4, 4, 4], [2, 2, 2, 2, 2, 2, 2, 2]]
    else:
        raise ValueError("Unsupported MixNet version {}".format(version))
    final_block_channels = 1536
    if width_scale != 1.0:
        channels = [[round_channels(cij * width_scale) for cij in ci] for ci in channels]
        init_block_channels = round_channels(init_block_channels * width_scale)
    net = MixNet(channels=channels, init_block_channels=init_block_channels, final_block_channels=final_block_channels,
                 exp_kernel_counts=exp_kernel_counts, conv1_kernel_counts=conv1_kernel_counts,
                 conv2_kernel_counts=conv2_kernel_counts, exp_factors=exp_factors, se_factors=se_factors, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


# MixNet-S, -M and -L = MixNet-M at width 1.3 (reference mixnet.py:507-573)
register_variants(__name__, get_mixnet, {"mixnet_s": dict(version="s", width_scale=1.0), "mixnet_m": dict(version="m", width_scale=1.0),
                                         "mixnet_l": dict(version="m", width_scale=1.3)})
