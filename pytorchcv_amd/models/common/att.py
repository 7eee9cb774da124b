"""
    Squeeze-and-Excitation (reference pytorchcv/models/common/att.py:15-105): same attributes (`conv1`/`conv2` with bias, or
    `fc1`/`fc2`), three small launches on the hot path: spatial mean -> fp32 excitation MLP -> channel scale fused with the
    unit's residual add and activation.
    Split attention (att.py:108-296: SABlock, SAConvBlock, saconv3x3_block): the same three-launch shape across the radix splits
    of one convolution's output - squeeze of their sum -> fp32 MLP + softmax over the splits -> weighted sum of the splits.
"""

__all__ = ['round_channels', 'SEBlock', 'SABlock', 'SAConvBlock', 'saconv3x3_block', 'fold_bn_into_fc']

import torch
import torch.nn as nn
from .activ import lambda_relu, lambda_sigmoid, create_activation_layer
from .conv import conv1x1, ConvBlock
from .norm import lambda_batchnorm2d, create_normalization_layer
from ... import engine


def round_channels(channels, divisor=8):
    """Make-divisible rule of reference att.py:15-35."""
    rounded = max(int(channels + divisor / 2.0) // divisor * divisor, divisor)
    if float(rounded) < 0.9 * channels:
        rounded += divisor
    return rounded


class SEBlock(nn.Module):
    def __init__(self, channels, reduction=16, mid_channels=None, round_mid=False, use_conv=True,
                 mid_activation=lambda_relu(), out_activation=lambda_sigmoid()):
        super(SEBlock, self).__init__()
        self.use_conv = use_conv
        if mid_channels is None:
            mid_channels = channels // reduction if not round_mid else round_channels(float(channels) / reduction)
        self.pool = nn.AdaptiveAvgPool2d(output_size=1)      # marker only; the squeeze kernel computes it
        if use_conv:
            self.conv1 = conv1x1(in_channels=channels, out_channels=mid_channels, bias=True)
        else:
            self.fc1 = nn.Linear(in_features=channels, out_features=mid_channels)
        self.activ = create_activation_layer(mid_activation)
        if use_conv:
            self.conv2 = conv1x1(in_channels=mid_channels, out_channels=channels, bias=True)
        else:
            self.fc2 = nn.Linear(in_features=mid_channels, out_features=channels)
        self.sigmoid = create_activation_layer(out_activation)

    def _mlp(self):
        a, b = (self.conv1, self.conv2) if self.use_conv else (self.fc1, self.fc2)
        w1 = a.weight.detach().float().reshape(a.weight.shape[0], -1).contiguous()
        w2 = b.weight.detach().float().reshape(b.weight.shape[0], -1).contiguous()
        return w1, a.bias.detach().float().contiguous(), w2, b.bias.detach().float().contiguous()

    def run_behind(self, conv_block, z, residual=None, post_act=None, next_conv=None):
        """`self(conv_block(z), residual, post_act)` in ONE pass over the wide tensor when `conv_block` is a plain 1x1 ConvBlock
        without activation (the bottleneck's last convolution, seresnet.py:60-71): BN(conv(.)) is affine, so the squeeze
        mean_hw(BN(conv(z))) = BN(conv(mean_hw(z))) is taken on the narrower input z, the excitation runs BEFORE the convolution
        and the channel scale + skip add + activation ride in its epilogue (pcv_conv2d_gated_fused). Returns None when the block
        is not of that shape (the caller then runs conv_block and this module one after the other). With `next_conv` (the next
        unit's first 1x1 ConvBlock) the result may be the tuple (y, next_conv(y)) of pcv_conv1x1_pair_gated_fused."""
        from .conv import ConvBlock
        c = getattr(conv_block, "conv", None)
        if not (engine.FUSE_UNITS and isinstance(conv_block, ConvBlock) and isinstance(z, engine.NHWC) and not conv_block.activate and
                not conv_block.use_pad and c is not None and tuple(c.kernel_size) == (1, 1) and tuple(c.stride) == (1, 1) and
                tuple(c.padding) == (0, 0) and c.groups == 1 and z.dense):
            return None
        runner = conv_block.runner()
        w1, b1, w2, b2 = self._mlp()
        gate = runner.squeezed_excite(z, w1, b1, w2, b2, engine.act_code(self.activ), engine.act_code(self.sigmoid))
        if next_conv is not None and residual is not None and isinstance(next_conv, ConvBlock):
            # ... and the next unit's first 1x1 in the same launch: returns (y, next conv1 output)
            pair = runner.run_pair(z, residual, 0, engine.act_code(post_act), next_conv.runner(), next_conv.act_code(), gate=gate)
            if pair is not None:
                return pair
        return runner.run(z, act=0, residual=residual, post_act=engine.act_code(post_act), gate=gate)

    def forward(self, x, residual=None, post_act=None):
        w1, b1, w2, b2 = self._mlp()
        return engine.boundary(self, x, lambda a: engine.se_forward(
            a, w1, b1, w2, b2, engine.act_code(self.activ), engine.act_code(self.sigmoid), residual, engine.act_code(post_act)))


def fold_bn_into_fc(w, b, bn):
    """(w [M, K], b [M] or None) of a 1x1 layer followed by the eval-mode BatchNorm2d `bn` -> fp32 (w', b') of the composed affine
    map: w' = w * g / sqrt(var + eps) (per row), b' = (b - mean) * g / sqrt(var + eps) + beta."""
    w = w.detach().float().reshape(w.shape[0], -1)
    b = b.detach().float() if b is not None else torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
    if bn is None:
        return w.contiguous(), b.contiguous()
    if bn.training:
        raise RuntimeError("pytorchcv_amd is an inference path: call net.eval() first (BatchNorm is folded)")
    g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(b)
    beta = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(b)
    sc = g / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    return (w * sc[:, None]).contiguous(), ((b - bn.running_mean.detach().float()) * sc + beta).contiguous()


class _FoldedMlp(object):
    """The fp32 (w1, b1, w2, b2) of a split-attention MLP, re-derived whenever a source parameter changes (load_state_dict, .to())."""
    def __init__(self):
        self.key, self.value = None, None

    def get(self, sources, build):
        key = engine.source_key(sources)
        if key != self.key:
            self.value, self.key = build(), key
        return self.value


class SABlock(nn.Module):
    """Split-attention block (reference att.py:108-189): same constructor, same attributes (`pool`, `conv1`/`fc1`, `bn`, `activ`,
    `conv2`/`fc2`, `softmax`). `forward(x, residual=None, post_act=None)` also takes the unit's skip tensor and the activation after
    the add (ResNeSt-A's basic block ends in this block, resnesta.py:196-198): they ride in the combine launch."""
    def __init__(self, out_channels, groups, radix, reduction=4, min_channels=32, use_conv=True,
                 normalization=lambda_batchnorm2d()):
        super(SABlock, self).__init__()
        self.groups = groups
        self.radix = radix
        self.use_conv = use_conv
        in_channels = out_channels * radix
        mid_channels = max(in_channels // reduction, min_channels)
        self.pool = nn.AdaptiveAvgPool2d(output_size=1)      # marker only; the squeeze kernel computes it
        if use_conv:
            self.conv1 = conv1x1(in_channels=out_channels, out_channels=mid_channels, bias=True)
        else:
            self.fc1 = nn.Linear(in_features=out_channels, out_features=mid_channels)
        self.bn = create_normalization_layer(normalization=normalization, num_features=mid_channels)
        self.activ = nn.ReLU(inplace=True)
        if use_conv:
            self.conv2 = conv1x1(in_channels=mid_channels, out_channels=in_channels, bias=True)
        else:
            self.fc2 = nn.Linear(in_features=mid_channels, out_features=in_channels)
        self.softmax = nn.Softmax(dim=1)
        self._pcv_mlp = _FoldedMlp()

    def _mlp(self):
        a, b = (self.conv1, self.conv2) if self.use_conv else (self.fc1, self.fc2)
        srcs = [a.weight, a.bias, b.weight, b.bias, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]

        def build():
            w1, b1 = fold_bn_into_fc(a.weight, a.bias, self.bn)
            return w1, b1, b.weight.detach().float().reshape(b.weight.shape[0], -1).contiguous(), b.bias.detach().float().contiguous()
        return self._pcv_mlp.get(srcs, build)

    def _run(self, a, residual=None, post_act=None):
        w1, b1, w2, b2 = self._mlp()
        return engine.splat_forward(a, self.radix, self.groups, w1, b1, w2, b2, residual, engine.act_code(post_act))

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual, post_act))


class SAConvBlock(nn.Module):
    """Split-attention convolution block (reference att.py:192-276): a ConvBlock with `out_channels * radix` outputs in
    `groups * radix` groups (one fused launch) followed by the SABlock (three launches)."""
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, groups=1, bias=False,
                 normalization=lambda_batchnorm2d(), activation=lambda_relu(), radix=2, reduction=4, min_channels=32,
                 use_conv=True):
        super(SAConvBlock, self).__init__()
        self.conv = ConvBlock(in_channels=in_channels, out_channels=(out_channels * radix), kernel_size=kernel_size, stride=stride,
                              padding=padding, dilation=dilation, groups=(groups * radix), bias=bias, normalization=normalization,
                              activation=activation)
        self.att = SABlock(out_channels=out_channels, groups=groups, radix=radix, reduction=reduction, min_channels=min_channels,
                           use_conv=use_conv, normalization=normalization)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self.att(self.conv(a), residual=residual, post_act=post_act))


def saconv3x3_block(stride=1, padding=1, **kwargs):
    return SAConvBlock(kernel_size=3, stride=stride, padding=padding, **kwargs)
