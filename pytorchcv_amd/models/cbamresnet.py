"""
    CBAM-ResNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/cbamresnet.py:15-435). Module tree, attribute
    names and factory signatures follow the reference so its state_dicts load strictly. A unit is the ResNet body (ResBlock /
    ResBottleneck with the stride on conv2, run without its skip add) followed by the CBAM block as four launches (channel pools,
    fp32 MLP, spatial pools of the channel-gated map, 7x7 spatial gate + both multiplications); the unit's skip add and ReLU ride in
    the last one, so the block reads the body's output three times and writes the unit's output once.
"""

__all__ = ['CbamResNet', 'cbam_resnet18', 'cbam_resnet34', 'cbam_resnet50', 'cbam_resnet101', 'cbam_resnet152', 'MLP', 'ChannelGate',
           'SpatialGate', 'CbamBlock', 'CbamResUnit', 'get_resnet']

import torch
import torch.nn as nn
from .common.conv import conv7x7_block
from .common.att import fold_bn_into_fc, _FoldedMlp
from .resnet import SkipUnit, ResInitBlock, ResBlock, ResBottleneck, resnet_channels
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class MLP(nn.Module):
    """fc1 -> ReLU -> fc2 on [N, C] (reference cbamresnet.py:15-45); inside a ChannelGate it runs on both pooled rows at once
    (pcv_cbam_excite). Called on its own with an fp32 device tensor [N, C(, 1, 1)] it is the two layers of pcv_se_excite."""
    def __init__(self, channels, reduction_ratio=16):
        super(MLP, self).__init__()
        mid_channels = channels // reduction_ratio
        self.fc1 = nn.Linear(in_features=channels, out_features=mid_channels)
        self.activ = nn.ReLU(inplace=True)
        self.fc2 = nn.Linear(in_features=mid_channels, out_features=channels)

    def weights(self):
        """fp32 (w1 [M, C], b1 [M], w2 [C, M], b2 [C]) as the excite launch reads them."""
        return tuple(t.detach().float().contiguous() for t in (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias))

    def forward(self, x):
        x = x.reshape(x.size(0), -1).float().contiguous()
        w1, b1, w2, b2 = self.weights()
        if x.shape[1] != w1.shape[1]:
            raise RuntimeError("MLP expects {} features, got {}".format(w1.shape[1], x.shape[1]))
        return engine.se_excite(x, w1, b1, w2, b2, engine.act_code(self.activ), 0)


class ChannelGate(nn.Module):
    """x * sigmoid(mlp(avg_pool(x)) + mlp(max_pool(x))) (reference cbamresnet.py:48-80). The fp32 [N, C] factor takes two launches
    (pcv_cbam_pool, pcv_cbam_excite); on its own the block multiplies by it in a third (pcv_se_scale), inside a CbamBlock the product
    is never stored."""
    def __init__(self, channels, reduction_ratio=16):
        super(ChannelGate, self).__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(output_size=(1, 1))      # markers only; pcv_cbam_pool computes both
        self.max_pool = nn.AdaptiveMaxPool2d(output_size=(1, 1))
        self.mlp = MLP(channels=channels, reduction_ratio=reduction_ratio)
        self.sigmoid = nn.Sigmoid()

    def _run(self, a):
        return engine.se_scale(a, engine.cbam_channel_gate(a, *self.mlp.weights()))

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class SpatialGate(nn.Module):
    """x * sigmoid(bn(conv7x7(cat(max_c x, mean_c x)))) (reference cbamresnet.py:83-102). `conv` is a ConvBlock for its parameters
    only (`conv.conv.weight` [1, 2, 7, 7], `conv.bn`): the 2 -> 1 convolution on a 25 KB map is a stencil inside pcv_cbam_apply."""
    def __init__(self):
        super(SpatialGate, self).__init__()
        self.conv = conv7x7_block(in_channels=2, out_channels=1, activation=None)
        self.sigmoid = nn.Sigmoid()
        self._pcv_stencil = _FoldedMlp()

    def stencil(self):
        """fp32 (w7 [2, 7, 7], scale [1], shift [1]) on the parameters' device: the taps and the folded BatchNorm (+ bias) behind
        them, re-derived whenever a source parameter changes."""
        c, bn = self.conv.conv, (self.conv.bn if self.conv.normalize else None)
        srcs = [c.weight, c.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])

        def build():
            # fold_bn_into_fc on a unit "weight" gives the affine map behind the convolution: scale = g / sqrt(var + eps), and the
            # shift with the convolution's bias folded in
            one = torch.ones((1, 1), dtype=torch.float32, device=c.weight.device)
            scale, shift = fold_bn_into_fc(one, c.bias, bn)
            return c.weight.detach().float().reshape(2, 7, 7).contiguous(), scale.reshape(1).contiguous(), shift.reshape(1).contiguous()
        return self._pcv_stencil.get(srcs, build)

    def _run(self, a):
        return engine.cbam_spatial(a, None, *self.stencil())

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class CbamBlock(nn.Module):
    """ChannelGate then SpatialGate (reference cbamresnet.py:105-128) as engine.cbam_forward's four launches. `forward(x, residual=
    None, post_act=None)` also takes the unit's skip tensor and the activation after the add: they ride in the last launch."""
    def __init__(self, channels, reduction_ratio=16):
        super(CbamBlock, self).__init__()
        self.ch_gate = ChannelGate(channels=channels, reduction_ratio=reduction_ratio)
        self.sp_gate = SpatialGate()

    def _run(self, a, residual=None, post_act=None):
        w1, b1, w2, b2 = self.ch_gate.mlp.weights()
        w7, scale, shift = self.sp_gate.stencil()
        return engine.cbam_forward(a, w1, b1, w2, b2, w7, scale, shift, residual, engine.act_code(post_act))

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self._run(a, residual, post_act))


class CbamResUnit(SkipUnit):
    """relu(cbam(body(x)) + identity) (reference cbamresnet.py:131-183)."""
    def __init__(self, in_channels, out_channels, stride, bottleneck):
        super(CbamResUnit, self).__init__()
        if bottleneck:
            self.body = ResBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride, conv1_stride=False)
        else:
            self.body = ResBlock(in_channels=in_channels, out_channels=out_channels, stride=stride)
        self.add_skip(in_channels, out_channels, stride, activation=None)
        self.cbam = CbamBlock(channels=out_channels)          # the reference has it between the skip block and the activation
        self.activ = nn.ReLU(inplace=True)

    def _run(self, a):
        identity = self._identity(a)
        return self.cbam(self.body(a), residual=identity, post_act=self.activ)      # the body without its own skip add


class CbamResNet(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` Linear (reference cbamresnet.py:186-253)."""
    def __init__(self, channels, init_block_channels, bottleneck, in_channels=3, in_size=(224, 224), num_classes=1000):
        super(CbamResNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        self.finish(add_stages(
            self.features, init_block_channels, channels,
            make_unit=lambda cin, cout, stride, i, j: CbamResUnit(in_channels=cin, out_channels=cout, stride=stride,
                                                                  bottleneck=bottleneck)))


def get_resnet(blocks, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    """CBAM-ResNet of a depth (the reference's factory and its name, cbamresnet.py:256-325)."""
    bottleneck = blocks >= 50
    net = CbamResNet(channels=resnet_channels(blocks, bottleneck, what="CBAM-ResNet", depths=(18, 34, 50, 101, 152)),
                     init_block_channels=64, bottleneck=bottleneck, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_resnet, {"cbam_resnet{}".format(n): dict(blocks=n) for n in (18, 34, 50, 101, 152)})
