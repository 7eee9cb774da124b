"""
    SE-ResNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/seresnet.py:17-258): ResNet bodies with an
    SEBlock between body and skip add; the channel scale, the add and the ReLU are one pass (pcv_se_scale).
"""

__all__ = ['SEResNet', 'seresnet10', 'seresnet18', 'seresnet26', 'seresnetbc26b', 'seresnetbc38b', 'seresnet50', 'seresnet50b',
           'seresnet101', 'seresnet101b', 'seresnet152', 'SEResUnit', 'get_seresnet']

from .common.att import SEBlock
from .resnet import SkipUnit, ResStage, ResBlock, ResBottleneck, ResInitBlock, resnet_channels
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT


class SEResUnit(SkipUnit):
    def __init__(self, in_channels, out_channels, stride, bottleneck, conv1_stride):
        super(SEResUnit, self).__init__()
        if bottleneck:
            self.body = ResBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride,
                                      conv1_stride=conv1_stride)
        else:
            self.body = ResBlock(in_channels=in_channels, out_channels=out_channels, stride=stride)
        self.se = SEBlock(channels=out_channels)
        self.add_skip(in_channels, out_channels, stride)

    pcv_chainable = True         # ResStage: first convolution handed in, last one (with the SE block) fused forward

    def run_chained(self, a, conv1_out=None, next_unit=None):
        """The SE units' stage-level execution (SE-ResNeXt's unit runs this very function)."""
        identity = self._identity(a)
        body = self.body
        if not hasattr(body, "conv3"):                           # basic block: the SE block follows a 3x3 (not affine in the mean)
            return self.se(body(a), residual=identity, post_act=self.activ), None
        z = body.conv2(conv1_out if conv1_out is not None else body.conv1(a))
        nxt = next_unit.body.conv1 if (next_unit is not None and hasattr(next_unit.body, "conv3")) else None
        y = self.se.run_behind(body.conv3, z, residual=identity, post_act=self.activ, next_conv=nxt)
        if y is None:
            y = self.se(body.conv3(z), residual=identity, post_act=self.activ)
        return y if isinstance(y, tuple) else (y, None)

    def _run(self, a):
        return self.run_chained(a)[0]


class SEResNet(ClassifierNet):
    def __init__(self, channels, init_block_channels, bottleneck, conv1_stride, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(SEResNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        self.finish(add_stages(
            self.features, init_block_channels, channels, container=ResStage,
            make_unit=lambda cin, cout, stride, i, j: SEResUnit(in_channels=cin, out_channels=cout, stride=stride,
                                                                bottleneck=bottleneck, conv1_stride=conv1_stride)))


def get_seresnet(blocks, bottleneck=None, conv1_stride=True, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    if bottleneck is None:
        bottleneck = (blocks >= 50)
    net = SEResNet(channels=resnet_channels(blocks, bottleneck, what="SE-ResNet"), init_block_channels=64, bottleneck=bottleneck,
                   conv1_stride=conv1_stride, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


_BC = dict(bottleneck=True, conv1_stride=False)
register_variants(__name__, get_seresnet, {
    "seresnet10": dict(blocks=10), "seresnet18": dict(blocks=18), "seresnet26": dict(blocks=26, bottleneck=False),
    "seresnetbc26b": dict(blocks=26, **_BC), "seresnetbc38b": dict(blocks=38, **_BC), "seresnet50": dict(blocks=50),
    "seresnet50b": dict(blocks=50, conv1_stride=False), "seresnet101": dict(blocks=101),
    "seresnet101b": dict(blocks=101, conv1_stride=False), "seresnet152": dict(blocks=152)})
