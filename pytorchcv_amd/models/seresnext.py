"""
    SE-ResNeXt for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/seresnext.py:17-271): ResNeXt bottleneck
    (grouped 3x3 as block-diagonal implicit GEMM) + SEBlock, with the channel scale, skip add and ReLU in one pass.
"""

__all__ = ['SEResNeXt', 'seresnext50_32x4d', 'seresnext101_32x4d', 'seresnext101_64x4d', 'SEResNeXtUnit', 'get_seresnext']

from .common.att import SEBlock
from .resnet import SkipUnit, ResStage, ResInitBlock, resnet_channels
from .resnext import ResNeXtBottleneck
from .seresnet import SEResUnit
from ._build import ClassifierNet, add_stages, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT


class SEResNeXtUnit(SkipUnit):
    def __init__(self, in_channels, out_channels, stride, cardinality, bottleneck_width):
        super(SEResNeXtUnit, self).__init__()
        self.body = ResNeXtBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride,
                                      cardinality=cardinality, bottleneck_width=bottleneck_width)
        self.se = SEBlock(channels=out_channels)
        self.add_skip(in_channels, out_channels, stride)

    pcv_chainable = True         # ResStage: first convolution handed in, last one (with the SE block) fused forward
    run_chained, _run = SEResUnit.run_chained, SEResUnit._run


class SEResNeXt(ClassifierNet):
    def __init__(self, channels, init_block_channels, cardinality, bottleneck_width, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(SEResNeXt, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        self.finish(add_stages(
            self.features, init_block_channels, channels, container=ResStage,
            make_unit=lambda cin, cout, stride, i, j: SEResNeXtUnit(in_channels=cin, out_channels=cout, stride=stride,
                                                                    cardinality=cardinality, bottleneck_width=bottleneck_width)))


def get_seresnext(blocks, cardinality, bottleneck_width, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    net = SEResNeXt(channels=resnet_channels(blocks, True, what="SE-ResNeXt", depths=(50, 101)), init_block_channels=64,
                    cardinality=cardinality, bottleneck_width=bottleneck_width, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


register_variants(__name__, get_seresnext, {
    "seresnext50_32x4d": dict(blocks=50, cardinality=32, bottleneck_width=4),
    "seresnext101_32x4d": dict(blocks=101, cardinality=32, bottleneck_width=4),
    "seresnext101_64x4d": dict(blocks=101, cardinality=64, bottleneck_width=4)})
