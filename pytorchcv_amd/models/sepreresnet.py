"""
    SE-PreResNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/sepreresnet.py:17-560): PreResNet bodies
    with an SEBlock between the body and the skip add: in the bottleneck nets it runs inside the body's last 1x1 convolution
    (SEBlock.run_behind / PreConvBlock.conv_then(se=...)), in the basic-block nets the channel scale and the add are one pass (pcv_se_scale).
"""

__all__ = ['SEPreResNet', 'sepreresnet10', 'sepreresnet12', 'sepreresnet14', 'sepreresnet16', 'sepreresnet18',
           'sepreresnet26', 'sepreresnetbc26b', 'sepreresnet34', 'sepreresnetbc38b', 'sepreresnet50', 'sepreresnet50b',
           'sepreresnet101', 'sepreresnet101b', 'sepreresnet152', 'sepreresnet152b', 'sepreresnet200',
           'sepreresnet200b', 'SEPreResUnit', 'get_sepreresnet']

from .common.conv import conv1x1
from .common.att import SEBlock
from .resnet import SkipUnit, resnet_channels, RESNET_DEPTHS
from .preresnet import PreResBlock, PreResBottleneck, PreResUnit, PreResNet
from ._build import register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT


class SEPreResUnit(SkipUnit):
    """reference sepreresnet.py:17-71: body -> SE -> + identity (identity_conv reads the pre-activated input)."""
    def __init__(self, in_channels, out_channels, stride, bottleneck, conv1_stride):
        super(SEPreResUnit, self).__init__()
        if bottleneck:
            self.body = PreResBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride,
                                         conv1_stride=conv1_stride)
        else:
            self.body = PreResBlock(in_channels=in_channels, out_channels=out_channels, stride=stride)
        self.se = SEBlock(channels=out_channels)
        self.add_skip(in_channels, out_channels, stride, block=conv1x1, activation=None)

    def _run(self, a):
        return PreResUnit._run(self, a, se=self.se)


class SEPreResNet(PreResNet):
    unit = SEPreResUnit


def get_sepreresnet(blocks, bottleneck=None, conv1_stride=True, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    if bottleneck is None:
        bottleneck = (blocks >= 50)
    net = SEPreResNet(channels=resnet_channels(blocks, bottleneck, "SE-PreResNet", RESNET_DEPTHS + (269,)), init_block_channels=64,
                      bottleneck=bottleneck, conv1_stride=conv1_stride, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


# name -> get_sepreresnet arguments (reference sepreresnet.py:239-560)
_B = dict(conv1_stride=False)
_BC = dict(bottleneck=True, conv1_stride=False)
register_variants(__name__, get_sepreresnet, {
    "sepreresnet10": dict(blocks=10), "sepreresnet12": dict(blocks=12), "sepreresnet14": dict(blocks=14),
    "sepreresnet16": dict(blocks=16), "sepreresnet18": dict(blocks=18), "sepreresnet26": dict(blocks=26, bottleneck=False),
    "sepreresnetbc26b": dict(blocks=26, **_BC), "sepreresnet34": dict(blocks=34), "sepreresnetbc38b": dict(blocks=38, **_BC),
    "sepreresnet50": dict(blocks=50), "sepreresnet50b": dict(blocks=50, **_B), "sepreresnet101": dict(blocks=101),
    "sepreresnet101b": dict(blocks=101, **_B), "sepreresnet152": dict(blocks=152), "sepreresnet152b": dict(blocks=152, **_B),
    "sepreresnet200": dict(blocks=200), "sepreresnet200b": dict(blocks=200, **_B)})
