"""
    ResNet for ImageNet-1K on the MI355X hot path. Module tree, attribute names and factory signatures follow the reference
    (pytorchcv/models/resnet.py:19-442) so its state_dicts load strictly; every unit is executed as fused launches:
    a bottleneck unit = 3 (or 4 with `identity_conv`) kernels, the residual add + ReLU living in the last one's epilogue.
"""

__all__ = ['ResNet', 'resnet10', 'resnet12', 'resnet14', 'resnetbc14b', 'resnet16', 'resnet18', 'resnet26', 'resnetbc26b',
           'resnet34', 'resnetbc38b', 'resnet50', 'resnet50b', 'resnet101', 'resnet101b', 'resnet152', 'resnet152b',
           'ResBlock', 'ResBottleneck', 'SkipUnit', 'ResUnit', 'ResStage', 'ResInitBlock', 'get_resnet']

import torch.nn as nn
from .common.activ import lambda_relu
from .common.norm import lambda_batchnorm2d
from .common.conv import conv1x1_block, conv3x3_block, conv7x7_block, conv_block_pair, conv_block_maxpool, conv_block_bottleneck
from ._build import ClassifierNet, add_stages, register_variants, stage_table
from ._tail import MaxPool2dNHWC, maybe_load_pretrained, DEFAULT_ROOT
from .. import engine


class ResBlock(nn.Module):
    """Two 3x3 blocks (reference resnet.py:19-66); `residual`/`post_act` ride on the second one."""
    def __init__(self, in_channels, out_channels, stride, bias=False, normalization=lambda_batchnorm2d(),
                 activation=lambda_relu(), final_activation=None):
        super(ResBlock, self).__init__()
        self.conv1 = conv3x3_block(in_channels=in_channels, out_channels=out_channels, stride=stride, bias=bias,
                                   normalization=normalization, activation=activation)
        self.conv2 = conv3x3_block(in_channels=out_channels, out_channels=out_channels, bias=bias,
                                   normalization=normalization, activation=final_activation)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self.conv2(self.conv1(a), residual=residual, post_act=post_act))


class ResBottleneck(nn.Module):
    """1x1 -> 3x3 -> 1x1 (reference resnet.py:69-140); the stride sits on conv1 when `conv1_stride`."""
    def __init__(self, in_channels, out_channels, stride, padding=1, dilation=1, bias=False,
                 normalization=lambda_batchnorm2d(), conv1_stride=False, bottleneck_factor=4, activation=lambda_relu(),
                 final_activation=None):
        super(ResBottleneck, self).__init__()
        mid_channels = out_channels // bottleneck_factor
        self.conv1 = conv1x1_block(in_channels=in_channels, out_channels=mid_channels, stride=(stride if conv1_stride else 1),
                                   bias=bias, normalization=normalization, activation=activation)
        self.conv2 = conv3x3_block(in_channels=mid_channels, out_channels=mid_channels,
                                   stride=(1 if conv1_stride else stride), padding=padding, dilation=dilation, bias=bias,
                                   normalization=normalization, activation=activation)
        self.conv3 = conv1x1_block(in_channels=mid_channels, out_channels=out_channels, bias=bias,
                                   normalization=normalization, activation=final_activation)

    def forward(self, x, residual=None, post_act=None):
        return engine.boundary(self, x, lambda a: self.conv3(self.conv2(self.conv1(a)), residual=residual, post_act=post_act))


class SkipUnit(nn.Module):
    """Base of the residual units: owns `resize_identity`, the skip-path block `identity_conv` (present only where the unit
    changes the shape), the activation `activ` behind the add, `_identity(a)` and the hot-path `forward`. A subclass registers
    its children in the reference's order, which is the state_dict order: `body` and whatever the reference has in front of
    the skip block (`se`), then `self.add_skip(...)`, then what it has behind it (`cbam`); it writes `_run(a)`."""
    pcv_chainable = False        # True: ResStage hands `run_chained` the first convolution's output and fuses the last one forward

    def add_skip(self, in_channels, out_channels, stride, block=conv1x1_block, activation=lambda_relu(), name="identity_conv",
                 **block_args):
        """`block(in_channels, out_channels, stride, **block_args)` as `name` where the shape changes, then `activ` (None: the
        unit has none, or places it itself). The default block is the reference's 1x1 convolution + BN without activation."""
        self.resize_identity = (in_channels != out_channels) or (stride != 1)
        if self.resize_identity:
            if block is conv1x1_block:
                block_args["activation"] = None
            self.add_module(name, block(in_channels=in_channels, out_channels=out_channels, stride=stride, **block_args))
        if activation is not None:
            self.activ = activation()

    def _identity(self, a):
        return self.identity_conv(a) if self.resize_identity else a

    def _run(self, a):
        return self.body(a, residual=self._identity(a), post_act=self.activ)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class ResUnit(SkipUnit):
    """relu(body(x) + identity) (reference resnet.py:143-229)."""
    def __init__(self, in_channels, out_channels, stride=1, padding=1, dilation=1, bias=False,
                 normalization=lambda_batchnorm2d(), bottleneck=True, conv1_stride=False, activation=lambda_relu(),
                 final_body_activation=None, final_activation=lambda_relu()):
        super(ResUnit, self).__init__()
        if bottleneck:
            self.body = ResBottleneck(in_channels=in_channels, out_channels=out_channels, stride=stride, padding=padding,
                                      dilation=dilation, bias=bias, normalization=normalization, conv1_stride=conv1_stride,
                                      activation=activation, final_activation=final_body_activation)
        else:
            self.body = ResBlock(in_channels=in_channels, out_channels=out_channels, stride=stride, bias=bias,
                                 normalization=normalization, activation=activation, final_activation=final_body_activation)
        self.add_skip(in_channels, out_channels, stride, activation=final_activation, bias=bias, normalization=normalization)
        self.pcv_chainable = bool(bottleneck)        # ResStage chains the bottleneck units only

    def run_chained(self, a, conv1_out=None, next_unit=None):
        """Stage-level execution of a bottleneck unit: `conv1_out` is this unit's first convolution when the previous unit
        already produced it; with `next_unit`, the last convolution (+ skip add + ReLU) and the next unit's first
        convolution go out as one launch whenever the pair is covered. Returns (unit output, next unit's conv1 output
        or None). A unit the fused bottleneck kernel covers (stage 1) runs as that one launch instead and hands nothing on."""
        body = self.body
        fused = conv_block_bottleneck(body.conv1, body.conv2, body.conv3, a, self.activ,
                                      id_block=self.identity_conv if self.resize_identity else None)
        if fused is not None:
            return fused, None
        if next_unit is not None and isinstance(next_unit, ResUnit) and self._stride1() and next_unit.fuses_whole(a):
            next_unit = None        # the next unit computes its own first convolution inside its launch: do not ask the pair for it
        y = body.conv2(conv1_out if conv1_out is not None else body.conv1(a))
        if next_unit is not None and self.resize_identity:
            # the skip convolution recomputed inside the fused pair (no launch, no 4x wider tensor written and re-read)
            pair = conv_block_pair(body.conv3, y, None, self.activ, next_unit.body.conv1, id_block=self.identity_conv, x0=a)
            if pair is not None:
                return pair
        identity = self._identity(a)
        if next_unit is not None:
            pair = conv_block_pair(body.conv3, y, identity, self.activ, next_unit.body.conv1)
            if pair is not None:
                return pair
        return body.conv3(y, residual=identity, post_act=self.activ), None

    def _stride1(self):
        return all(tuple(b.conv.stride) == (1, 1) for b in (self.body.conv1, self.body.conv2, self.body.conv3))

    def fuses_whole(self, a_prev):
        """Whether this unit will run as the fused bottleneck launch when it follows, at stride 1, a unit whose input is `a_prev`."""
        if not isinstance(self.body, ResBottleneck) or not isinstance(a_prev, engine.NHWC):
            return False
        body = self.body
        x = engine.ShapeOnly(a_prev.N, a_prev.H, a_prev.W, body.conv1.conv.in_channels, a_prev.dtype)
        return conv_block_bottleneck(body.conv1, body.conv2, body.conv3, x, self.activ,
                                     id_block=self.identity_conv if self.resize_identity else None, probe=True)


class ResStage(nn.Sequential):
    """A stage of units (plain nn.Sequential in the reference, resnet.py:297-313; same child names, same state_dict). On
    the hot path consecutive bottleneck units are chained so that a unit's last 1x1 convolution and the next unit's
    first one can share a launch."""
    def forward(self, x):
        units = list(self.children())
        chainable = all(getattr(u, "pcv_chainable", False) for u in units)
        if not isinstance(x, engine.NHWC) or not chainable:
            return super(ResStage, self).forward(x)
        conv1_out = None
        for i, unit in enumerate(units):
            x, conv1_out = unit.run_chained(x, conv1_out, units[i + 1] if i + 1 < len(units) else None)
        return x


class ResInitBlock(nn.Module):
    """7x7/2 stem + 3x3/2 max-pool (reference resnet.py:232-263)."""
    def __init__(self, in_channels, out_channels, normalization=lambda_batchnorm2d()):
        super(ResInitBlock, self).__init__()
        self.conv = conv7x7_block(in_channels=in_channels, out_channels=out_channels, stride=2, normalization=normalization)
        self.pool = MaxPool2dNHWC(kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        return engine.boundary(self, x, lambda a: conv_block_maxpool(self.conv, a, self.pool), stem=True)


class ResNet(ClassifierNet):
    """`features` (init_block, stage1..4 of unit1..n, final_pool) + `output` Linear (reference resnet.py:266-337)."""
    def __init__(self, channels, init_block_channels, bottleneck, conv1_stride, in_channels=3, in_size=(224, 224),
                 num_classes=1000):
        super(ResNet, self).__init__(in_size, num_classes)
        self.features.add_module("init_block", ResInitBlock(in_channels=in_channels, out_channels=init_block_channels))
        self.finish(add_stages(
            self.features, init_block_channels, channels, container=ResStage,
            make_unit=lambda cin, cout, stride, i, j: ResUnit(in_channels=cin, out_channels=cout, stride=stride,
                                                              bottleneck=bottleneck, conv1_stride=conv1_stride)))


# The one depth table of the ResNet-shaped families (reference resnet.py:373-411; 269 is PreResNet's / ResNeSt's). Depths 14, 26
# and 38 depend on the block type, see resnet_layers.
_LAYERS = {10: [1, 1, 1, 1], 12: [2, 1, 1, 1], 16: [2, 2, 2, 1], 18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3],
           101: [3, 4, 23, 3], 152: [3, 8, 36, 3], 200: [3, 24, 36, 3], 269: [3, 30, 48, 8]}
RESNET_DEPTHS = (10, 12, 14, 16, 18, 26, 34, 38, 50, 101, 152, 200)


def resnet_layers(blocks, bottleneck, what="ResNet", depths=RESNET_DEPTHS):
    """Units per stage for a depth; `depths` are the ones the family `what` has (every reference table is a subset of this one)."""
    if blocks not in depths:
        layers = None
    elif blocks == 14:
        layers = [1, 1, 1, 1] if bottleneck else [2, 2, 1, 1]
    elif blocks == 26:
        layers = [2, 2, 2, 2] if bottleneck else [3, 3, 3, 3]
    elif blocks == 38:
        layers = [3, 3, 3, 3] if bottleneck else None
    else:
        layers = _LAYERS[blocks]
    if layers is None:
        raise ValueError("Unsupported {} with number of blocks: {}".format(what, blocks))
    assert (sum(layers) * (3 if bottleneck else 2) + 2 == blocks)
    return layers


def resnet_channels(blocks, bottleneck, what="ResNet", depths=RESNET_DEPTHS, width_scale=1.0):
    """The stage table of a depth: 64 .. 512 channels (x4 with bottlenecks); `width_scale` spares the very last unit."""
    table = stage_table([w * (4 if bottleneck else 1) for w in (64, 128, 256, 512)], resnet_layers(blocks, bottleneck, what, depths))
    if width_scale != 1.0:
        table = [[int(c * width_scale) for c in stage] for stage in table]
        table[-1][-1] = 512 * (4 if bottleneck else 1)
    return table


def get_resnet(blocks, bottleneck=None, conv1_stride=True, width_scale=1.0, model_name=None, pretrained=False,
               root=DEFAULT_ROOT, **kwargs):
    if bottleneck is None:
        bottleneck = (blocks >= 50)
    net = ResNet(channels=resnet_channels(blocks, bottleneck, width_scale=width_scale),
                 init_block_channels=(64 if width_scale == 1.0 else int(64 * width_scale)), bottleneck=bottleneck,
                 conv1_stride=conv1_stride, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


_B = dict(conv1_stride=False)                    # the "b" nets: stride on the 3x3
_BC = dict(bottleneck=True, conv1_stride=False)  # the "bc..b" nets: bottlenecks at a basic-block depth
register_variants(__name__, get_resnet, {
    "resnet10": dict(blocks=10), "resnet12": dict(blocks=12), "resnet14": dict(blocks=14), "resnetbc14b": dict(blocks=14, **_BC),
    "resnet16": dict(blocks=16), "resnet18": dict(blocks=18), "resnet26": dict(blocks=26, bottleneck=False),
    "resnetbc26b": dict(blocks=26, **_BC), "resnet34": dict(blocks=34), "resnetbc38b": dict(blocks=38, **_BC),
    "resnet50": dict(blocks=50), "resnet50b": dict(blocks=50, **_B), "resnet101": dict(blocks=101),
    "resnet101b": dict(blocks=101, **_B), "resnet152": dict(blocks=152), "resnet152b": dict(blocks=152, **_B)})
