"""
    HRNet for ImageNet-1K on the MI355X hot path (reference pytorchcv/models/hrnet.py:17-680). Module tree, attribute names and
    state_dict keys are the reference's (`features.stage3.layers.block2.fuse_layers.layer1.block3.conv.bn.weight`,
    `features.stage2.transition.block3.subblock1.conv.weight`, `features.final_block.down_blocks.block1.conv.bias`, ...), so its
    weights load with strict=True. Branch units, transitions, down chains and the final block are fused ConvBlock launches; the
    exchange at the end of every HRBlock (hrnet.py:126-134) is ONE launch per output branch (pcv_hr_fuse, csrc/hrfuse.hpp): each
    UpSamplingBlock runs its 1x1 convolution at the coarse resolution and hands the result over with its shift, so the upsampled
    tensor never exists; down chains and the identity term are shift-0 sources. The sum keeps the reference's order j = 0 .. B-1.

    `FUSED = False` selects the composed path instead - `engine.interpolate` + `engine.add`, one launch per upsample and per add,
    partial sums rounded to the storage type like the reference's own tensors. It is also what runs where pcv_hr_fuse_supported
    refuses a shape (a map that does not divide, a scale factor that is no power of two), the baseline of tests/tools/bench_hrnet.py
    and a cross-check in tests: in fp32 both paths give the same bits. The net keeps its own trunk loop (not `add_stages`): a
    stage is one multi-branch HRStage that takes and returns a list of maps, not a sequence of units.
"""

__all__ = ['HRNet', 'hrnet_w18_small_v1', 'hrnet_w18_small_v2', 'hrnetv2_w18', 'hrnetv2_w30', 'hrnetv2_w32', 'hrnetv2_w40',
           'hrnetv2_w44', 'hrnetv2_w48', 'hrnetv2_w64', 'Identity', 'UpSamplingBlock', 'HRBlock', 'HRStage', 'HRInitBlock',
           'HRFinalBlock', 'get_hrnet']

import torch
import torch.nn as nn
from .common.conv import conv1x1_block, conv3x3_block
from .resnet import ResUnit, ResStage
from ._build import ClassifierNet, register_variants
from ._tail import maybe_load_pretrained, DEFAULT_ROOT
from .. import engine

FUSED = True      # module-level switch: False = every exchange through engine.interpolate + engine.add (see the module docstring)


class Identity(nn.Module):
    """The reference's placeholder block (common/tutti.py): no parameters, returns its input."""
    def forward(self, x):
        return x


def _on_handles(module, xs, fn):
    """engine.boundary for a LIST of maps: NHWC handles pass straight through; NCHW fp32 tensors (how the reference's blocks are
    called) are converted in, and every result is converted back under the fp16 range guard."""
    many = isinstance(xs, (list, tuple))
    items = list(xs) if many else [xs]
    if all(isinstance(x, engine.NHWC) for x in items):
        return fn(items if many else items[0])
    if not all(torch.is_tensor(x) for x in items):
        raise TypeError("expected torch.Tensors or NHWC handles")
    dtype = engine.compute_dtype_of(module)
    guard = engine.Fp16Guard(items[0].device, engine.DTYPES[dtype][1])
    handles = [engine.from_nchw(x, dtype, stem=False) for x in items]
    ys = fn(handles if many else handles[0])
    if isinstance(ys, list):
        return [guard.finish(engine.to_nchw(y)) for y in ys]
    return guard.finish(engine.to_nchw(ys))


def _shift_of(scale_factor):
    s = int(scale_factor)
    return s.bit_length() - 1 if s == scale_factor and s >= 1 and (s & (s - 1)) == 0 else None


class UpSamplingBlock(nn.Module):
    """1x1 ConvBlock without activation + nearest upsampling by `scale_factor` (reference hrnet.py:17-47). Inside an HRBlock only
    `conv` runs, at the coarse resolution: the fuse launch reads its output through `shift` = log2(scale_factor). Called on its own
    the upsampling is that launch with one source."""
    def __init__(self, in_channels, out_channels, scale_factor):
        super(UpSamplingBlock, self).__init__()
        self.conv = conv1x1_block(in_channels=in_channels, out_channels=out_channels, stride=1, activation=None)
        self.upsample = nn.Upsample(scale_factor=scale_factor, mode="nearest")
        self.scale_factor = scale_factor
        self.shift = _shift_of(scale_factor)      # None: no power of two, composed path only

    def _run(self, a):
        c = self.conv(a)
        if FUSED and self.shift is not None and engine.hr_fuse_supported([self.shift], c.N, c.H << self.shift, c.W << self.shift,
                                                                         c.cpitch, 0, c.dtype):
            return engine.hr_fuse([c], [self.shift], 0)
        return engine.interpolate(c, (int(c.H * self.scale_factor), int(c.W * self.scale_factor)), False, False)

    def forward(self, x):
        return engine.boundary(self, x, self._run)


class HRBlock(nn.Module):
    """Parallel branches of basic ResUnits, then the exchange between all resolutions (reference hrnet.py:50-136). Takes and
    returns a list of maps, branch i at 1 / 2**i of branch 0's size."""
    def __init__(self, in_channels_list, out_channels_list, num_branches, num_subblocks):
        super(HRBlock, self).__init__()
        self.in_channels_list = in_channels_list          # (the caller's list, updated in place as the reference does)
        self.num_branches = num_branches

        self.branches = nn.Sequential()
        for i in range(num_branches):
            layers = nn.Sequential()
            in_channels_i = self.in_channels_list[i]
            out_channels_i = out_channels_list[i]
            for j in range(num_subblocks[i]):
                layers.add_module("unit{}".format(j + 1), ResUnit(in_channels=in_channels_i, out_channels=out_channels_i, stride=1,
                                                                  bottleneck=False))
                in_channels_i = out_channels_i
            self.in_channels_list[i] = out_channels_i
            self.branches.add_module("branch{}".format(i + 1), layers)

        if num_branches > 1:
            self.fuse_layers = nn.Sequential()
            for i in range(num_branches):
                fuse_layer = nn.Sequential()
                for j in range(num_branches):
                    if j > i:
                        fuse_layer.add_module("block{}".format(j + 1), UpSamplingBlock(
                            in_channels=in_channels_list[j], out_channels=in_channels_list[i], scale_factor=2 ** (j - i)))
                    elif j == i:
                        fuse_layer.add_module("block{}".format(j + 1), Identity())
                    else:
                        conv3x3_seq = nn.Sequential()
                        for k in range(i - j):
                            if k == i - j - 1:
                                conv3x3_seq.add_module("subblock{}".format(k + 1), conv3x3_block(
                                    in_channels=in_channels_list[j], out_channels=in_channels_list[i], stride=2, activation=None))
                            else:
                                conv3x3_seq.add_module("subblock{}".format(k + 1), conv3x3_block(
                                    in_channels=in_channels_list[j], out_channels=in_channels_list[j], stride=2))
                        fuse_layer.add_module("block{}".format(j + 1), conv3x3_seq)
                self.fuse_layers.add_module("layer{}".format(i + 1), fuse_layer)
            self.activ = nn.ReLU(True)

    def _exchange(self, i, x):
        """Output branch i of the exchange: the terms j = 0 .. B-1 in the reference's order, each (handle, shift, block)."""
        terms = []
        for j in range(self.num_branches):
            blk = self.fuse_layers[i][j]
            if j == i:
                terms.append((x[j], 0, None))
            elif j < i:
                terms.append((blk(x[j]), 0, None))                 # stride-2 chain: already at branch i's size
            else:
                terms.append((blk.conv(x[j]), blk.shift, blk))     # 1x1 at the coarse size; the upsampling is the fuse launch's read
        act = engine.act_code(self.activ)
        H, W = x[i].H, x[i].W
        shifts = [s for _, s, _ in terms]
        if FUSED and None not in shifts and engine.hr_fuse_supported(shifts, x[i].N, H, W, x[i].cpitch, act, x[i].dtype):
            return engine.hr_fuse([t for t, _, _ in terms], shifts, act)
        # composed: one launch per upsample and per add (hrnet.py:128-134 as written)
        y = None
        for k, (t, s, blk) in enumerate(terms):
            if blk is not None:
                t = engine.interpolate(t, (H, W), False, False)
            y = t if y is None else engine.add(y, t, post_act=act if k == len(terms) - 1 else 0)
        return y

    def _run(self, x):
        x = [self.branches[i](x[i]) for i in range(self.num_branches)]
        if self.num_branches == 1:
            return x
        return [self._exchange(i, x) for i in range(len(self.fuse_layers))]

    def forward(self, x):
        return _on_handles(self, x, self._run)


class HRStage(nn.Module):
    """Transition to this stage's branch widths (a new branch opens from the LAST map of the previous stage through stride-2
    convolutions), then `layers` of HRBlocks (reference hrnet.py:139-207). Takes one map or a list, returns a list."""
    def __init__(self, in_channels_list, out_channels_list, num_modules, num_branches, num_subblocks):
        super(HRStage, self).__init__()
        self.branches = num_branches
        self.in_channels_list = out_channels_list
        in_branches = len(in_channels_list)
        out_branches = len(out_channels_list)

        self.transition = nn.Sequential()
        for i in range(out_branches):
            if i < in_branches:
                if out_channels_list[i] != in_channels_list[i]:
                    self.transition.add_module("block{}".format(i + 1), conv3x3_block(
                        in_channels=in_channels_list[i], out_channels=out_channels_list[i], stride=1))
                else:
                    self.transition.add_module("block{}".format(i + 1), Identity())
            else:
                conv3x3_seq = nn.Sequential()
                for j in range(i + 1 - in_branches):
                    in_channels_i = in_channels_list[-1]
                    out_channels_i = out_channels_list[i] if j == i - in_branches else in_channels_i
                    conv3x3_seq.add_module("subblock{}".format(j + 1), conv3x3_block(
                        in_channels=in_channels_i, out_channels=out_channels_i, stride=2))
                self.transition.add_module("block{}".format(i + 1), conv3x3_seq)

        self.layers = nn.Sequential()
        for i in range(num_modules):
            self.layers.add_module("block{}".format(i + 1), HRBlock(
                in_channels_list=self.in_channels_list, out_channels_list=out_channels_list, num_branches=num_branches,
                num_subblocks=num_subblocks))
            self.in_channels_list = self.layers[-1].in_channels_list

    def _run(self, x):
        many = isinstance(x, list)
        x_list = []
        for j in range(self.branches):
            if not isinstance(self.transition[j], Identity):
                x_list.append(self.transition[j](x[-1] if many else x))
            else:
                x_list.append(x[j] if many else x)
        return self.layers(x_list)

    def forward(self, x):
        return _on_handles(self, x, self._run)


class HRInitBlock(nn.Module):
    """Two stride-2 3x3 ConvBlocks and `num_subblocks` bottleneck ResUnits (reference hrnet.py:210-253)."""
    def __init__(self, in_channels, out_channels, mid_channels, num_subblocks):
        super(HRInitBlock, self).__init__()
        self.conv1 = conv3x3_block(in_channels=in_channels, out_channels=mid_channels, stride=2)
        self.conv2 = conv3x3_block(in_channels=mid_channels, out_channels=mid_channels, stride=2)
        in_channels = mid_channels
        self.subblocks = ResStage()               # nn.Sequential in the reference: same children, same keys; chains the 1x1 pairs
        for i in range(num_subblocks):
            self.subblocks.add_module("block{}".format(i + 1), ResUnit(in_channels=in_channels, out_channels=out_channels, stride=1,
                                                                       bottleneck=True))
            in_channels = out_channels

    def forward(self, x):
        return engine.boundary(self, x, lambda a: self.subblocks(self.conv2(self.conv1(a))), stem=True)


class HRFinalBlock(nn.Module):
    """Classification head (reference hrnet.py:256-296): a bottleneck ResUnit per branch widens it to 128 .. 1024 channels; going
    down, `inc_blocks[i + 1](x[i + 1]) + down_blocks[i](y)` is the epilogue of the biased stride-2 down convolution (its own ReLU,
    then the add, nothing after it); a biased 1x1 ConvBlock to 2048 channels closes it."""
    def __init__(self, in_channels_list, out_channels_list):
        super(HRFinalBlock, self).__init__()
        self.inc_blocks = nn.Sequential()
        for i, in_channels_i in enumerate(in_channels_list):
            self.inc_blocks.add_module("block{}".format(i + 1), ResUnit(in_channels=in_channels_i, out_channels=out_channels_list[i],
                                                                        stride=1, bottleneck=True))
        self.down_blocks = nn.Sequential()
        for i in range(len(in_channels_list) - 1):
            self.down_blocks.add_module("block{}".format(i + 1), conv3x3_block(
                in_channels=out_channels_list[i], out_channels=out_channels_list[i + 1], stride=2, bias=True))
        self.final_layer = conv1x1_block(in_channels=1024, out_channels=2048, stride=1, bias=True)

    def _run(self, x):
        y = self.inc_blocks[0](x[0])
        for i in range(len(self.down_blocks)):
            y = self.down_blocks[i](y, residual=self.inc_blocks[i + 1](x[i + 1]), post_act=None)
        return self.final_layer(y)

    def forward(self, x):
        return _on_handles(self, x, self._run)


class HRNet(ClassifierNet):
    """`features` (init_block, stage1..3, final_block, final_pool) + `output` Linear (reference hrnet.py:299-379)."""
    def __init__(self, channels, init_block_channels, init_num_subblocks, num_modules, num_subblocks, in_channels=3,
                 in_size=(224, 224), num_classes=1000):
        super(HRNet, self).__init__(in_size, num_classes)
        self.branches = [2, 3, 4]
        self.features.add_module("init_block", HRInitBlock(in_channels=in_channels, out_channels=init_block_channels, mid_channels=64,
                                                           num_subblocks=init_num_subblocks))
        in_channels_list = [init_block_channels]
        for i in range(len(self.branches)):
            self.features.add_module("stage{}".format(i + 1), HRStage(
                in_channels_list=in_channels_list, out_channels_list=channels[i], num_modules=num_modules[i],
                num_branches=self.branches[i], num_subblocks=num_subblocks[i]))
            in_channels_list = self.features[-1].in_channels_list
        self.features.add_module("final_block", HRFinalBlock(in_channels_list=in_channels_list, out_channels_list=[128, 256, 512, 1024]))
        self.finish(2048)


def get_hrnet(version, model_name=None, pretrained=False, root=DEFAULT_ROOT, **kwargs):
    """HRNet with the reference's tables (hrnet.py:406-462)."""
    widths = {"w18s1": 16, "w18s2": 18, "w18": 18, "w30": 30, "w32": 32, "w40": 40, "w44": 44, "w48": 48, "w64": 64}
    if version not in widths:
        raise ValueError("Unsupported HRNet version {}".format(version))
    w = widths[version]
    channels = [[w, 2 * w], [w, 2 * w, 4 * w], [w, 2 * w, 4 * w, 8 * w]]
    if version == "w18s1":
        init_block_channels, init_num_subblocks, num_modules = 128, 1, [1, 1, 1]
    elif version == "w18s2":
        init_block_channels, init_num_subblocks, num_modules = 256, 2, [1, 3, 2]
    else:
        init_block_channels, init_num_subblocks, num_modules = 256, 4, [1, 4, 3]
    num_subblocks = [[max(2, init_num_subblocks)] * len(ci) for ci in channels]
    net = HRNet(channels=channels, init_block_channels=init_block_channels, init_num_subblocks=init_num_subblocks,
                num_modules=num_modules, num_subblocks=num_subblocks, **kwargs)
    return maybe_load_pretrained(net, model_name, pretrained, root)


# HRNet-W18 Small V1 / V2 and HRNetV2-W18 .. W64 (reference hrnet.py:476-635)
register_variants(__name__, get_hrnet, dict(
    [("hrnet_w18_small_v1", dict(version="w18s1")), ("hrnet_w18_small_v2", dict(version="w18s2"))] +
    [("hrnetv2_w{}".format(w), dict(version="w{}".format(w))) for w in (18, 30, 32, 40, 44, 48, 64)]))
