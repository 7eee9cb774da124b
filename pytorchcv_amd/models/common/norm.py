"""
    Normalisation generators (reference pytorchcv/models/common/norm.py:34-50,95-115). Eval-mode BatchNorm2d holds the
    parameters under the reference's state_dict names and is folded into the convolution epilogue as fp32 scale/shift
    (pcv_bn_fold); `IBN` (norm.py:118-162) adds the one normalisation that cannot fold, InstanceNorm2d over the image in flight
    (pcv_instnorm_act).
"""

__all__ = ['lambda_batchnorm2d', 'create_normalization_layer', 'IBN']

import math
from inspect import isfunction
import torch.nn as nn
from ... import engine


def lambda_batchnorm2d(eps: float = 1e-5):
    return lambda num_features: nn.BatchNorm2d(num_features=num_features, eps=eps)


def create_normalization_layer(normalization, **kwargs):
    assert (normalization is not None)
    if isfunction(normalization):
        return normalization(**kwargs)
    assert isinstance(normalization, nn.Module)
    return normalization


class IBN(nn.Module):
    """Instance-Batch Normalization (reference norm.py:118-162): InstanceNorm2d(affine=True) on the first
    floor(channels * first_fraction) channels, BatchNorm2d on the rest, in the original channel order. Attribute names are the
    reference's. On the hot path the module never sees the BatchNorm half: the producing convolution folds it into its epilogue
    (engine.IBNConvRunner) and hands the whole tensor here, so `forward(x, act)` on a handle is pcv_instnorm_act over
    (C, Cn = split_sections[0]) with the block's activation behind it. Both sections must be multiples of 8 (16-byte channel
    chunks); `inst_first=False` is not built."""
    def __init__(self, channels, first_fraction=0.5, inst_first=True):
        super(IBN, self).__init__()
        if not inst_first:
            raise NotImplementedError("IBN(inst_first=False) is not on the MI355X path")
        self.inst_first = inst_first
        h1_channels = int(math.floor(channels * first_fraction))
        h2_channels = channels - h1_channels
        if h1_channels % 8 or h2_channels % 8 or h1_channels <= 0 or h2_channels <= 0:
            raise NotImplementedError("IBN sections {} + {}: the MI355X path needs multiples of 8".format(h1_channels, h2_channels))
        self.split_sections = [h1_channels, h2_channels]
        self.inst_norm = nn.InstanceNorm2d(num_features=h1_channels, affine=True)
        self.batch_norm = nn.BatchNorm2d(num_features=h2_channels)
        self._pcv_in = None
        self._pcv_bn = None

    def run_inst(self, a, act=0):
        """The InstanceNorm half + activation on a convolution output whose BatchNorm half is already applied."""
        if self._pcv_in is None:
            self._pcv_in = engine.InstNormRunner(self.inst_norm)
        return self._pcv_in.run(a, act)

    def _run(self, a):
        # stand-alone (the reference's forward on a raw tensor): the BatchNorm half as an elementwise pass over its slice
        if self._pcv_bn is None:
            self._pcv_bn = engine.BnActRunner(self.batch_norm)
        h1, h2 = self.split_sections
        y = self.run_inst(a, 0)
        z = self._pcv_bn.run(engine.channel_slice(a, h1, h2), 0)
        engine.channel_concat_into(z, y.t, h1)
        return y

    def forward(self, x):
        return engine.boundary(self, x, self._run)
