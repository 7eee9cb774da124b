"""float64 restatement of the four stages of a CBAM block (ChannelGate and SpatialGate of CBAM-ResNet) on NHWC tensors, for the kernel
sweeps of tests/test_gpu_cbam.py. Every function returns the exact result AND the conditioning of the sums behind it (the same sums
over absolute values), which is what an fp32 error bound is relative to. Torch on the CPU only; nothing here touches the library."""

import torch
import torch.nn.functional as F


def pool(x):
    """x [N, H, W, C] -> (s [N, 2, C]: mean then max over the map, cond [N, C]: mean of |x|)."""
    x = x.double()
    N, H, W, C = x.shape
    f = x.reshape(N, H * W, C)
    return torch.stack([f.mean(dim=1), f.max(dim=1).values], dim=1), f.abs().mean(dim=1)


def excite(s, w1, b1, w2, b2):
    """s [N, 2, C] -> (gate [N, C] = sigmoid(fc2(relu(fc1(mean))) + fc2(relu(fc1(max)))), mid [N, 2, M], cond [N, C]: the
    conditioning of the pre-activation: the two layers evaluated on absolute values)."""
    s, w1, b1, w2, b2 = (t.double() for t in (s, w1, b1, w2, b2))
    mid = torch.relu(s @ w1.t() + b1)                                  # [N, 2, M]
    z = (mid @ w2.t() + b2).sum(dim=1)
    amid = s.abs() @ w1.abs().t() + b1.abs()
    cond = (amid @ w2.abs().t() + b2.abs()).sum(dim=1)
    return torch.sigmoid(z), mid, cond


def spatial_pool(x, gate):
    """x [N, H, W, C], gate [N, C] -> (p [N, H, W, 2]: max then mean over the channels of x * gate, cond [N, H, W, 2]: max and mean
    of |x * gate|)."""
    g = x.double() * gate.double()[:, None, None, :]
    p = torch.stack([g.max(dim=3).values, g.mean(dim=3)], dim=3)
    cond = torch.stack([g.abs().max(dim=3).values, g.abs().mean(dim=3)], dim=3)
    return p, cond


def spatial_gate(p, w7, scale, shift):
    """p [N, H, W, 2] -> (sg [N, H, W] = sigmoid(scale * conv7x7(p, w7, pad 3) + shift), cond [N, H, W]: |scale| * the convolution
    of |p| with |w7| + |shift|)."""
    p, w7 = p.double(), w7.double().reshape(1, 2, 7, 7)
    scale, shift = float(scale), float(shift)
    z = F.conv2d(p.permute(0, 3, 1, 2), w7, padding=3)[:, 0]
    cond = abs(scale) * F.conv2d(p.abs().permute(0, 3, 1, 2), w7.abs(), padding=3)[:, 0] + abs(shift)
    return torch.sigmoid(scale * z + shift), cond


def apply(x, gate, p, w7, scale, shift, res=None, relu=False):
    """y = post_act((x * gate[n, c]) * sg[n, h, w] + residual) -> (y [N, H, W, C], sg [N, H, W], cond_sg [N, H, W], xg = |x * gate|)."""
    sg, cond_sg = spatial_gate(p, w7, scale, shift)
    xg = x.double() * gate.double()[:, None, None, :]
    y = xg * sg[..., None]
    if res is not None:
        y = y + res.double()
    if relu:
        y = torch.relu(y)
    return y, sg, cond_sg, xg.abs()


def block(x, w1, b1, w2, b2, w7, scale, shift, res=None, relu=False):
    """The four stages chained in float64: (y, channel gate [N, C], spatial gate [N, H, W])."""
    s, _ = pool(x)
    gate, _, _ = excite(s, w1, b1, w2, b2)
    p, _ = spatial_pool(x, gate)
    y, sg, _, _ = apply(x, gate, p, w7, scale, shift, res, relu)
    return y, gate, sg
