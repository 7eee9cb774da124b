"""
float64 reference, elementwise bound, inputs and shape table of the InstanceNorm sweep (csrc/instnorm.hpp behind pcv_instnorm_act),
shared by tests/test_gpu_instnorm.py (GPU) and tests/test_instnorm_bounds.py (CPU: that plausible bugs violate the bound).

Semantics, on the stored (already rounded) x[N, HW, x_cpitch], C logical channels, Cn normalised ones, per image n:
    c <  Cn : y = act(gamma[c] (x - m[n,c]) / sqrt(v[n,c] + eps) + beta[c])      m, v: mean and BIASED variance over the HW positions
    c >= Cn : y = act(x)

The kernel's reduction plan, restated (as pair_ref.py restates WPairCfg): a statistics block has 512 threads over [rows x chunks] with
at most GROUP = 8 eight-channel chunks, so a group of Gc chunks keeps rows = 512 // Gc pixels in flight; a thread sums
n_t = ceil(HW / rows) values as s1 = sum (x - K), s2 = sum (x - K)^2 with K its first value, forms (n_t, K + s1 / n_t, s2 - s1^2 / n_t),
and the rows meet pairwise by Chan's formula in T = ceil(log2(min(rows, HW))) levels. Then v = M2 (1 / HW), a = gamma / sqrt(v + eps),
b = beta - m a, and the second kernel computes act(x a + b).

Bound, first order in u = 2^-24, per (image, channel) plane with R = max |x - m| and |.| of float64 quantities:
  mean     : a thread's s1 is n_t - 1 additions of rounded differences, |d| <= 2 R: (n_t + 2) u 2 R on s1 / n_t, then K + . rounds with
             u (|m| + R). A merge m_a + (m_b - m_a) f is a convex combination of its inputs (their errors do not grow) and rounds
             with u (|m| + R) + 3 u 2 R. After T levels
                 E_m = u ((T + 1) (|m| + R) + (2 n_t + 4 + 6 T) R)
             - the only terms that see |m| are T + 1 final roundings: the shift K keeps the magnitude of the mean out of the sums.
  M2       : per thread s2 - s1^2 / n_t: each of s2 and s1^2 / n_t is within (2 n_t + 2) u sum d^2 (Cauchy-Schwarz for the second),
             and sum over all threads of d^2 <= 2 HW (v + R^2). A merge (q_a + q_b) + d^2 (n_a n_b / n) rounds within 4 u of the
             merged M2 (<= HW v) and sees the error of d: 2 |d| (n_a n_b / n) 2 E_m; over one level sum |d| n_a n_b / n <=
             sqrt(sum d^2 n_a n_b / n  sum n_a n_b / n) <= sqrt(HW v  HW / 4). After T levels and the rounded 1 / HW and product
                 E_v = u (4 n_t + 4) 2 (v + R^2) + 4 T u v + 2 T E_m sqrt(v) + 2 u v
  a, b     : w = v + eps rounds once: E_w = E_v + u w; sqrt, reciprocal and the product with gamma are correctly rounded:
             rel_a = E_w / (2 w) + 3 u. b = beta - m a: |b' - b| <= |m| |a| rel_a + |a| E_m + u (|m a| + |b|).
  apply    : pre = x a + b, one product and one sum (or one fma): the m a parts of x a and of b cancel,
                 E_pre = |x - m| |a| rel_a + |a| E_m + u (|m a| + |b|) + u (|x a| + |pre|)
             c >= Cn: E_pre = 0 (x is copied).
  then the activation (act_err) and the output rounding (out_bound) of tests/test_gpu_dw_se.py.
Nothing here is fitted to what the kernel gives.
"""

import math
import torch
from test_gpu_dw_se import U32, ULP, FLOOR, act64, act_err, out_bound      # noqa: F401  (ULP / FLOOR: re-exported for the tests)

EPS = 1e-5
THREADS, GROUP = 512, 8         # instnorm.hpp: kInThreads, kInGroup

# (N, H, W, C, Cn, x_cpitch)
SHAPES = [(2, 1, 1, 8, 8, 8), (3, 7, 9, 64, 32, 64), (2, 5, 5, 24, 8, 24), (2, 33, 31, 40, 40, 40), (1, 56, 56, 16, 16, 16),
          (2, 12, 12, 512, 256, 512), (2, 6, 6, 32, 16, 48), (4, 14, 14, 256, 128, 256), (2, 9, 7, 64, 0, 64)]
ALL_ACTS_SHAPE = (3, 7, 9, 64, 32, 64)
OFFSET_SHAPE = (2, 32, 32, 16, 16, 16)          # fp32 storage, mean 1024, standard deviation 1
TINY_STD = 3e-3                                 # one channel of every input: eps matters there


def plan(HW, Cn):
    """(n_t, T) per channel chunk of the Cn normalised channels: samples per thread and merge levels (see the module text)."""
    out = []
    Cn8 = Cn // 8
    for g0 in range(0, Cn8, GROUP):
        Gc = min(GROUP, Cn8 - g0)
        rows = THREADS // Gc
        live = min(rows, HW)
        out += [((HW + rows - 1) // rows, int(math.ceil(math.log2(live))) if live > 1 else 0)] * Gc
    return out


def make_inputs(shape, dtype, seed=0):
    """x[N, HW, x_cpitch] in `dtype` (the pad channels beyond C hold other values, never read), gamma, beta (fp32 [Cn]). Per-channel
    scale and mean differ, image n is offset by its own amount (pooled statistics differ from per-image ones), channel 3 has a
    standard deviation of TINY_STD."""
    N, H, W, C, Cn, xp = shape
    g = torch.Generator().manual_seed(1000 * seed + N + 7 * H + 13 * W + C + Cn)
    std = 0.25 + 1.5 * torch.rand(xp, generator=g)
    std[3] = TINY_STD
    mean = torch.randn(xp, generator=g)
    img = 0.5 * torch.randn((N, 1, xp), generator=g) * std
    x = torch.randn((N, H * W, xp), generator=g) * std + mean + img
    gamma = 0.5 + torch.rand(max(Cn, 0), generator=g)
    beta = torch.rand(max(Cn, 0), generator=g) - 0.5
    return x.to(dtype), gamma, beta


def offset_inputs(seed=0):
    N, H, W, C, Cn, xp = OFFSET_SHAPE
    g = torch.Generator().manual_seed(77 + seed)
    x = 1024.0 + torch.randn((N, H * W, xp), generator=g)
    return x.float(), 0.5 + torch.rand(Cn, generator=g), torch.rand(Cn, generator=g) - 0.5


def instnorm_ref(x, gamma, beta, C, Cn, act, eps=EPS, stats=None):
    """(ref, err) in float64, [N, HW, C]: the exact result on the stored x and the bound on the kernel's pre-rounding error.
    `stats` = (m, v) [N, 1, Cn] replaces the statistics (the bug models of the CPU test)."""
    N, HW, _ = x.shape
    xd = x.double()[:, :, :C]
    pre = xd.clone()
    e = torch.zeros_like(pre)
    if Cn > 0:
        xn = xd[:, :, :Cn]
        m = xn.mean(dim=1, keepdim=True)
        v = ((xn - m) ** 2).mean(dim=1, keepdim=True)
        if stats is not None:
            ms, vs = stats
        else:
            ms, vs = m, v
        gd, bd = gamma.double()[None, None, :], beta.double()[None, None, :]
        a = gd / torch.sqrt(vs + eps)
        b = bd - ms * a
        pre[:, :, :Cn] = xn * a + b
        R = (xn - m).abs().amax(dim=1, keepdim=True)
        pl = plan(HW, Cn)
        nt = torch.tensor([p[0] for p in pl], dtype=torch.float64).repeat_interleave(8)[None, None, :]
        T = torch.tensor([p[1] for p in pl], dtype=torch.float64).repeat_interleave(8)[None, None, :]
        u = U32
        E_m = u * ((T + 1) * (m.abs() + R) + (2 * nt + 4 + 6 * T) * R)
        E_v = u * (4 * nt + 4) * 2 * (v + R ** 2) + 4 * T * u * v + 2 * T * E_m * torch.sqrt(v) + 2 * u * v
        w = v + eps
        rel_a = (E_v + u * w) / (2 * w) + 3 * u
        e[:, :, :Cn] = (xn - m).abs() * a.abs() * rel_a + a.abs() * E_m + u * ((m * a).abs() + b.abs()) + \
            u * ((xn * a).abs() + pre[:, :, :Cn].abs())
    return act64(pre, act), act_err(pre, e, act)


def fp32_single_pass_stats(x, Cn):
    """The form the kernel must NOT use, evaluated in fp32: mean = sum(x) / HW, var = sum(x^2) / HW - mean^2."""
    xf = x.float()[:, :, :Cn]
    n = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    mean = xf.sum(dim=1, keepdim=True) / n
    ex2 = (xf * xf).sum(dim=1, keepdim=True) / n
    return mean.double(), (ex2 - mean * mean).double()


def fp32_two_pass_stats(x, Cn):
    """A permitted form in fp32: mean, then the mean of (x - mean)^2."""
    xf = x.float()[:, :, :Cn]
    n = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    mean = xf.sum(dim=1, keepdim=True) / n
    d = xf - mean
    return mean.double(), ((d * d).sum(dim=1, keepdim=True) / n).double()
