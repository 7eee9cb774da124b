"""
float64 reference and error bound of the depthwise MixConv launch (csrc/mixconv.hpp behind pcv_mixconv2d_fused), shared by the GPU
sweep (tests/test_gpu_mixconv.py) and the CPU checks of its bounds (tests/test_mixconv_bounds.py).

Reference: the depthwise restatement `dw_ref` of tests/test_gpu_dw_se.py applied per channel group - group g has the window
k = 3 + 2 g, padding k // 2 and the channels MixConv.split_channels gives it (the first group takes the remainder).

Bound: that file's derived depthwise bound with KK = the channel's OWN k * k, whatever window the kernel runs the channel in. A
chunk of channels that straddles a group boundary runs the larger window with the smaller filter zero-embedded at the centre; the
extra taps are exact zeros, fma(acc, x, 0) = acc for finite x, so they round nothing and the smaller window's bound holds. The order
in which a kernel sums the k * k products does not enter the bound. Nothing here is fitted to observed errors.

`taps_from_blob` reads the taps back from the packed blob (the layout documented in DESIGN.md and csrc/mixconv.hpp), so the
reference convolves with exactly what the kernel reads; it also checks that every embedded ring is zero.
"""

import torch

from test_gpu_dw_se import TDT, NONE, dw_ref, out_bound        # noqa: F401  (out_bound: re-exported for the two test files)


def split_channels(C, G):
    """MixConv.split_channels of the reference: C // G each, the first group takes the remainder."""
    w = [C // G] * G
    w[0] += C - sum(w)
    return w


def group_bounds(C, G):
    """[(begin, end)] of the G channel groups"""
    out, b = [], 0
    for w in split_channels(C, G):
        out.append((b, b + w))
        b += w
    return out


def mix_operands(N, H, W, C, G, dtype, seed):
    """x (rounded to the compute dtype), the fp32 weights [Cg, 1, k, k] of the G groups, BN (gamma, beta, mean, var)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, C), generator=g).to(TDT[dtype]).float()
    ws = [torch.randn((wg, 1, 3 + 2 * i, 3 + 2 * i), generator=g) * (1.5 / (3 + 2 * i)) for i, wg in enumerate(split_channels(C, G))]
    gamma = torch.rand(C, generator=g) * 1.5 + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    mean = torch.randn(C, generator=g) * 0.3
    var = torch.rand(C, generator=g) * 1.5 + 0.5
    return x, ws, (gamma, beta, mean, var)


def taps_of_group(w, dtype):
    """[k*k][Cg] taps of one group's weight [Cg, 1, k, k], rounded to the storage type (what pcv_mixconv_pack stores)"""
    return w.reshape(w.shape[0], -1).t().contiguous().to(TDT[dtype]).float()


def mix_ref(x, taps, scale, shift, s, act):
    """float64 act(scale * mixdw(x) + shift) on NHWC x; taps[g] = [k*k][Cg] of group g. Returns (reference, bound of the kernel's
    fp32 error before the output rounding), both NHWC over all channels."""
    C, G = x.shape[3], len(taps)
    refs, errs = [], []
    for g, (b, e) in enumerate(group_bounds(C, G)):
        k = 3 + 2 * g
        assert tuple(taps[g].shape) == (k * k, e - b)
        r, err = dw_ref(x[..., b:e], taps[g], scale[b:e], shift[b:e], k, s, (k // 2,) * 4, act, None, NONE)
        refs.append(r)
        errs.append(err)
    return torch.cat(refs, dim=3), torch.cat(errs, dim=3)


# ---- the packed blob ------------------------------------------------------------------------------------------------------------
def mix_plan(C, G, esize):
    """The class regions of the packed blob (mix_plan of csrc/mixconv.hpp): per window class g (K = 3 + 2 g) the first channel, the
    number of channels and the byte offset of its taps [K*K][span]; and the blob size."""
    ends = [e for _, e in group_bounds(C, G)]
    e3 = ends[0] & ~3
    b4 = C if G == 2 else ends[1] & ~3
    regions, off = [], 0
    for g in range(G):
        b = 0 if g == 0 else e3 if g == 1 else b4 if g == 2 else ends[g - 1]
        e = e3 if g == 0 else b4 if g == 1 else ends[g]
        K = 3 + 2 * g
        regions.append((b, e - b, off))
        off += (K * K * (e - b) * esize + 15) // 16 * 16
    return regions, off


def taps_from_blob(packed, C, G, dtype):
    """taps[g] = [k*k][Cg] per GROUP, read back from the blob pcv_mixconv_pack wrote (a uint8 tensor); every channel that a larger
    window class runs must have an exactly zero ring around its own k x k filter."""
    tdt = TDT[dtype]
    es = torch.tensor([], dtype=tdt).element_size()
    regions, total = mix_plan(C, G, es)
    assert packed.numel() >= total
    per_channel = [None] * C
    for cls, (b, span, off) in enumerate(regions):
        K = 3 + 2 * cls
        if span == 0:
            continue
        t = packed[off:off + K * K * span * es].view(tdt).view(K, K, span).float().cpu()
        for g, (gb, ge) in enumerate(group_bounds(C, G)):
            lo, hi = max(gb, b), min(ge, b + span)
            if lo >= hi:
                continue
            k, ring = 3 + 2 * g, (K - (3 + 2 * g)) // 2
            assert ring >= 0, "a channel runs in a window class smaller than its own window"
            blk = t[:, :, lo - b:hi - b]
            inner = blk[ring:ring + k, ring:ring + k]
            outer = blk.clone()
            outer[ring:ring + k, ring:ring + k] = 0
            assert int(torch.count_nonzero(outer)) == 0, "embedded ring of class {} group {} is not zero".format(K, g)
            for c in range(lo, hi):
                per_channel[c] = inner[:, :, c - lo].reshape(k * k)
    assert all(v is not None for v in per_channel), "a channel is in no class region"
    return [torch.stack(per_channel[b:e], dim=1) for (b, e) in group_bounds(C, G)]
