"""
CPU restatement of the HRNet fuse launch (pcv_hr_fuse, csrc/hrfuse.hpp) and the mistakes a kernel of this kind plausibly makes.

    y[n, h, w, c] = act( sum_t src_t[n, h >> shift_t, w >> shift_t, c] )

`model` does what the launch is specified to do: sequential fp32 adds in source order, the activation, then ONE `.to(storage)`.
fp32 adds are IEEE and the conversion rounds to nearest even, on the CPU as on the GPU, so a kernel is checked against it with
`torch.equal` - no tolerance. The bug models share its code and differ in one step each; tests/test_hrfuse_model.py shows that every
one of them changes the result on the sweep's data, i.e. that the sweep would catch it.

Tensors are NHWC [N, H >> s, W >> s, C] in the storage type, as the launch takes them.
"""

import functools
import torch

NONE, RELU = 0, 1
TORCH_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}

# (N, C, H, W, shifts): each the smallest shape that can trip one mechanism
SWEEP = [
    (2, 8, 8, 16, [0, 1, 2, 3]),          # the coarsest source is 1x2
    (2, 24, 4, 6, [0, 1]),                # H != W
    (3, 40, 8, 8, [0, 0, 0, 0]),          # all sources at one resolution
    (2, 144, 14, 14, [0, 0, 0, 1]),       # mixed: three fine sources, one coarse
    (2, 16, 56, 56, [0, 1, 2, 3]),        # a real map size
    (2, 8, 8, 8, [3]),                    # one source, a pure upsample
    (2, 72, 2, 2, [0, 1]),                # 1x1 coarse source
    (1, 32, 16, 24, [1, 0]),              # the fine source is not the first
]


def sweep_id(case):
    N, C, H, W, shifts = case
    return "n{}c{}_{}x{}_s{}".format(N, C, H, W, "".join(str(s) for s in shifts))


def make_sources(case, dtype, seed=0, small_ints=False):
    """The sources of a sweep case in the storage type `dtype` (a name of TORCH_DTYPES). Default data: normal values times a power
    of two in 2^-6 .. 2^6 per element, so that fp32 sums of three and more round (their order matters) and 16-bit partial sums
    round differently from the final one. `small_ints`: integers in [-8, 8] - every sum is exact in every type."""
    N, C, H, W, shifts = case
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for s in shifts:
        shape = (N, H >> s, W >> s, C)
        if small_ints:
            v = torch.randint(-8, 9, shape, generator=g).float()
        else:
            v = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())
        out.append(v.to(TORCH_DTYPES[dtype]).contiguous())
    return out


def _gather(src, s, H, W, how="floor"):
    """fp32 [N, H, W, C]: what output pixel (n, h, w) reads of `src` ([N, H >> s, W >> s, C]) - as specified ("floor") or with one
    indexing mistake. Pixel indices are formed flat, as a kernel forms them, and wrap inside the tensor."""
    N, Hs, Ws, C = src.shape
    n = torch.arange(N).view(N, 1, 1)
    h = torch.arange(H).view(1, H, 1)
    w = torch.arange(W).view(1, 1, W)
    if how == "floor":
        pix = (n * Hs + (h >> s)) * Ws + (w >> s)
    elif how == "shift_h_only":                    # the shift applied to h only
        pix = (n * Hs + (h >> s)) * Ws + w
    elif how == "row_pitch_fine":                  # the coarse row pitch taken as W instead of W >> s
        pix = (n * Hs + (h >> s)) * W + (w >> s)
    elif how == "image_stride_fine":               # the coarse image stride taken from the fine H * W
        pix = n * (H * W) + (h >> s) * Ws + (w >> s)
    elif how == "round_half":                      # (h + half) >> s instead of floor, kept inside the map
        half = (1 << s) >> 1
        pix = (n * Hs + ((h + half) >> s).clamp(max=Hs - 1)) * Ws + ((w + half) >> s).clamp(max=Ws - 1)
    else:
        raise ValueError(how)
    pix = (pix % (N * Hs * Ws)).expand(N, H, W).reshape(-1)
    return src.reshape(-1, C)[pix].reshape(N, H, W, C).float()


def _act(v, act):
    return torch.relu(v) if act == RELU else v


def model(sources, shifts, H, W, act, how="floor"):
    """The launch as specified: fp32 adds in source order, activation, one rounding to the sources' type."""
    acc = _gather(sources[0], shifts[0], H, W, how)
    for t in range(1, len(sources)):
        acc = acc + _gather(sources[t], shifts[t], H, W, how)
    return _act(acc, act).to(sources[0].dtype)


def model_f64(sources, shifts, H, W, act):
    """float64 sum, rounded once: equals `model` wherever fp32 summation is exact."""
    acc = torch.zeros((sources[0].shape[0], H, W, sources[0].shape[3]), dtype=torch.float64)
    for src, s in zip(sources, shifts):
        acc = acc + _gather(src, s, H, W).double()
    return _act(acc, act).to(sources[0].dtype)


# ---- the bug models: name -> (function, applies(case, dtype, act)) ---------------------------------------------------------------
def _bug_index(how):
    return lambda sources, shifts, H, W, act: model(sources, shifts, H, W, act, how)


def _bug_act_per_term(sources, shifts, H, W, act):
    acc = _act(_gather(sources[0], shifts[0], H, W), act)
    for t in range(1, len(sources)):
        acc = acc + _act(_gather(sources[t], shifts[t], H, W), act)
    return acc.to(sources[0].dtype)


def _bug_partial_rounding(sources, shifts, H, W, act):
    dt = sources[0].dtype
    acc = _gather(sources[0], shifts[0], H, W)
    for t in range(1, len(sources)):
        acc = (acc + _gather(sources[t], shifts[t], H, W)).to(dt).float()
    return _act(acc, act).to(dt)


def _bug_drop_last_of_four(sources, shifts, H, W, act):
    k = 3 if len(sources) == 4 else len(sources)
    return model(sources[:k], shifts[:k], H, W, act)


def _bug_reverse_order(sources, shifts, H, W, act):
    return model(sources[::-1], shifts[::-1], H, W, act)


def _coarse(case):
    return any(s > 0 for s in case[4])


BUGS = {
    "shift_h_only": (_bug_index("shift_h_only"), lambda case, dtype, act: _coarse(case)),
    "row_pitch_fine": (_bug_index("row_pitch_fine"), lambda case, dtype, act: _coarse(case)),
    # one image: the stride is never used
    "image_stride_fine": (_bug_index("image_stride_fine"), lambda case, dtype, act: _coarse(case) and case[0] > 1),
    # a 1x1 coarse map has only one pixel to read, whatever the rounding
    "round_half": (_bug_index("round_half"),
                   lambda case, dtype, act: any(s > 0 and ((case[2] >> s) > 1 or (case[3] >> s) > 1) for s in case[4])),
    "act_per_term": (_bug_act_per_term, lambda case, dtype, act: act == RELU and len(case[4]) > 1),
    # two sources: the only partial sum is the final one; fp32: rounding to the storage type is the identity
    "partial_rounding": (_bug_partial_rounding, lambda case, dtype, act: dtype != "fp32" and len(case[4]) > 2),
    "drop_last_of_four": (_bug_drop_last_of_four, lambda case, dtype, act: len(case[4]) == 4),
    # a + b == b + a; 16-bit inputs mostly sum exactly in fp32, so the order has to show in fp32 only
    "reverse_order": (_bug_reverse_order, lambda case, dtype, act: dtype == "fp32" and len(case[4]) > 2),
}


@functools.lru_cache(maxsize=None)
def sweep_reference(index, dtype, act):
    """(sources, expected output) of sweep case `index`: computed once per process and shared - callers do not write into them."""
    case = SWEEP[index]
    sources = make_sources(case, dtype, seed=index)
    return sources, model(sources, case[4], case[2], case[3], act)
