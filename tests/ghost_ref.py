"""
float64 reference, derived error bound and CPU bug models of the ghost-module launch (csrc/ghost.hpp, pcv_ghost_dw_fused):

    y[.., c]      = m[.., c]                                     + res[.., c]          c in [0, Cm)
    y[.., Cm + c] = act(scale[c] * dw3x3(m)[.., c] + shift[c])   + res[.., Cm + c]

m is NHWC [N, H, W, CP] with CP = round8(Cm) (pad channels are never read), taps [9][CP], scale / shift [CP]; y and res are dense
[N, H, W, 2 Cm]. Shared by tests/test_ghost_bounds.py (CPU) and tests/test_gpu_ghost.py (GPU).

Bound (first order in u = 2^-24, built on `dw_ref` of tests/test_gpu_dw_se.py; U = the output rounding of the storage type):
  cheap half : the depthwise bound with KK = 9, |e_pre| <= 10 u (|scale| sum_k |m_k||w_k| + |shift|), through the activation
               (e_a = L e_pre + T(pre); clamp(v, 0, 1) is a clamp: L = 1, T = 0), then the fp32 add of res, u (|a| + |res|), then ONE
               storage rounding of the sum: |y - ref| <= U |ref| + (1 + U) e + F.
  main half  : without res a bit copy of m[.., :Cm] (16 bit -> fp32 -> 16 bit is exact) - checked with torch.equal, bound 0; with res
               one fp32 add, u (|m| + |res|), and one storage rounding.
The bound is not fitted to observed errors: the bug models below (CPU restatements of the launch with one plausible mistake each) have
to violate it, or the exact-copy check, on the sweep shapes.
"""

import torch
from test_gpu_dw_se import TDT, U32, LIP, NONE, RELU, act64, act_err, out_bound, dw_ref

CLAMP01 = 7
ALL_CODES = tuple(range(8))

# (N, Cm, H, W), each the smallest that can trip one mechanism
SWEEP_SHAPES = [(2, 12, 9, 11),      # pitch 16, offset 12
                (2, 8, 5, 5),
                (2, 92, 7, 7),
                (2, 100, 14, 14),
                (3, 20, 1, 1),       # centre tap only
                (2, 36, 40, 3),      # several row strips
                (2, 60, 6, 1),       # W = 1
                (2, 240, 7, 9)]
SENTINEL = 32768.0                   # pad channels of m: large, finite in every storage type, exact in bf16 / fp16


def round8(c):
    return (c + 7) // 8 * 8


def act64x(v, code):
    return v.clamp(0, 1) if code == CLAMP01 else act64(v, code)


def act_errx(v, e, code):
    return e if code == CLAMP01 else act_err(v, e, code)


def ghost_ref(m, taps, scale, shift, Cm, act, res=None):
    """float64 reference [N, H, W, 2 Cm] and the bound of the kernel's fp32 error before the output rounding (0 on the main half
    without res). `m` [N, H, W, CP], `taps` [9][CP], `scale` / `shift` [CP]: only their first Cm channels are used."""
    mm = m[..., :Cm]
    pre, e_pre = dw_ref(mm, taps[:, :Cm], scale[:Cm], shift[:Cm], 3, 1, (1, 1, 1, 1), NONE)
    cheap = act64x(pre, act)
    e_cheap = act_errx(pre, e_pre, act)
    main = mm.double()
    e_main = torch.zeros_like(main)
    if res is not None:
        r = res.double()
        e_cheap = e_cheap + U32 * (cheap.abs() + r[..., Cm:].abs())
        cheap = cheap + r[..., Cm:]
        e_main = U32 * (main.abs() + r[..., :Cm].abs())
        main = main + r[..., :Cm]
    return torch.cat((main, cheap), dim=3), torch.cat((e_main, e_cheap), dim=3)


def ghost_bound(ref, err, dtype, Cm, has_res):
    """|y - ref| allowed per element; the main half without res is exact (bound 0)."""
    b = out_bound(ref, err, dtype)
    if not has_res:
        b[..., :Cm] = 0.0
    return b


def violations(y, ref, bound):
    """number of elements outside the bound (a NaN - an element nobody wrote - counts)"""
    return int((~((y.double() - ref).abs() <= bound)).sum())


def ghost_operands(N, Cm, H, W, dtype, seed, with_res):
    """m [N, H, W, CP] in the compute dtype (as fp32 values) with SENTINEL in its pad channels, the fp32 depthwise weight [Cm, 1, 3, 3],
    BN (gamma, beta, mean, var) and the residual [N, H, W, 2 Cm]"""
    g = torch.Generator().manual_seed(seed)
    CP = round8(Cm)
    m = torch.full((N, H, W, CP), SENTINEL)
    m[..., :Cm] = torch.randn((N, H, W, Cm), generator=g)
    m = m.to(TDT[dtype]).float()
    w = torch.randn((Cm, 1, 3, 3), generator=g) * 0.5
    gamma = torch.rand(Cm, generator=g) * 1.5 + 0.5
    beta = torch.randn(Cm, generator=g) * 0.5
    mean = torch.randn(Cm, generator=g) * 0.3
    var = torch.rand(Cm, generator=g) * 1.5 + 0.5
    res = torch.randn((N, H, W, 2 * Cm), generator=g).to(TDT[dtype]).float() if with_res else None
    return m, w, (gamma, beta, mean, var), res


def padded_taps(w, dtype):
    """[9][CP] taps of a depthwise weight [Cm, 1, 3, 3] rounded to the storage type, zero in the pad channels (what pcv_dwconv_pack
    writes for the layer padded to round8(Cm) channels)"""
    Cm = w.shape[0]
    t = torch.zeros((9, round8(Cm)))
    t[:, :Cm] = w.reshape(Cm, 9).t()
    return t.to(TDT[dtype]).float()


def padded(v, fill=0.0):
    out = torch.full((round8(v.shape[0]),), fill, dtype=v.dtype)
    out[:v.shape[0]] = v
    return out


# ---- CPU restatement of the launch in fp32, with one optional mistake ------------------------------------------------------------
BUGS = ("cheap_at_round8", "pad_channel_copied", "res_on_one_half", "act_on_main", "taps_at_pitch_cm", "border_taps_swapped")


def bug_applies(bug, Cm, W, act, has_res):
    """whether `bug` changes anything on this case (a pitch mistake needs Cm % 8 != 0, a border swap a second column, ...)"""
    if bug in ("cheap_at_round8", "pad_channel_copied", "taps_at_pitch_cm"):
        return Cm % 8 != 0
    if bug == "res_on_one_half":
        return has_res
    if bug == "act_on_main":
        return act not in (NONE,)
    if bug == "border_taps_swapped":
        return W >= 2
    return True


def ghost_model(m, taps, scale, shift, Cm, act, res, dtype, bug=None):
    """What the launch stores, restated in fp32 on the CPU and rounded to `dtype`: [N, H, W, 2 Cm] as fp32 values, NaN where
    nothing was written."""
    N, H, W, CP = m.shape
    x = m.float()
    flat = taps.float().reshape(-1)
    pitch = Cm if bug == "taps_at_pitch_cm" else CP
    idx = torch.arange(Cm)
    w = torch.stack([flat[k * pitch + idx] for k in range(9)]).view(3, 3, Cm)
    xp = torch.nn.functional.pad(x[..., :Cm], (0, 0, 1, 1, 1, 1))
    z = torch.zeros((N, H, W, Cm))
    for dy in range(3):
        for dx in range(3):
            z = z + xp[:, dy:dy + H, dx:dx + W, :] * w[dy, dx]
    if bug == "border_taps_swapped":
        zs = torch.zeros((N, H, W, Cm))
        for dy in range(3):
            for dx in range(3):
                zs = zs + xp[:, dy:dy + H, dx:dx + W, :] * w[dy, 2 - dx]
        z[:, :, 0, :] = zs[:, :, 0, :]
        z[:, :, W - 1, :] = zs[:, :, W - 1, :]
    cheap = act64x(scale[:Cm].float() * z + shift[:Cm].float(), act).float()
    main = x[..., :Cm].clone()
    if bug == "act_on_main":
        main = act64x(main, act).float()
    if res is not None:
        main = main + res[..., :Cm].float()
        if bug != "res_on_one_half":
            cheap = cheap + res[..., Cm:].float()
    y = torch.full((N, H, W, 2 * Cm + 8), float("nan"))
    off = CP if bug == "cheap_at_round8" else Cm
    y[..., off:off + Cm] = cheap
    if bug == "pad_channel_copied":
        y[..., :CP] = x if res is None else torch.cat((main, x[..., Cm:]), dim=3)      # whole 8-channel chunks of m, after the cheap half
    else:
        y[..., :Cm] = main
    return y[..., :2 * Cm].to(TDT[dtype]).float()
