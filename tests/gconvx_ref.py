"""
The any-width grouped 3x3 kernel (csrc/gconvx.hpp) restated for the tests (plain module: CPU only, nothing of the GPU side is
imported): the case list of tests/test_gpu_gconvx_sweep.py, the library's routing and tile planner (plan_conv's `gconvx`,
gconvx_launch_why and plan_gconvx of csrc/pcv_api.hip) in Python, and an fp32 emulation of the kernel that walks its own structure -
tiles of R whole output rows x GB whole groups, the contiguous window, K = 9 taps x Cg / 8 eight-channel chunks in steps of four
chunks padded with zero chunks, 16-row output slabs, border taps zeroed - with the bug models tests/test_gconvx_bounds.py applies:
  group_shift   a group reads its neighbour's input channels (the next group of the channel block)
  pad_chunk     the zero-padded K chunks are multiplied (their weights repeat chunk 0, their data is read instead of zeroed)
  border_tap    the tap left of column 0 / above row 0 is not zeroed: it reads the pixel its address holds
  parity_swap   stride 2: even and odd input columns swapped
  skip_last_cb  the last, partial channel block is not computed
  drop_tail     the tail tile (the last rows of the last image) is not computed
"""

import collections

import torch

from conv_ref import Geom, conv_ref_bound, operands
from test_gpu_conv_sweep import C, NONE, RELU, RELU6, case_id, geom_of, plan, seed_of  # noqa: F401
from test_gpu_dw_se import act64

WIDTHS = (8, 16, 24, 40, 48, 56, 64)          # GCONVX_WIDTHS
MAX_LDS = 48 * 1024                            # kGConvXMaxLds
PB = (4, 7)                                    # kGConvXPB
MAX_W = 112
DTYPES16 = ("bf16", "fp16")


def X(N, ch, cg, H, W, s, act=RELU, note="", **kw):
    return C(N, ch, ch, H, W, s=s, groups=ch // cg, act=act, note=note, **kw)


# ---- the cases (N, C, Cg, H, W, stride) ------------------------------------------------------------------------------------------
_REQUIRED = [
    (2, 24, 8, 6, 10, 2, ""), (2, 56, 8, 5, 7, 1, ""), (3, 152, 8, 4, 6, 1, "tail tile across image borders, 19 groups in blocks of 10 + 9"),
    (2, 72, 24, 6, 8, 2, ""), (3, 120, 24, 7, 5, 1, "5 groups: one channel block of 128 / Cg groups"), (2, 80, 40, 5, 9, 1, ""),
    (2, 240, 40, 8, 8, 2, ""), (2, 96, 48, 7, 7, 1, ""), (2, 168, 56, 6, 6, 2, ""),
    (2, 48, 16, 9, 11, 1, "C % 64 != 0 with an 'old' group width"),
    (1, 24, 8, 4, 112, 2, "the 112-wide window; LDS budget: R = 2 rows fit with all 3 groups"),
    (1, 48, 24, 4, 112, 2, "the 112-wide window; LDS budget: two groups (four units) only fit at R = 1"),
]
_BOUNDARIES = [
    (1, 16, 8, 3, 64, 1, "tile size: Wo = 64, R = 1, 64 pixels - the 4-block instantiation"),
    (1, 16, 8, 3, 65, 1, "tile size: 65 pixels - the 7-block instantiation"),
    (1, 16, 8, 4, 56, 1, "row count: Wo = 56, R = 2, all 112 pixels of the 7-block tile"),
    (1, 16, 8, 3, 57, 1, "row count: Wo = 57, R = 1"),
    (2, 144, 24, 5, 5, 1, "channel block: 6 groups = 128 / Cg + 1, two blocks of 3"),
    (1, 56, 8, 2, 112, 2, "LDS budget: room for 5 of the 7 groups, blocks of 4 + 3"),
    (1, 96, 48, 4, 26, 2, "measured class: 48 per group at stride 2 below the 28 .. 56-wide maps that went back to the generic kernel"),
    (1, 112, 56, 2, 56, 2, "measured class: 56 per group at stride 2, the widest map the kernel keeps"),
    (1, 112, 56, 3, 28, 1, "measured class: 56 per group at stride 1, the widest map the kernel keeps"),
]                                     # (every row names the planner or routing boundary it sits on)
_EPI_SHAPES = [(2, 56, 8, 5, 7, 1), (2, 72, 24, 6, 8, 2), (2, 80, 40, 5, 9, 1)]

CASES = ([X(N, ch, cg, H, W, s, act=(RELU, NONE, RELU6)[i % 3], note=note) for i, (N, ch, cg, H, W, s, note) in enumerate(_REQUIRED + _BOUNDARIES)] +
         [X(*shape, act=a, note="epilogue") for shape in _EPI_SHAPES for a in (RELU, NONE, RELU6)])
CASES = list(dict.fromkeys(CASES))
# launches the kernel declines: they run on the generic kernel and hold the same bound
DECLINED = [X(2, 56, 8, 5, 7, 1, act=NONE, post=RELU, res=True, note="residual + post_act"),
            X(2, 56, 8, 5, 7, 1, cpitch=64, note="padded x_cpitch"),
            X(2, 56, 8, 5, 7, 1, yslice=(8, 16), note="sliced y")]
# ... and the other side of the measured classes: shapes the kernel could run that the routing leaves on the generic kernel
CLASS_DECLINED = [X(1, 96, 48, 4, 28, 2, note="48 per group, stride 2, W = 28"), X(1, 96, 48, 2, 56, 2, note="48 per group, stride 2, W = 56"),
                  X(1, 112, 56, 2, 58, 2, note="56 per group, stride 2, W = 58"), X(1, 112, 56, 3, 30, 1, note="56 per group, stride 1, W = 30"),
                  X(1, 80, 40, 4, 28, 2, note="40 per group follows 48"), X(1, 128, 64, 3, 30, 1, note="64 per group: nowhere"),
                  X(2, 128, 64, 14, 14, 2, note="64 per group: nowhere"), X(1, 192, 64, 7, 7, 1, note="64 per group: nowhere")]


# ---- routing and planner restated (csrc/pcv_api.hip) ---------------------------------------------------------------------------------
XPlan = collections.namedtuple("XPlan", "R GB pbi win pitch lds nRowTiles nCB")


def plan_gconvx(stride, H, W, Ho, Wo, groups, cg, N=1):
    """plan_gconvx: the tile of a launch, or None where the kernel does not take the map"""
    if stride == 2 and ((H | W) & 1):
        return None
    if W > MAX_W or Ho <= 0 or Wo <= 0:
        return None
    cpg, sl = cg // 8, (cg + 15) // 16
    min_gb = min(groups, (4 + sl - 1) // sl)
    want_gb = min(groups, max(min_gb, 128 // cg))
    for R in range(16 * PB[1] // Wo, 0, -1):
        win = (2 * R + 1) * W + 2 if stride == 2 else (R + 2) * W + 2
        p16 = MAX_LDS // (16 * win)
        if p16 % 2 == 0:
            p16 -= 1
        fit_gb = p16 // cpg
        if fit_gb < (1 if R == 1 else min_gb):
            continue
        gb = min(want_gb, fit_gb)
        ncb = (groups + gb - 1) // gb
        gb = (groups + ncb - 1) // ncb
        pitch = 16 * ((gb * cpg) | 1)
        return XPlan(R, gb, 0 if R * Wo <= 16 * PB[0] else 1, win, pitch, win * pitch, (N * Ho + R - 1) // R, (groups + gb - 1) // gb)
    return None


def gconvx_pays(cg, stride, W):
    """gconvx_pays: the shape classes the kernel keeps after the measurement (profiles/experiments/gconvx_kernel.md)"""
    if cg <= 24:
        return True
    if cg <= 48:
        return not (stride == 2 and 28 <= W <= 56)
    if cg > 56:
        return False
    return not ((stride == 2 and W > 56) or (stride == 1 and W > 28))


def gconvx_static(c, dtype):
    """plan_conv's `gconvx`: the shapes that carry the kernel's weight blob"""
    P = plan(c, dtype)
    cg = c.Cin // c.groups
    return (P.ok and not P.gconv and dtype != "fp32" and c.groups > 1 and (c.kh, c.kw) == (3, 3) and c.sh == c.sw and c.sh in (1, 2) and
            (c.dh, c.dw) == (1, 1) and (c.pt, c.pl, c.pb, c.pr) == (1, 1, 1, 1) and c.Cin == c.Cout and cg in WIDTHS and not c.out_f32)


def route(c, dtype):
    """the tile (XPlan) of a launch that the library's own routing sends to gconvx.hpp, else None (gconvx_launch_why)"""
    if not gconvx_static(c, dtype) or c.gate or c.res or c.post != NONE or c.yslice:
        return None
    if (c.cpitch or c.Cin) != c.Cin or (c.wpitch or c.W) != c.W:
        return None
    tune = dict(c.tune)
    if tune.get("gconvx", 1) == 0 or tune.get("gconvr", 1) == 0:
        return None
    P = plan(c, dtype)
    if c.N * P.Ho * P.Wo * c.Cin * 2 >= 1 << 31:
        return None
    if not gconvx_pays(c.Cin // c.groups, c.sh, c.W):
        return None
    return plan_gconvx(c.sh, c.H, c.W, P.Ho, P.Wo, c.groups, c.Cin // c.groups, c.N)


# ---- the kernel, emulated in fp32 --------------------------------------------------------------------------------------------------------
MUTANTS = ("group_shift", "pad_chunk", "border_tap", "parity_swap", "skip_last_cb", "drop_tail")


def relevant_mutants(c, dtype):
    xp = route(c, dtype)
    cg = c.Cin // c.groups
    Ho = (c.H - 1) // c.sh + 1
    m = ["border_tap"]
    if xp.GB > 1:
        m.append("group_shift")
    if (9 * (cg // 8)) % 4 and Ho > 1:             # (a pad chunk sits at tap (0, 0): on a one-row map the top border zeroes it anyway)
        m.append("pad_chunk")
    if c.sh == 2:
        m.append("parity_swap")
    if c.groups % xp.GB:
        m.append("skip_last_cb")
    if (c.N * Ho) % xp.R:
        m.append("drop_tail")
    return m


def pack(w, groups, cg, mutant=None):
    """pack_gconvx_kernel: w [C][Cg][3][3] -> [group][slab][step][16 rows][32 K]"""
    cpg, sl = cg // 8, (cg + 15) // 16
    nk = (9 * cpg + 3) // 4
    out = torch.zeros((groups, sl, nk, 16, 32), dtype=torch.float32)
    wg = w.float().reshape(groups, cg, cg, 9)                 # [group][o][ci][tap]
    for j in range(4 * nk):
        live = j < 9 * cpg
        if not live and mutant != "pad_chunk":
            continue
        tap, cc = (j // cpg, j % cpg) if live else (0, 0)
        ks, f = j // 4, j % 4
        for s in range(sl):
            rows = min(16, cg - 16 * s)
            out[:, s, ks, :rows, 8 * f:8 * f + 8] = wg[:, 16 * s:16 * s + rows, 8 * cc:8 * cc + 8, tap]
    return out


def emulate(c, ops, dtype, mutant=None):
    """the output of the kernel on the case's operands in fp32 arithmetic, rounded to the storage type; NHWC float64. Elements the
    (mutated) kernel never writes stay 0."""
    from conv_ref import round_to
    xp = route(c, dtype)
    assert xp is not None
    S, W, H, N, Cc = c.sh, c.W, c.H, c.N, c.Cin
    cg, G = Cc // c.groups, c.groups
    cpg, sl = cg // 8, (cg + 15) // 16
    nch, nk = 9 * cpg, (9 * cpg + 3) // 4
    Ho, Wo = (H - 1) // S + 1, (W - 1) // S + 1
    Min, Mout = N * H * W, N * Ho * Wo
    R, GB, win = xp.R, xp.GB, xp.win
    RWo = R * Wo
    xflat = ops.x.float().reshape(Min, Cc)
    wp = pack(ops.w, G, cg, mutant)
    y = torch.zeros((Mout, Cc), dtype=torch.float32)
    # per K chunk j = 4 ks + f: tap (r, q), channel chunk; a pad chunk reads chunk 0 of tap 0 and is killed
    jr = torch.tensor([(j // cpg) // 3 if j < nch else 0 for j in range(4 * nk)])
    jq = torch.tensor([(j // cpg) % 3 if j < nch else 0 for j in range(4 * nk)])
    jc = torch.tensor([j % cpg if j < nch else 0 for j in range(4 * nk)])
    jpad = torch.tensor([j >= nch for j in range(4 * nk)])
    ml = torch.arange(RWo)
    ho_l, wo = ml // Wo, ml % Wo
    for cb in range(xp.nCB):
        grp0 = cb * GB
        glive = min(GB, G - grp0)
        if mutant == "skip_last_cb" and glive < GB:
            continue
        for rt in range(xp.nRowTiles):
            if mutant == "drop_tail" and rt == xp.nRowTiles - 1:
                continue
            g0 = rt * R
            cbase = (S * g0 - 1) * W - 1
            # the window: [win][GB Cg], zeros outside the batch and beyond the block's channels
            pix = cbase + torch.arange(win)
            okp = (pix >= 0) & (pix < Min)
            wnd = torch.zeros((win, GB * cg), dtype=torch.float32)
            wnd[okp, :glive * cg] = xflat[pix[okp], grp0 * cg:(grp0 + glive) * cg]
            gh = (g0 + ho_l) % Ho
            m = g0 * Wo + ml
            okm = m < Mout
            for gl in range(glive):
                src = gl
                if mutant == "group_shift":
                    src = (gl + 1) % glive
                acc = torch.zeros((RWo, sl * 16), dtype=torch.float32)
                for ks in range(nk):
                    b = torch.zeros((RWo, 32), dtype=torch.float32)
                    for f in range(4):
                        j = 4 * ks + f
                        r, q, cc = int(jr[j]), int(jq[j]), int(jc[j])
                        col = S * wo + q
                        if mutant == "parity_swap":
                            col = col ^ 1
                        row = S * ho_l * W + r * W + col
                        kill = torch.zeros(RWo, dtype=torch.bool)
                        if mutant != "border_tap":
                            kill |= (gh == 0) & (r == 0)
                            kill |= (wo == 0) & (q == 0)
                        if S == 1:
                            kill |= (gh == Ho - 1) & (r == 2)
                            kill |= (wo == W - 1) & (q == 2)
                        if bool(jpad[j]) and mutant != "pad_chunk":
                            kill |= True
                        v = wnd[row.clamp(0, win - 1), src * cg + 8 * cc:src * cg + 8 * cc + 8]
                        b[:, 8 * f:8 * f + 8] = torch.where(kill[:, None], torch.zeros_like(v), v)
                    a = wp[grp0 + gl, :, ks].reshape(sl * 16, 32)
                    acc = acc + b @ a.t()                      # one MFMA K-step: 32 products summed, added to the accumulator
                ch = (grp0 + gl) * cg
                v = acc[:, :cg]
                if ops.scale is not None:
                    v = v * ops.scale[ch:ch + cg]
                v = act64(v + ops.shift[ch:ch + cg], c.act)
                assert v.dtype == torch.float32
                y[m[okm], ch:ch + cg] = v[okm]
    return round_to(y, dtype).double().reshape(N, Ho, Wo, Cc)


def case_reference(c, dtype):
    """(operands, float64 reference, bound) of a case"""
    ops = operands(c.N, c.H, c.W, c.Cout, geom_of(c), dtype, seed_of(c), with_res=c.res, with_gate=c.gate)
    ref, bound = conv_ref_bound(ops.x, ops.w, ops.scale, ops.shift, geom_of(c), c.act, ops.res, c.post, ops.gate, out_dtype=dtype)
    return ops, ref, bound
