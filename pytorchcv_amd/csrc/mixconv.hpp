// mixconv.hpp - depthwise MixConv (mixed window sizes per channel group), NHWC, fused scale/shift/activation epilogue, ONE launch.
//
// Replaces: MixConv.forward with groups == channels (reference pytorchcv/models/mixnet.py:76-80: torch.split, one depthwise Conv2d per
//           group with windows 3, 5, ..., 3 + 2 (G - 1) and padding k // 2, torch.cat) + BatchNorm2d(eval) + activation of
//           MixConvBlock.forward (mixnet.py:151-157), as MixUnit.conv1 uses it (mixnet.py:256-263).
//
// Every group reads its own channel slice of x in place and writes its own slice of y: no slice copy, no concat copy, no launch per
// group. Blocks map to (window class, channel chunk, output column, row strip): a wave never mixes window sizes.
//
// Form. The row-streaming scheme of dwconv5_kernel (dwconv.hpp), generalised to KS = 3 .. 11: a thread owns CPT channels of one output
// column over a strip of rows, keeps ONE input row of its KS columns plus one accumulator per in-flight output row (ceil(KS / S) of
// them), and feeds input row t into output row (t - dy) / S through filter row dy. Where the KS * KS taps live decides the rest. As
// fp32 pairs (what v_pk_fma_f32 takes) at 2 channels per thread they cost 2 KS KS registers: 98 at 7 x 7, 162 at 9 x 9, 242 at
// 11 x 11 - and 512 registers at one wave per SIMD are no way out, because the VALU reads only the first 256 (the other half is
// AGPRs: the compiler copied every tap through v_accvgpr_read, measured 186-239 AGPRs for the G = 5 instances). So:
//     KS      16 bit                                             fp32
//     3, 5    CPT 4, taps as fp32 pairs (36 / 100 registers)     CPT 2, fp32 pairs (18 / 50)
//     7       CPT 2, taps as fp32 pairs (98)                     CPT 2, fp32 pairs (98)
//     9, 11   CPT 2, taps as PACKED 16-bit pairs, one dword per  CPT 2, taps re-read per filter row through the vector L1
//             tap (81 / 121), unpacked on use                    (11 pairs live; the validation mode, not a hot path)
// and the 9 x 9 / 11 x 11 classes hand their input row over by register copies (two rows live) instead of the static ring, whose
// PERIOD slots stay live as a whole across the conditional phases. Every instance runs at two waves per SIMD and none spills
// (220-226 registers at 16 bit, 138-252 at fp32, scratch 0: profiles/experiments/mixconv_kernel.md). The unpack costs two VALU
// instructions and a copy per packed FMA; taps in LDS would put a ds_read_b64 in front of every packed FMA with the four SIMDs of
// a CU sharing one LDS port, and the L1 form of the fp32 column measured 1.5-1.7x slower than the packed form at 16 bit; a
// filter-row split reads every input row KS times.
// A kernel instance holds the classes 3 .. 3 + 2 (G - 1), so its register allocation is that of its LARGEST class (the 5 x 5 one).
//
// Group boundaries. Group widths follow MixConv.split_channels (mixnet.py:83-86: the first group takes the remainder) and must be
// even, so a CPT = 2 chunk never straddles two groups. A CPT = 4 chunk may (width 90: boundaries at 90, 180, 270): it then runs the
// LARGER window, with the smaller filter zero-embedded at the centre by the pack kernel - a k x k filter with pad k // 2 equals a
// K x K filter (K > k) with pad K // 2 whose outer ring is zero, at stride 1 and 2, with the same output size; the added products are
// exact zeros, so nothing rounds differently. The class regions (mix_plan below, shared by the pack and the launch):
//     class 3   channels [0, e3)            e3 = end of group 0 rounded DOWN to a multiple of 4
//     class 5   channels [e3, b4)           b4 = end of group 1 rounded down to a multiple of 4 (G == 2: b4 = C)
//     class 7   channels [b4, end of group 2), class 9 and 11: their own groups
// Packed blob: per class, from a 16-byte aligned offset, the taps [KS * KS][span] in the storage type (span = channels of the region).
//
// Loads are buffer loads with range checking: a padded tap is an offset beyond num_records and returns zeros, no branches.
// The chunk types, loadn / storen and the packed-fp32 helpers are dw_device.hpp's; the streaming loop is dw_stream_rows, shared with dwconv5_kernel.
#pragma once
#include "dw_device.hpp"

constexpr int kMixMaxGroups = 5;

// channels per thread of window class g (KS = 3 + 2 g) at `esize` bytes per element
constexpr int mix_cpt(int esize, int g) { return (g < 2 && esize == 2) ? 4 : 2; }

struct MixPlan {
    int cbeg[kMixMaxGroups], span[kMixMaxGroups], cpt[kMixMaxGroups];
    uint32_t woff[kMixMaxGroups];
    size_t bytes;
};
// `why` (when not NULL) receives the reason of a refusal
static inline bool mix_plan(int C, int G, int esize, MixPlan& P, const char** why = nullptr) {
    const char* dummy;
    if (!why) why = &dummy;
    if (G < 2 || G > kMixMaxGroups) { *why = "mixconv: 2 to 5 kernels"; return false; }
    if (C <= 0 || C % 8 != 0) { *why = "mixconv: channels must be a multiple of 8"; return false; }
    const int wr = C / G, w0 = C - (G - 1) * wr;
    if (wr < 2 || (wr & 1) || (w0 & 1)) { *why = "mixconv: odd group width (MixConv.split_channels of this channel count) unsupported"; return false; }
    int gend[kMixMaxGroups];
    for (int j = 0; j < G; ++j) gend[j] = w0 + j * wr;
    const int e3 = gend[0] & ~3, b4 = G == 2 ? C : (gend[1] & ~3);
    size_t off = 0;
    for (int g = 0; g < kMixMaxGroups; ++g) {
        const int ks = 3 + 2 * g;
        int b = 0, e = 0;
        if (g < G) {
            b = g == 0 ? 0 : (g == 1 ? e3 : (g == 2 ? b4 : gend[g - 1]));
            e = g == 0 ? e3 : (g == 1 ? b4 : gend[g]);
        }
        P.cbeg[g] = b;
        P.span[g] = e - b;
        P.cpt[g] = mix_cpt(esize, g);
        P.woff[g] = (uint32_t)off;
        off += ((size_t)ks * ks * (e - b) * esize + 15) & ~(size_t)15;
    }
    P.bytes = off;
    return true;
}

struct MixParams {
    const void* x;
    const void* w;        // packed blob (layout above)
    void* y;
    const float* scale;
    const float* shift;
    uint32_t x_bytes;     // buffer num_records of x
    int N, H, W, C, Ho, Wo;
    int TH;               // output rows per thread
    int nseg;             // ceil(Ho / TH)
    int act;
    int flags;            // bit 0 = non-temporal output stores, bit 1 = blocks in dispatch order (as DwParams)
    uint32_t* ovf;        // the context's fp16 overflow counter
    int cbeg[kMixMaxGroups];         // per window class: first channel,
    int nchunk[kMixMaxGroups];       // chunks of CPT channels,
    int span[kMixMaxGroups];         // channels (= row length of its taps in the blob),
    uint32_t woff[kMixMaxGroups];    // byte offset of its taps in the blob,
    uint32_t blk_end[kMixMaxGroups]; // and the end of its run of blocks in the grid
};

struct MixPackParams {
    const float* w[kMixMaxGroups];   // fp32 [Cg, 1, k, k] of every group, as in the state dict
    void* out;
    int G, w0, wr;                   // group widths: w0 (group 0), wr (the others)
    int cbeg[kMixMaxGroups], span[kMixMaxGroups];
    uint32_t woff[kMixMaxGroups];
    int elem_end[kMixMaxGroups];     // running total of blob elements per class
};

template <int DT>
__global__ __launch_bounds__(256) void pack_mix_kernel(const MixPackParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.elem_end[kMixMaxGroups - 1]) return;
    int g = 0;
    while (i >= p.elem_end[g]) ++g;
    const int r = i - (g == 0 ? 0 : p.elem_end[g - 1]);
    const int ks = 3 + 2 * g, span = p.span[g];
    const int k = r / span, c = p.cbeg[g] + r % span;
    const int j = c < p.w0 ? 0 : 1 + (c - p.w0) / p.wr;                 // the channel's own group and window
    const int cj = c < p.w0 ? c : (c - p.w0) % p.wr;
    const int kj = 3 + 2 * j, ring = (ks - kj) / 2;
    const int fr = k / ks - ring, fq = k % ks - ring;
    float v = 0.f;                                                         // outside the centred kj x kj filter: the zero ring
    if (fr >= 0 && fr < kj && fq >= 0 && fq < kj) v = p.w[j][((size_t)cj * kj + fr) * kj + fq];
    store_elem<DT>(static_cast<char*>(p.out) + p.woff[g], (size_t)r, v);
}

// one window class: KS x KS over the chunks of class GI = (KS - 3) / 2; `blk` counts from the first block of the class
template <int DT, int KS, int S, bool FAST, int CPT>
__device__ __forceinline__ void mixdw_class(const MixParams& p, const uint32_t blk) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int GI = (KS - 3) / 2;
    const int nchunk = p.nchunk[GI];
    const long idx = (long)blk * 256 + threadIdx.x;
    if (idx >= (long)p.N * p.nseg * p.Wo * nchunk) return;
    const DwThread th = dw_decode(idx, nchunk, p.Wo, p.nseg, p.TH, p.Ho);
    const int cr = th.chunk * CPT;                 // channel within the class region
    const DwStream a = {p.x, p.x_bytes, static_cast<const char*>(p.w) + p.woff[GI], p.span[GI], cr, p.scale, p.shift, nullptr, p.y,
                        p.H, p.W, p.C, p.Ho, p.Wo, KS / 2, KS / 2, p.act, PCV_ACT_NONE, p.ovf};
    dw_stream_rows<DT, KS, S, FAST, CPT, false>(a, th, p.cbeg[GI] + cr);
#endif  // __HIP_DEVICE_COMPILE__
}

// G window classes (3 .. 3 + 2 (G - 1)) in one grid: blocks [blk_end[g - 1], blk_end[g]) run class g. FAST as in dwconv.hpp.
template <int DT, int S, bool FAST, int G>
__global__ __launch_bounds__(256, 2) void mixdw_kernel(const MixParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    // neighbouring blocks of a class read overlapping input columns: each XCD gets a contiguous run of blocks (see dwconv_kernel)
    const uint32_t b = (p.flags & 2) ? blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    constexpr int CPT35 = mix_cpt(DT == PCV_F32 ? 4 : 2, 0);
    if (b < p.blk_end[0]) { mixdw_class<DT, 3, S, FAST, CPT35>(p, b); return; }
    if (b < p.blk_end[1]) { mixdw_class<DT, 5, S, FAST, CPT35>(p, b - p.blk_end[0]); return; }
    if constexpr (G >= 3) {
        if (b < p.blk_end[2]) { mixdw_class<DT, 7, S, FAST, 2>(p, b - p.blk_end[1]); return; }
    }
    if constexpr (G >= 4) {
        if (b < p.blk_end[3]) { mixdw_class<DT, 9, S, FAST, 2>(p, b - p.blk_end[2]); return; }
    }
    if constexpr (G >= 5) {
        if (b < p.blk_end[4]) { mixdw_class<DT, 11, S, FAST, 2>(p, b - p.blk_end[3]); return; }
    }
#endif  // __HIP_DEVICE_COMPILE__
}

// instantiation lists: one translation unit per storage type (mixconv_*.hip), declared extern in pcv_api.hip
#define MIX_INSTANCES(X, DT) \
    X(DT, 1, true, 2) X(DT, 1, true, 3) X(DT, 1, true, 4) X(DT, 1, true, 5) \
    X(DT, 2, true, 2) X(DT, 2, true, 3) X(DT, 2, true, 4) X(DT, 2, true, 5) \
    X(DT, 1, false, 2) X(DT, 1, false, 3) X(DT, 1, false, 4) X(DT, 1, false, 5) \
    X(DT, 2, false, 2) X(DT, 2, false, 3) X(DT, 2, false, 4) X(DT, 2, false, 5)
#define MIX_DECLARE(DT, S, FAST, G) extern template __global__ void mixdw_kernel<DT, S, FAST, G>(const MixParams);
#define MIX_DEFINE(DT, S, FAST, G) template __global__ void mixdw_kernel<DT, S, FAST, G>(const MixParams);
