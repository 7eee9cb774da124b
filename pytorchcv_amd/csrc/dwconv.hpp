// dwconv.hpp - depthwise KSxKS convolution, NHWC, fused scale/shift/activation/residual epilogue.
//
// Replaces: dwconv_block -> ConvBlock(groups=out_channels) (reference pytorchcv/models/common/conv.py:437-473),
//           i.e. Conv2d(groups=C) + BatchNorm2d(eval) + ReLU6 of LinearBottleneck.conv2 (mobilenetv2.py:53-57).
//
// HBM-bound (3.4 FLOP/B): the job is to read every input byte once and write every output byte once with 16-byte
// accesses and enough of them in flight. One thread owns 8 consecutive channels (one 16-byte NHWC chunk at 16 bit) of
// one output column and walks DOWN the image with a KS x KS fp32 window in registers, so per output row it loads only
// the STRIDE new input rows (KS chunks each).
//   * Loads are `buffer_load_dwordx4` with range checking: a padded (out-of-image) tap is an offset beyond
//     num_records and returns zeros - no branches, so all loads of a step issue back to back.
//   * Software prefetch: the rows needed by output row h+1 are requested before the FMAs of row h.
//   * The window rotates by register renaming (the row loop is unrolled over the rotation period), no moves.
//   * Consecutive lanes = consecutive channel chunks, then consecutive output columns: every wave-level access is one
//     contiguous NHWC span; the +-1 column re-reads hit the same lines in the vector L1.
// The chunk types, loadn / storen and the packed-fp32 helpers live in dw_device.hpp, shared with mixconv.hpp and ghost.hpp.
#pragma once
#include "dw_device.hpp"

struct DwParams {
    const void* x;
    const void* w;        // packed [KS*KS][C] in DT
    const void* res;
    void* y;
    const float* scale;
    const float* shift;
    uint32_t x_bytes;     // buffer num_records of x
    int N, H, W, C, Ho, Wo;
    int pt, pl;
    int C8;               // C / channels-per-thread
    int TH;               // output rows per thread
    int nseg;             // ceil(Ho / TH)
    int act, post_act;
    long total;           // N * nseg * Wo * C8
    int flags;            // tuning: bit 0 = non-temporal output stores, bit 1 = blocks in dispatch order (no XCD remap)
    uint32_t* ovf;        // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
};

// FAST: both activations are none/relu/relu6 (a clamp); the general activation codes live in the FAST=false build so
// that their transcendental code does not bloat the hot kernel.
// CPT: channels per thread (8, or 4 for the 5x5 window whose 25 taps x 8 channels would not fit the register file).
template <int DT, int KS, int S, bool FAST, int CPT = 8>
__global__ __launch_bounds__(256, 2) void dwconv_kernel(const DwParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int ES = Elem<DT>::BYTES;
    constexpr int KEEP = KS > S ? KS - S : 0;       // rows shared by consecutive output rows
    constexpr int NEW = KS - KEEP;                  // rows fetched per output row
    // Neighbouring blocks read overlapping input columns (+-1 column per output column: up to three blocks per line). Blocks b and
    // b + 8 share an XCD's L2, not b and b + 1: in dispatch order every shared line was fetched into two or three L2s (PMC: 1.33x the
    // algorithmic bytes at the fabric, which this HBM-bound kernel cannot afford). xcd_remap gives each XCD a contiguous run of blocks.
    const long idx = (long)((p.flags & 2) ? blockIdx.x : xcd_remap(blockIdx.x, gridDim.x)) * 256 + threadIdx.x;      // (flags bit 1: dispatch order, A/B)
    if (idx >= p.total) return;
    const DwThread th = dw_decode(idx, p.C8, p.Wo, p.nseg, p.TH, p.Ho);
    const int n = th.n, wo = th.wo, c0 = th.chunk * CPT, ho_begin = th.ho_begin, ho_end = th.ho_end;

    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(p.x, p.x_bytes);

    constexpr int NV = CPT / 2;          // packed fp32 pairs per chunk
    f32x2 wgt[KS * KS][NV];
#pragma unroll
    for (int k = 0; k < KS * KS; ++k) {
        float w8[CPT];
        loadn<DT, CPT>(p.w, (size_t)k * p.C + c0, w8);
#pragma unroll
        for (int e = 0; e < NV; ++e) wgt[k][e] = (f32x2){w8[2 * e], w8[2 * e + 1]};
    }
    f32x2 sc[NV], sf[NV];
    {
        float a8[CPT], b8[CPT];
        loadn<PCV_F32, CPT>(p.scale, c0, a8);
        loadn<PCV_F32, CPT>(p.shift, c0, b8);
#pragma unroll
        for (int e = 0; e < NV; ++e) { sc[e] = (f32x2){a8[2 * e], a8[2 * e + 1]}; sf[e] = (f32x2){b8[2 * e], b8[2 * e + 1]}; }
    }
    const ActClamp act = make_act(p.act), pact = make_act(p.post_act);

    // per-column byte offsets (relative to the row start) or "invalid"
    const int wi0 = wo * S - p.pl;
    uint32_t coloff[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q)
        coloff[q] = (unsigned)(wi0 + q) < (unsigned)p.W ? (uint32_t)(((wi0 + q) * p.C + c0) * ES) : kOutOfRange;
    const uint32_t rowbytes = (uint32_t)(p.W * p.C * ES);
    const uint32_t imgoff = (uint32_t)n * (uint32_t)p.H * rowbytes;

    auto fetch_row = [&](int hi, RawChunk<DT, CPT> (&row)[KS]) {
        const bool rowok = (unsigned)hi < (unsigned)p.H;
        const uint32_t rbase = imgoff + (uint32_t)hi * rowbytes;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            const uint32_t off = (rowok && coloff[q] != kOutOfRange) ? rbase + coloff[q] : kOutOfRange;
            raw_load<DT, CPT>(xrsrc, off, row[q]);
        }
    };

    f32x2 win[KS][KS][NV];               // slot-indexed rows; row r of the current window lives in slot (r + S*phase) % KS
    constexpr int PD = (KS == 3 && S == 1) ? 3 : 1;   // prefetch depth in output rows; divides the unroll period (static ring slots)
    RawChunk<DT, CPT> raw[PD][NEW][KS];       // ring: raw[t % PD] holds the NEW rows of output row t (relative to ho_begin)

    // prologue: the KEEP rows shared with the first output row go straight into the window; the NEW rows of the first
    // PD output rows are requested up front
    const int hi_first = ho_begin * S - p.pt;
    {
        RawChunk<DT, CPT> tmp[KEEP > 0 ? KEEP : 1][KS];
#pragma unroll
        for (int r = 0; r < KEEP; ++r) fetch_row(hi_first + r, tmp[r]);
#pragma unroll
        for (int d = 0; d < PD; ++d) {
            // rows beyond this thread's strip are not requested (offset forced invalid through hi = -1)
            const bool need = ho_begin + d < ho_end;
#pragma unroll
            for (int r = 0; r < NEW; ++r) fetch_row(need ? hi_first + d * S + KEEP + r : -1, raw[d][r]);
        }
#pragma unroll
        for (int r = 0; r < KEEP; ++r)
#pragma unroll
            for (int q = 0; q < KS; ++q) raw_to_f32x2<DT, CPT>(tmp[r][q], win[r][q]);
    }

    int ho = ho_begin;
    int hi = hi_first;
    F16Guard<DT> guard;
    const bool bounded = act_bounded(p.post_act) || (p.post_act == PCV_ACT_NONE && p.res == nullptr && act_bounded(p.act));
    while (ho < ho_end) {
        static_for<KS>([&](auto PHC) {
            constexpr int PH = decltype(PHC)::value;
            if (ho < ho_end) {
                // rows KEEP..KS-1 of this window arrive from the ring slot of this output row
#pragma unroll
                for (int r = 0; r < NEW; ++r)
#pragma unroll
                    for (int q = 0; q < KS; ++q) raw_to_f32x2<DT, CPT>(raw[PH % PD][r][q], win[(KEEP + r + S * PH) % KS][q]);
                // refill the slot with the rows of output row ho + PD before doing this row's arithmetic
                {
                    const bool need = ho + PD < ho_end;
#pragma unroll
                    for (int r = 0; r < NEW; ++r) fetch_row(need ? hi + PD * S + KEEP + r : -1, raw[PH % PD][r]);
                }
                f32x2 acc[NV];
#pragma unroll
                for (int e = 0; e < NV; ++e) acc[e] = pk_mul(win[(S * PH) % KS][0][e], wgt[0][e]);
#pragma unroll
                for (int r = 0; r < KS; ++r)
#pragma unroll
                    for (int q = 0; q < KS; ++q) {
                        if (r == 0 && q == 0) continue;
#pragma unroll
                        for (int e = 0; e < NV; ++e)
                            pk_fma_acc(acc[e], win[(r + S * PH) % KS][q][e], wgt[r * KS + q][e]);
                    }

                const size_t eoff = (((size_t)n * p.Ho + ho) * p.Wo + wo) * p.C + c0;
                float v[CPT];
                dw_bn<CPT>(acc, sc, sf, v);
                dw_act<FAST>(v, act);
                if (p.res != nullptr) dw_add_res<DT, CPT>(p.res, eoff, v);
                if (p.post_act != PCV_ACT_NONE) {
                    dw_act<FAST>(v, pact);
                }
                if (!bounded) guard.see(v);
                storen<DT, CPT>(p.y, eoff, v, (p.flags & 1) != 0);      // (dw_flags bit 0 reaches the 8-channel 16-bit store only: kept)
                ++ho;
                hi += S;
            }
        });
    }
    guard.commit(p.ovf);
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- depthwise 5x5 (dwconv5x5_block, conv.py:511-543: MobileNetV3, EfficientNet): the row-streaming core of dw_device.hpp -----------
// The register window above needs KS * KS input chunks AND KS * KS taps live per thread: 200 registers at 5x5 even with 4 channels
// per thread, which spilled. Row streaming keeps 25 taps + 5 (stride 1) or 3 (stride 2) accumulators + the rows in flight, nothing
// spills, the same 5 loads per output row. One thread = 4 channels (8 bytes at 16 bit) of one output column over its strip of rows.
template <int DT, int S, bool FAST>
__global__ __launch_bounds__(256, 2) void dwconv5_kernel(const DwParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int CPT = 4;
    // (dw_flags bit 1, blocks in dispatch order, has never reached this kernel: kept)
    const long idx = (long)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;      // (see dwconv_kernel)
    if (idx >= p.total) return;
    const DwThread th = dw_decode(idx, p.C8, p.Wo, p.nseg, p.TH, p.Ho);
    const int c0 = th.chunk * CPT;
    const DwStream a = {p.x, p.x_bytes, p.w, p.C, c0, p.scale, p.shift, p.res, p.y, p.H, p.W, p.C, p.Ho, p.Wo, p.pt, p.pl,
                        p.act, p.post_act, p.ovf};
    dw_stream_rows<DT, 5, S, FAST, CPT, true>(a, th, c0);
#endif  // __HIP_DEVICE_COMPILE__
}
