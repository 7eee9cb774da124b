// ghost.hpp - the second half of GhostNet's ghost module as ONE launch: cheap depthwise 3x3 + channel concatenation + skip add.
//
// Replaces: `y = self.cheap_conv(x); return torch.cat((x, y), dim=1)` of GhostConvBlock.forward (reference
//           pytorchcv/models/ghostnet.py:57-60, cheap_conv = dwconv3x3_block: Conv2d(groups=C) + BatchNorm2d(eval) + activation) and,
//           for the unit's last ghost module, the `x = x + identity` of GhostUnit.forward (ghostnet.py:167-174).
//
//   m   NHWC [N, H, W, CP], CP = round8(Cm): the main convolution's output, Cm logical channels (pad channels are never read)
//   y   NHWC [N, H, W, 2 Cm] dense, res (optional) the same shape:
//         y[.., c]      = m[.., c]                                       + res[.., c]           c in [0, Cm)
//         y[.., Cm + c] = act(scale[c] * dw3x3(m)[.., c] + shift[c])     + res[.., Cm + c]
//
// HBM-bound like dwconv.hpp and built from the same parts (dw_device.hpp: chunk loads, loadn / storen, packed fp32): one thread owns FOUR consecutive channels (Cm % 4 == 0 is all the net's widths
// share: 12, 20, 36, 60, 92, 100 are no multiples of 8) of one column and walks down a strip of rows with the 3x3 fp32 window in
// registers. Per row: one new input row through range-checked buffer loads (a tap outside the image is an offset beyond num_records
// and reads zeros, no branches), requested three rows ahead; two stores, the window's centre (+ res) into [c, c + 4) and the cheap
// result (+ res) into [Cm + c, Cm + c + 4). A 4-channel chunk never straddles the main / cheap boundary, so no offset needs a special
// case. Lanes run over channel chunks first, then columns: a wave's loads and each of its two store streams are contiguous NHWC spans.
// Without res the main half is a bit copy of m for every finite value (16-bit -> fp32 -> 16-bit is exact).
#pragma once
#include "dw_device.hpp"

struct GhostParams {
    const void* m;
    const void* w;        // [9][CP] in DT: the first part of pcv_dwconv_pack's blob for round8(Cm) channels
    const void* res;
    void* y;
    const float* scale;   // [CP]
    const float* shift;
    uint32_t x_bytes;     // buffer num_records of m
    int N, H, W;
    int Cm, CP;           // logical channels of m (= of each half of y), channel pitch of m / taps / scale / shift
    int C4;               // Cm / 4
    int TH;               // output rows per thread
    int nseg;             // ceil(H / TH)
    int act;              // cheap half only
    long total;           // N * nseg * W * C4
    int flags;            // dw_flags: bit 0 = non-temporal output stores, bit 1 = blocks in dispatch order (no XCD remap)
    uint32_t* ovf;        // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
};

// FAST: the cheap activation is none / relu / relu6 (dwconv.hpp)
template <int DT, bool FAST>
__global__ __launch_bounds__(256, 2) void ghost_dw_kernel(const GhostParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int KS = 3, CPT = 4, NV = 2, PD = 3;          // PD: prefetch depth in rows = the window's rotation period
    constexpr int ES = Elem<DT>::BYTES;
    const long idx = (long)((p.flags & 2) ? blockIdx.x : xcd_remap(blockIdx.x, gridDim.x)) * 256 + threadIdx.x;      // (see dwconv_kernel)
    if (idx >= p.total) return;
    const DwThread th = dw_decode(idx, p.C4, p.W, p.nseg, p.TH, p.H);
    const int n = th.n, wo = th.wo, c0 = th.chunk * CPT, ho_begin = th.ho_begin, ho_end = th.ho_end;

    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(p.m, p.x_bytes);

    f32x2 wgt[KS * KS][NV];
#pragma unroll
    for (int k = 0; k < KS * KS; ++k) {
        float w4[CPT];
        loadn<DT, CPT>(p.w, (size_t)k * p.CP + c0, w4);
#pragma unroll
        for (int e = 0; e < NV; ++e) wgt[k][e] = (f32x2){w4[2 * e], w4[2 * e + 1]};
    }
    f32x2 sc[NV], sf[NV];
    {
        float a4[CPT], b4[CPT];
        loadn<PCV_F32, CPT>(p.scale, c0, a4);
        loadn<PCV_F32, CPT>(p.shift, c0, b4);
#pragma unroll
        for (int e = 0; e < NV; ++e) { sc[e] = (f32x2){a4[2 * e], a4[2 * e + 1]}; sf[e] = (f32x2){b4[2 * e], b4[2 * e + 1]}; }
    }
    const ActClamp act = make_act(p.act);

    // per-column byte offsets (relative to the row start) or "invalid"
    uint32_t coloff[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q)
        coloff[q] = (unsigned)(wo - 1 + q) < (unsigned)p.W ? (uint32_t)(((wo - 1 + q) * p.CP + c0) * ES) : kOutOfRange;
    const uint32_t rowbytes = (uint32_t)(p.W * p.CP * ES);
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

    f32x2 win[KS][KS][NV];               // slot-indexed rows: row r of the current window lives in slot (r + phase) % 3
    RawChunk<DT, CPT> raw[PD][KS];       // ring: raw[t % PD] holds the new (bottom) row of output row t of the strip

    // prologue: the two rows shared with the first output row go straight into the window; the bottom rows of the first PD output
    // rows are requested up front (rows beyond this thread's strip are not requested: offset forced invalid through hi = -1)
    const int hi_first = ho_begin - 1;
    {
        RawChunk<DT, CPT> tmp[2][KS];
        fetch_row(hi_first, tmp[0]);
        fetch_row(hi_first + 1, tmp[1]);
#pragma unroll
        for (int d = 0; d < PD; ++d) fetch_row(ho_begin + d < ho_end ? hi_first + d + 2 : -1, raw[d]);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < KS; ++q) raw_to_f32x2<DT, CPT>(tmp[r][q], win[r][q]);
    }

    const bool has_res = p.res != nullptr;
    const bool nt = (p.flags & 1) != 0;
    const bool bounded = !has_res && (act_bounded(p.act) || p.act == PCV_ACT_CLAMP01);
    const size_t C2 = 2 * (size_t)p.Cm;
    int ho = ho_begin;
    F16Guard<DT> guard;
    while (ho < ho_end) {
        static_for<KS>([&](auto PHC) {
            constexpr int PH = decltype(PHC)::value;
            if (ho < ho_end) {
#pragma unroll
                for (int q = 0; q < KS; ++q) raw_to_f32x2<DT, CPT>(raw[PH][q], win[(2 + PH) % KS][q]);
                // refill the slot with the bottom row of output row ho + PD before doing this row's arithmetic
                fetch_row(ho + PD < ho_end ? ho + PD + 1 : -1, raw[PH]);
                f32x2 acc[NV];
#pragma unroll
                for (int e = 0; e < NV; ++e) acc[e] = pk_mul(win[PH % KS][0][e], wgt[0][e]);
#pragma unroll
                for (int r = 0; r < KS; ++r)
#pragma unroll
                    for (int q = 0; q < KS; ++q) {
                        if (r == 0 && q == 0) continue;
#pragma unroll
                        for (int e = 0; e < NV; ++e) pk_fma_acc(acc[e], win[(r + PH) % KS][q][e], wgt[r * KS + q][e]);
                    }

                const size_t eoff = (((size_t)n * p.H + ho) * p.W + wo) * C2 + c0;
                float v[CPT], u[CPT];
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    f32x2 t2 = sf[e];
                    pk_fma_acc(t2, acc[e], sc[e]);
                    v[2 * e] = t2[0];
                    v[2 * e + 1] = t2[1];
                    const f32x2 ctr = win[(1 + PH) % KS][1][e];          // the window's centre: m itself
                    u[2 * e] = ctr[0];
                    u[2 * e + 1] = ctr[1];
                }
                dw_act<FAST>(v, act);
                if (has_res) {
                    float r4[CPT], s4[CPT];
                    loadn<DT, CPT>(p.res, eoff, r4);
                    loadn<DT, CPT>(p.res, eoff + p.Cm, s4);
#pragma unroll
                    for (int e = 0; e < CPT; ++e) { u[e] += r4[e]; v[e] += s4[e]; }
                    guard.see(u);                                        // (without res the main half stores what m already held)
                }
                if (!bounded) guard.see(v);
                // (dw_flags bit 0 reaches both 4-channel stores here, at every width - unlike the 5x5 and MixConv stores: kept)
                storen<DT, CPT>(p.y, eoff, u, nt);
                storen<DT, CPT>(p.y, eoff + p.Cm, v, nt);
                ++ho;
            }
        });
    }
    guard.commit(p.ovf);
#endif  // __HIP_DEVICE_COMPILE__
}

#define GHOST_INSTANCES(X, DT) X(DT, true) X(DT, false)
#define GHOST_DECLARE(DT, FAST) extern template __global__ void ghost_dw_kernel<DT, FAST>(const GhostParams);
#define GHOST_DEFINE(DT, FAST) template __global__ void ghost_dw_kernel<DT, FAST>(const GhostParams);
