// gconvx.hpp - grouped 3x3 / pad 1 convolution at ANY group width that is a multiple of 8 up to 64 channels (8, 16, 24, 40, 48, 56,
// 64) and any number (>= 2) of groups, stride 1 or stride 2 on even maps, 16-bit storage: conv2 of every RegNetX / RegNetY unit
// (reference regnet.py:60-64, conv3x3_block(groups=mid_channels // group_width) inside RegNetBottleneck; call site
// pytorchcv_amd/models/regnet.py, RegNetUnit.run). Companion of gconv3x3.hpp / gconv3x3r.hpp, which cover ResNeXt's shapes only
// (C % 64 == 0, 4..32 channels per group); RegNet's widths are arbitrary multiples of the group width (24, 56, 152, 368, 888, ...),
// its group counts include primes (19, 13, 37), and on those the generic kernel's group blocking multiplies mostly zero weights.
//   * a tile = GB whole groups (CB = GB Cg channels) x R whole OUTPUT ROWS (R Wo <= 112 pixels = at most seven 16-pixel MFMA
//     blocks). As in gconv3x3r.hpp the input rows of global output row g (= n Ho + ho) are the flat rows S g - 1 .. S g + 1 whatever
//     the image (even H at stride 2), so the tile's window is ONE contiguous pixel range of (S R + 3 - S) W + 2 pixels; it is staged
//     once into LDS ([window pixel][CB channels], pitch an odd number of 16-byte chunks), and an image border is resolved by
//     zeroing the B fragment of a lane whose tap leaves the image;
//   * K of a group = 9 taps x (Cg / 8) eight-channel chunks, tap-major, padded with zero chunks to a multiple of 4 (one MFMA
//     K-step = 4 chunks = 32 values; lane group fq of step ks holds chunk 4 ks + fq): NK = ceil(9 Cg / 32) steps, no zero
//     weights but that pad (Cg = 8: 3 of 12 chunks, 16: 2 of 20, 24: 1 of 28, 40: 3 of 48, 48: 2 of 56, 56: 1 of 64, 64: none);
//   * the output channels of a group are ceil(Cg / 16) slabs of 16 MFMA rows (Cg % 16 == 8: the last slab's upper half is zero
//     weights, never stored). The (group, slab) units of the channel block are dealt to the block's four waves; a wave runs one unit
//     over ALL pixel blocks of the tile, so every weight fragment is read once per block and tile - from L2, in fragment order
//     (9 Cg^2 values per group do not fit in registers beyond Cg = 24) - and is shared by up to seven MFMAs;
//   * tiles are ordered channel block major and spread over the XCDs like gconv3x3r.hpp's.
// Bounds: activations are read once per tile (+ the halo rows, L2 hits) and written once; the weights come from L2 once per tile:
// 9 Cg / (pixels of the window + R Wo) times the activation bytes - 0.4x at Cg = 8, up to 3x at Cg = 64 on a 14 x 14 map.
#pragma once
#include "conv_device.hpp"

struct GConvXParams {
    const void* x;
    const void* w;          // [group][slab][NK][16 rows][32 K]: fragment order (pack_gconvx_kernel)
    void* y;
    const float* scale;
    const float* shift;
    uint32_t x_bytes, w_bytes, y_bytes;
    int Min, Mout;          // input / output pixels of the batch
    int W, Wo, Ho, C;
    int G, GB;              // groups; groups per channel block
    int R, RWo;             // output rows per tile, R * Wo (<= 112)
    int npb;                // 16-pixel blocks of a tile: ceil(RWo / 16) (<= 7)
    int win;                // input pixels of a tile's window
    int pitch;              // bytes of one window pixel in LDS: an odd number of 16-byte chunks >= GB Cg / 8
    FastDiv div_wo, div_ho, div_cpb;    // cpb = GB Cg / 8: 16-byte chunks per staged pixel
    int nRowTiles, nTiles;
    int act;
    uint32_t* ovf;          // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
};

template <int CG> struct GConvXCfg {
    static_assert(CG % 8 == 0 && CG >= 8 && CG <= 64, "8..64 channels per group, whole 16-byte chunks");
    static constexpr int CPG = CG / 8;                    // 16-byte chunks of a group's input channels
    static constexpr int NCH = 9 * CPG;                   // live K chunks
    static constexpr int NK = (NCH + 3) / 4;              // MFMA K-steps
    static constexpr int SL = (CG + 15) / 16;             // 16-row output slabs per group
};
constexpr int kGConvXMaxLds = 48 * 1024;                  // a tile's window: three blocks per CU
constexpr int kGConvXPB[2] = {4, 7};                      // 16-pixel blocks of a tile: the two instantiations (64 / 112 pixels)

template <int DT, int S, int CG, int PB>
__global__ __launch_bounds__(256, 2) void gconvx_kernel(const GConvXParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(DT != PCV_F32 && (S == 1 || S == 2), "16-bit storage; stride 1 or 2");
    typedef GConvXCfg<CG> G;
    typedef typename Mma<DT>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [win pixels][pitch bytes]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    const int perXcd = (p.nTiles + 7) >> 3;
    const int xcd = blockIdx.x & 7;
    const int tstride = gridDim.x >> 3;
    const int tend = min(p.nTiles, (xcd + 1) * perXcd);

    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(p.w, p.w_bytes);
    const __amdgpu_buffer_rsrc_t yrsrc = buffer_rsrc(p.y, p.y_bytes);
    const int cpb = (int)p.div_cpb.d;

    // ---- this lane's K chunks: step ks holds chunk j = 4 ks + fq = (tap j / CPG, channel chunk j % CPG); the tap's byte offset
    //      inside the window and, one bit per step, which border kills it (a pad chunk is always killed: its weights are zero,
    //      but what its lane would read need not be finite)
    int toff[G::NK];
    uint32_t m_pad = 0, m_r0 = 0, m_r2 = 0, m_q0 = 0, m_q2 = 0;
#pragma unroll
    for (int ks = 0; ks < G::NK; ++ks) {
        const int j = 4 * ks + fq;
        const bool live = j < G::NCH;
        const int tap = live ? j / G::CPG : 0;
        const int cc = live ? j - tap * G::CPG : 0;
        const int r = tap / 3, q = tap - 3 * r;
        toff[ks] = (r * p.W + q) * p.pitch + cc * 16;
        m_pad |= (live ? 0u : 1u) << ks;
        m_r0 |= (r == 0 ? 1u : 0u) << ks;
        m_r2 |= (r == 2 ? 1u : 0u) << ks;
        m_q0 |= (q == 0 ? 1u : 0u) << ks;
        m_q2 |= (q == 2 ? 1u : 0u) << ks;
    }
    // ---- this lane's output pixel in every pixel block of a tile (the same for every tile: tiles are whole rows): window pixel of
    //      its tap (0, 0) and the row of the tile it sits in; a lane beyond the tile's pixels computes the last pixel again
    int xoff[PB], hol[PB];
    uint32_t m_col[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        const int ml = min(pb * 16 + fr, p.RWo - 1);
        const int ho_l = (int)fastdiv((uint32_t)ml, p.div_wo);
        const int wo = ml - ho_l * p.Wo;
        hol[pb] = ho_l;
        xoff[pb] = (S * ho_l * p.W + S * wo) * p.pitch;
        // (stride 2, even W: column 2 wo + 1 is always inside)
        m_col[pb] = m_pad | (wo == 0 ? m_q0 : 0u) | ((S == 1 && wo == p.W - 1) ? m_q2 : 0u);
    }
    const ActClamp act = make_act(p.act);

#pragma nounroll
    for (int tile = xcd * perXcd + (int)(blockIdx.x >> 3); tile < tend; tile += tstride) {     // (block-uniform bounds)
        const int cb = tile / p.nRowTiles;
        const int g0 = (tile - cb * p.nRowTiles) * p.R;        // first global output row
        const int grp0 = cb * p.GB;                            // first group of the channel block
        const int glive = min(p.GB, p.G - grp0);               // its groups (the last block may be partial)
        const int ch0 = grp0 * CG;

        // ---- stage the window: pixel c' of it = flat input pixel cbase + c'; a pixel outside the batch and a chunk beyond the
        //      block's channels read zeros (an out-of-range buffer offset)
        __syncthreads();                                       // the previous tile's reads are done
        {
            const int cbase = (S * g0 - 1) * p.W - 1;
            const int total = p.win * cpb;
            const int clive = glive * G::CPG;
#pragma nounroll
            for (int i0 = tid; i0 < total; i0 += 4 * 256) {
                u32x4 v[4];
                int dst[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * 256;
                    const int px = (int)fastdiv((uint32_t)min(i, total - 1), p.div_cpb);
                    const int ck = min(i, total - 1) - px * cpb;
                    const int c = cbase + px;
                    const bool ok = i < total && ck < clive && c >= 0 && c < p.Min;
                    dst[u] = i < total ? px * p.pitch + ck * 16 : -1;
                    v[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                        xrsrc, ok ? (uint32_t)((c * p.C + ch0 + ck * 8) * 2) : kOutOfRange, 0, 0));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (dst[u] >= 0) *reinterpret_cast<u32x4*>(smem + dst[u]) = v[u];
            }
        }
        __syncthreads();

        // ---- this tile's border masks: the image row of each pixel block's output row
        uint32_t kill[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            const uint32_t grow = (uint32_t)(g0 + hol[pb]);
            const int gh = (int)(grow - fastdiv(grow, p.div_ho) * (uint32_t)p.Ho);
            // (stride 2, even H: row 2 ho + 1 is always inside)
            kill[pb] = m_col[pb] | (gh == 0 ? m_r0 : 0u) | ((S == 1 && gh == p.Ho - 1) ? m_r2 : 0u);
        }

        // ---- the (group, slab) units of the channel block, dealt to the waves
        const int nunits = glive * G::SL;
#pragma nounroll
        for (int u = wave; u < nunits; u += 4) {               // (wave-uniform)
            const int gl = u / G::SL, sl = u - gl * G::SL;
            const int grp = grp0 + gl;
            auto wfrag = [&](int ks) {
                return __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(
                    wrsrc, (uint32_t)(((((grp * G::SL + sl) * G::NK + ks) * 16 + fr) * 32 + 8 * fq) * 2), 0, 0));
            };
            // output channels 4 fq .. 4 fq + 3 of the slab: beyond the group in the upper half of a half-filled last slab
            const bool rows_ok = sl * 16 + 4 * fq < CG;
            const int ch = rows_ok ? grp * CG + sl * 16 + 4 * fq : 0;
            const f32x4 sc = p.scale ? *reinterpret_cast<const f32x4*>(p.scale + ch) : (f32x4){1.f, 1.f, 1.f, 1.f};
            const f32x4 sf = p.shift ? *reinterpret_cast<const f32x4*>(p.shift + ch) : (f32x4){0.f, 0.f, 0.f, 0.f};

            f32x4 acc[PB];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) acc[pb] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // this unit's window addresses and tap masks, opaque to the optimiser: hoisted out of the unit loop, the PB x NK sums and
            // masks (invariant from tile to tile) would take more registers than the kernel has
            int xa[PB];
            uint32_t live[PB];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                xa[pb] = xoff[pb] + gl * (CG * 2);
                live[pb] = ~kill[pb];
                asm volatile("" : "+v"(xa[pb]), "+v"(live[pb]));
            }
            // the weights run two steps ahead of the MFMAs that use them (L2 latency under two steps' LDS reads and MFMAs)
            frag a0 = wfrag(0), a1 = wfrag(G::NK > 1 ? 1 : 0);
#pragma unroll
            for (int ks = 0; ks < G::NK; ++ks) {
                const frag a = a0;
                a0 = a1;
                if (ks + 2 < G::NK) a1 = wfrag(ks + 2);
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    u32x4 b = *reinterpret_cast<const u32x4*>(smem + xa[pb] + toff[ks]);
                    const uint32_t keep = (uint32_t)__builtin_amdgcn_sbfe((int)live[pb], ks, 1);     // all ones, or zero for a killed tap
                    b &= (u32x4){keep, keep, keep, keep};
                    acc[pb] = Mma<DT>::run(a, __builtin_bit_cast(frag, b), acc[pb]);
                }
                __builtin_amdgcn_sched_barrier(0);             // (keeps the LDS reads of later steps from piling up in registers)
            }

            // ---- epilogue: MFMA rows 4 fq + e = channels ch + e, output pixel g0 Wo + 16 pb + fr: 8-byte stores
            F16Guard<DT> guard;
            bool any = false;
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                {
                    const int ml = pb * 16 + fr;
                    const int m = g0 * p.Wo + ml;
                    const bool ok = rows_ok && ml < p.RWo && m < p.Mout;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[pb][e] * sc[e] + sf[e];
                    apply_actn(v, act);
                    if (ok) guard.see(v);
                    any |= ok;
                    u32x2 o = {pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3])};
                    __builtin_amdgcn_raw_buffer_store_b64(o, yrsrc, ok ? (uint32_t)((m * p.C + ch) * 2) : kOutOfRange, 0, 0);
                }
            }
            guard.commit(p.ovf, any);
        }
    }
#endif  // __HIP_DEVICE_COMPILE__
}

// ---- weight packing: w fp32 [C][Cg][3][3] -> [C / Cg groups][SL slabs][NK steps][16 rows][32 K]; row = output channel 16 slab + row
//      of the group, K element k of step ks = chunk j = 4 ks + k / 8 -> (tap j / CPG, input channel 8 (j % CPG) + k % 8); zeros in the
//      rows beyond the group and in the pad chunks -----------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void pack_gconvx_kernel(const float* __restrict__ w, void* __restrict__ out, int groups, int Cg) {
    const int cpg = Cg / 8, nk = (9 * cpg + 3) / 4, sl = (Cg + 15) / 16;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)groups * sl * nk * 16 * 32;
    if (i >= total) return;
    const int k = (int)(i & 31);
    const int row = (int)((i >> 5) & 15);
    const long f = i >> 9;                     // (group, slab, step)
    const int ks = (int)(f % nk);
    const int s = (int)((f / nk) % sl);
    const int g = (int)(f / ((long)nk * sl));
    const int j = 4 * ks + (k >> 3);
    const int o = s * 16 + row;
    float v = 0.f;
    if (j < 9 * cpg && o < Cg) {
        const int tap = j / cpg, ci = (j - tap * cpg) * 8 + (k & 7);
        v = w[(((size_t)g * Cg + o) * Cg + ci) * 9 + tap];
    }
    store_elem<DT>(out, (size_t)i, v);
}

// total 16-bit elements of the packed blob
static inline long long gconvx_packed_elems(int groups, int Cg) {
    const int cpg = Cg / 8;
    return (long long)groups * ((Cg + 15) / 16) * ((9 * cpg + 3) / 4) * 16 * 32;
}

// every instantiation: (storage type) x (stride 1, 2) x (channels per group); defined in gconvx_bf16.hip / gconvx_f16.hip
#define GCONVX_WIDTHS(X, DT, S, PB) \
    X(DT, S, 8, PB) X(DT, S, 16, PB) X(DT, S, 24, PB) X(DT, S, 40, PB) X(DT, S, 48, PB) X(DT, S, 56, PB) X(DT, S, 64, PB)
#define GCONVX_INSTANCES(X, DT) GCONVX_WIDTHS(X, DT, 1, 4) GCONVX_WIDTHS(X, DT, 2, 4) GCONVX_WIDTHS(X, DT, 1, 7) GCONVX_WIDTHS(X, DT, 2, 7)
#define GCONVX_DECLARE(DT, S, CG, PB) extern template __global__ void gconvx_kernel<DT, S, CG, PB>(const GConvXParams);
#define GCONVX_DEFINE(DT, S, CG, PB) template __global__ void gconvx_kernel<DT, S, CG, PB>(const GConvXParams);
