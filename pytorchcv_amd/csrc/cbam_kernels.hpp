// cbam_kernels.hpp - the CBAM block (reference pytorchcv/models/cbamresnet.py:48-128) as four HBM-bound launches over the
// NHWC output x [N, HW, C] of a unit body; everything between the launches is fp32:
//   cbam_pool_kernel          s[N][2][C]   = (mean_HW x, max_HW x)                              reads x once
//   se_fc_kernel + cbam_gate_kernel  gate[N][C] = sigmoid(fc2(relu(fc1(mean))) + fc2(relu(fc1(max))))   no pass over x
//   cbam_spatial_pool_kernel  p[N][HW][2]  = (max_c, mean_c) of x * gate                        reads x once, writes 8 bytes per pixel
//   cbam_apply_kernel         y = post_act((x * gate) * sigmoid(bn(conv7x7(p))) + residual)     reads x (+ residual), writes y
// The channel-gated tensor never exists in memory: three reads of x and one write of y per block.
// Every maximum is gfx950's IEEE-754-2019 maximum (__builtin_elementwise_maximum, as maxpool_kernel): it PROPAGATES NaN like
// AdaptiveMaxPool2d and torch.max(dim); fmaxf would return the other operand and hide a NaN activation.
#pragma once
#include "pcv_common.hpp"

// ---- ChannelGate pools (cbamresnet.py:64-65,72,74): spatial_mean_kernel's structure with a second running value ---------------
// One 512-thread block per (image, group of <= 512 channel chunks), threads tile [rows x chunks], rows meet in LDS in row order: an
// image's result depends on that image only, in a fixed order - no atomics, no cross-block reduction. The mean is computed by the
// same operations in the same order as spatial_mean_kernel's (s[n][0] has pcv_se_squeeze's bits).
template <int DT>
__global__ __launch_bounds__(512) void cbam_pool_kernel(const void* __restrict__ x, float* __restrict__ s, int HW, int C) {
    __shared__ float part[512][9];                       // +1: the row reads below walk it with a stride of Gc rows
    const int n = blockIdx.x;
    const int C8 = C >> 3;
    const int g0 = blockIdx.y * 512;
    const int Gc = min(512, C8 - g0);                    // chunks of this group
    const int R = 512 / Gc;                              // rows in flight
    const int t = threadIdx.x;
    const int r = t / Gc, c = t - r * Gc;
    float a[8], m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = 0.f;
        m[e] = -INFINITY;
    }
    if (r < R) {
        const size_t base = (size_t)n * HW * C + (size_t)(g0 + c) * 8;
#pragma unroll 4
        for (int hw = r; hw < HW; hw += R) {
            float v[8];
            load8<DT>(x, base + (size_t)hw * C, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a[e] += v[e];
                m[e] = __builtin_elementwise_maximum(m[e], v[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[t][e] = a[e];
    __syncthreads();
    if (t < Gc) {
        const float inv = 1.f / (float)HW;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += part[q * Gc + t][e];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] *= inv;
        store8<PCV_F32>(s, (size_t)n * 2 * C + (size_t)(g0 + t) * 8, a);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) part[t][e] = m[e];        // idle rows (r >= R) hold -inf, the identity
    __syncthreads();
    if (t < Gc) {
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = __builtin_elementwise_maximum(m[e], part[q * Gc + t][e]);
        store8<PCV_F32>(s, (size_t)n * 2 * C + C + (size_t)(g0 + t) * 8, m);
    }
}

// ---- ChannelGate second layer (cbamresnet.py:73,75-77): gate[n][c] = sigmoid((W2 . mid[n][0] + b2) + (W2 . mid[n][1] + b2)) --
// mid [N][2][M] is relu(fc1) of the mean and of the max row (se_fc_kernel over 2N rows). One thread = one output channel for the 8
// images of the block (every weight fetched is used 16 times); the hidden rows are LDS broadcasts staged 128 columns at a time.
// Each image slot is one explicit fma chain over k = 0 .. M-1, so an image's gate does not depend on its batch position, bit for bit.
__global__ __launch_bounds__(256) void cbam_gate_kernel(const float* __restrict__ mid, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, float* __restrict__ gate, int N, int C, int M) {
    constexpr int IMG = 8, KC = 128;
    __shared__ float sm[IMG][2][KC];
    const int t = threadIdx.x;
    const int c = blockIdx.x * 256 + t;
    const int n0 = blockIdx.y * IMG;
    float aa[IMG], am[IMG];
#pragma unroll
    for (int i = 0; i < IMG; ++i) aa[i] = am[i] = 0.f;
    for (int kc = 0; kc < M; kc += KC) {
        const int kn = min(KC, M - kc);
        if (kc > 0) __syncthreads();
        for (int i = t; i < IMG * 2 * kn; i += 256) {
            const int row = i / kn, k = i - row * kn;            // row = 2 * img + half
            sm[row >> 1][row & 1][k] = n0 + (row >> 1) < N ? mid[((size_t)n0 * 2 + row) * M + kc + k] : 0.f;
        }
        __syncthreads();
        if (c < C) {
            const float* wr = w2 + (size_t)c * M + kc;
            for (int k = 0; k < kn; ++k) {
                const float wv = wr[k];
#pragma unroll
                for (int i = 0; i < IMG; ++i) {
                    aa[i] = fmaf(wv, sm[i][0][k], aa[i]);
                    am[i] = fmaf(wv, sm[i][1][k], am[i]);
                }
            }
        }
    }
    if (c < C) {
        const float b = b2[c];
#pragma unroll
        for (int i = 0; i < IMG; ++i)
            if (n0 + i < N) gate[(size_t)(n0 + i) * C + c] = apply_act((aa[i] + b) + (am[i] + b), PCV_ACT_SIGMOID);
    }
}

// ---- SpatialGate pools (cbamresnet.py:96-98) of the channel-gated tensor: p[n][q] = (max_c, mean_c) of x[n][q][c] * gate[n][c] --
// The product is formed in fp32 registers and never stored. A pixel gets LP lanes (LP = min(64, C / 8) rounded up to a power of two:
// the lanes of a pixel are one aligned group of a wave), lane j takes the 8-channel chunks j, j + LP, ...; the lanes meet by an xor
// butterfly (LP / 2, ..., 1), the same order for every pixel. A block owns `ppb` consecutive pixels of ONE image (`bpi` blocks per
// image) and stages that image's gate in LDS once (C <= 2048; a wider gate is read through the cache). Lanes past C / 8 carry (0, -inf).
constexpr int kCbamGateLds = 2048;
template <int DT>
__global__ __launch_bounds__(256) void cbam_spatial_pool_kernel(const void* __restrict__ x, const float* __restrict__ gate,
                                                               float* __restrict__ p, int HW, int C, int LP, int ppb, int bpi) {
    __shared__ __attribute__((aligned(16))) float sg[kCbamGateLds];
    const int t = threadIdx.x;
    const int n = blockIdx.x / bpi;
    const int C8 = C >> 3;
    const float* gn = gate + (size_t)n * C;
    const bool staged = C <= kCbamGateLds;
    if (staged) {
        for (int i = t; i < C8 * 2; i += 256)
            *reinterpret_cast<f32x4*>(&sg[i * 4]) = *reinterpret_cast<const f32x4*>(gn + i * 4);
        __syncthreads();
    }
    const int slots = 256 / LP;                          // pixels in flight
    const int slot = t / LP, j = t - slot * LP;
    const int q0 = (blockIdx.x - n * bpi) * ppb;
    const int q1 = min(HW, q0 + ppb);
    const float invC = 1.f / (float)C;
    // every lane of a group runs the same trip count (the butterfly below needs the whole group)
    for (int q = q0 + slot; q < q1; q += slots) {
        const size_t base = ((size_t)n * HW + q) * C;
        float sum = 0.f, mx = -INFINITY;
        for (int ch = j; ch < C8; ch += LP) {
            float v[8], g[8];
            load8<DT>(x, base + (size_t)ch * 8, v);
            if (staged) {
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(&sg[ch * 8]), g1 = *reinterpret_cast<const f32x4*>(&sg[ch * 8 + 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    g[e] = g0[e];
                    g[4 + e] = g1[e];
                }
            } else {
                load8<PCV_F32>(gn, (size_t)ch * 8, g);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float pr = v[e] * g[e];
                sum += pr;
                mx = __builtin_elementwise_maximum(mx, pr);
            }
        }
        for (int o = LP >> 1; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            mx = __builtin_elementwise_maximum(mx, __shfl_xor(mx, o, 64));
        }
        if (j == 0) *reinterpret_cast<f32x2*>(p + ((size_t)n * HW + q) * 2) = (f32x2){mx, sum * invC};      // cat order: max first
    }
}

// ---- SpatialGate convolution + both multiplications + the unit's tail (cbamresnet.py:99-101, 79, 181-182) ---------------------
// sg[n,h,w] = sigmoid(scale * conv7x7(p, w7, pad 3)[n,h,w] + shift); y = post_act((x * gate[n,c]) * sg[n,h,w] + residual), the
// reference's multiplication order, one rounding. A tile is R rows x CW columns of one image with CW == W or R == 1, i.e. a run of
// consecutive pixels holding about 8 K elements (four 16-byte chunks per thread). A block
//   1. issues the loads of its first four chunks of x and of the residual (raw, they stay in the registers the loads wrote),
//   2. stages the tile's p halo (R + 6) x (CW + 6) in LDS (zeros outside the map = the convolution's padding),
//   3. computes the tile's R * CW gate values there: 16 lanes per pixel, lane k < 14 owns filter row (channel k / 7, dy = k % 7) as
//      one fma chain over dx with its seven taps in registers, the rows meet by an xor butterfly (8, 4, 2, 1) - a fixed order,
//   4. finishes the chunks it holds and streams what is left of the run (only when a pixel is wider than the tile budget).
// The memory latency of step 1 hides steps 2 and 3. Tiles are walked grid-stride (one tile per block unless the test cap shrinks
// the grid).
constexpr int kCbamTilePix = 256;                        // pixels a tile may hold
constexpr int kCbamHalo = 2048;                          // p pixels (float2) of a tile's halo: (R + 6)(CW + 6) <= 1834 when R CW <= 256
constexpr int kCbamPrefetch = 4;                         // chunks per thread in flight before the gate is computed (16-bit)
struct CbamApplyParams {
    const void* x;
    const float* gate;
    const float* p;
    const float* w7;
    const float* scale;                                  // [1] each: the folded BatchNorm of the 1-channel convolution
    const float* shift;
    const void* res;
    void* y;
    int H, W, C, R, CW, tiles_h, tiles_w;
    long tiles;                                          // N * tiles_h * tiles_w
    int post_act;
    uint32_t* ovf;
};
template <int DT> struct CbamRaw8 {                      // 8 channels as they come from memory
    u32x4 q[DT == PCV_F32 ? 2 : 1];
    __device__ __forceinline__ void load(const void* base, size_t eidx) {
        if constexpr (DT == PCV_F32) {
            q[0] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(base) + eidx);
            q[1] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(base) + eidx + 4);
        } else {
            q[0] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(base) + eidx);
        }
    }
    __device__ __forceinline__ void unpack(float (&v)[8]) const {
        if constexpr (DT == PCV_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = __uint_as_float(q[0][e]);
                v[4 + e] = __uint_as_float(q[1][e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) unpack2<DT>(q[0][e], v[2 * e], v[2 * e + 1]);
        }
    }
};
template <int DT>
__global__ __launch_bounds__(256, 4) void cbam_apply_kernel(const CbamApplyParams q) {      // 4 waves per SIMD: at most 128 registers
    __shared__ f32x2 sp[kCbamHalo];
    __shared__ float ssg[kCbamTilePix];
    constexpr int U = DT == PCV_F32 ? kCbamPrefetch / 2 : kCbamPrefetch;      // fp32 chunks are two registers wider: half of them held, the rest streamed
    const int t = threadIdx.x;
    const int C8 = q.C >> 3;
    const int HW = q.H * q.W;
    const ActClamp pact = make_act(q.post_act);
    const bool has_res = q.res != nullptr;
    const float scale = q.scale[0], shift = q.shift[0];
    // the stencil's lane roles: 16 lanes per pixel, lane k < 14 holds filter row k = (channel, dy)
    const int k = t & 15, kch = k >= 7 ? 1 : 0, kdy = k - 7 * kch;
    float wk[7];
#pragma unroll
    for (int dx = 0; dx < 7; ++dx) wk[dx] = k < 14 ? q.w7[k * 7 + dx] : 0.f;
    F16Guard<DT> guard;
    for (long tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
        const int tw = (int)(tile % q.tiles_w);
        const long tq = tile / q.tiles_w;
        const int th = (int)(tq % q.tiles_h);
        const int n = (int)(tq / q.tiles_h);
        const int r0 = th * q.R, c0 = tw * q.CW;
        const int rows = min(q.R, q.H - r0), cols = min(q.CW, q.W - c0);
        const int hw = cols + 6, hh = rows + 6;
        const int npix = rows * cols;
        // rows x cols is a run of consecutive pixels (cols == W, or one row)
        const size_t pix0 = (size_t)n * HW + (size_t)r0 * q.W + c0;
        const int total8 = npix * C8;
        // 1. the first U chunks of this thread
        CbamRaw8<DT> xr[U], rr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = t + u * 256;
            if (i < total8) {
                const int lp = i / C8, c8 = i - lp * C8;
                const size_t e0 = (pix0 + lp) * q.C + (size_t)c8 * 8;
                xr[u].load(q.x, e0);
                if (has_res) rr[u].load(q.res, e0);
            }
        }
        // 2. the halo
        __syncthreads();                                 // the previous tile's readers of sp / ssg are done
        const float* pn = q.p + (size_t)n * HW * 2;
        for (int i = t; i < hh * hw; i += 256) {
            const int hr = i / hw, hc = i - hr * hw;
            const int r = r0 - 3 + hr, c = c0 - 3 + hc;
            f32x2 v = {0.f, 0.f};
            if ((unsigned)r < (unsigned)q.H && (unsigned)c < (unsigned)q.W) v = *reinterpret_cast<const f32x2*>(pn + ((size_t)r * q.W + c) * 2);
            sp[i] = v;
        }
        __syncthreads();
        // 3. the gate values: 16 pixels per round, every lane takes part in the butterfly
        const float* spf = reinterpret_cast<const float*>(sp);
        for (int base = 0; base < npix; base += 16) {
            const int lp = base + (t >> 4);
            float a = 0.f;
            if (lp < npix && k < 14) {
                const int r = lp / cols, c = lp - r * cols;
                const float* row = spf + ((r + kdy) * hw + c) * 2 + kch;
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) a = fmaf(wk[dx], row[2 * dx], a);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if (k == 0 && lp < npix) ssg[lp] = apply_act(fmaf(scale, a, shift), PCV_ACT_SIGMOID);
        }
        __syncthreads();
        // 4. the chunks in registers, then the rest of the run
        const float* gn = q.gate + (size_t)n * q.C;
        auto finish = [&](int i, const CbamRaw8<DT>& xq, const CbamRaw8<DT>& rq) {
            const int lp = i / C8, c8 = i - lp * C8;
            const size_t e0 = (pix0 + lp) * q.C + (size_t)c8 * 8;
            float v[8], g[8];
            xq.unpack(v);
            load8<PCV_F32>(gn, (size_t)c8 * 8, g);
            const float s = ssg[lp];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (v[e] * g[e]) * s;
            if (has_res) {
                float w[8];
                rq.unpack(w);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += w[e];
            }
            if (q.post_act != PCV_ACT_NONE) apply_act8(v, pact);
            guard.see(v);
            store8<DT>(q.y, e0, v);
        };
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = t + u * 256;
            if (i < total8) finish(i, xr[u], rr[u]);
        }
        for (int i = t + U * 256; i < total8; i += 256) {
            const int lp = i / C8, c8 = i - lp * C8;
            const size_t e0 = (pix0 + lp) * q.C + (size_t)c8 * 8;
            CbamRaw8<DT> xq, rq;
            xq.load(q.x, e0);
            if (has_res) rq.load(q.res, e0);
            finish(i, xq, rq);
        }
    }
    guard.commit(q.ovf);
}
