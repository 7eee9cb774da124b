// instnorm.hpp - nn.InstanceNorm2d(affine=True) at inference on the leading Cn of C channels, with the activation behind it
// (IBN, common/norm.py:118-162 of the reference; the b-variant's whole-tensor norms, ibnbresnet.py). NHWC [N, HW, xpitch]:
//     c <  Cn : y = act(gamma[c] * (x - mean[n, c]) * rsqrt(var[n, c] + eps) + beta[c])      mean / biased var over the HW positions
//     c >= Cn : y = act(x)                                                                   (the producing convolution folded the BN)
// The statistics belong to the image in flight, so nothing folds at load time: two launches.
//   instnorm_stats_kernel  x -> ws[n][c] = (a, b),  a = gamma * rstd,  b = beta - mean * a      (fp32 pairs, [N, Cn, 2])
//   instnorm_apply_kernel  y = act(x * a + b)  - bn_act_kernel with per-(image, channel) coefficients
#pragma once
#include "pcv_common.hpp"

constexpr int kInGroup = 8;        // 8-channel chunks per statistics block: 64 channels, one 128-byte line per pixel at 16 bit
constexpr int kInThreads = 512;

// (count, mean, M2 = sum of squared deviations) of two disjoint sample sets -> of their union (Chan et al.). Exact for equal means
// (a constant plane keeps M2 == 0); an empty side leaves the other untouched; a NaN on either side stays.
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; qa = qb; return; }
    const float n = na + nb;
    const float d = mb - ma;
    const float f = nb / n;
    ma = ma + d * f;
    qa = (qa + qb) + (d * d) * (na * f);
    na = n;
}

// One 512-thread block per (image, group of <= kInGroup chunks), threads tiled [rows x chunks] as in spatial_mean_kernel: with Gc
// chunks the block reads 512 / Gc pixels' worth of the group per iteration, so that Cn = 32 keeps every lane on a 16-byte load.
// ONE pass over x: a thread keeps, per channel, the sums of (x - K) and (x - K)^2 with K the first value it sees - the shift
// removes the mean's magnitude from the squares, which is what E[x^2] - mean^2 in fp32 loses (a map of mean 1024 and deviation
// 1 has x^2 ~ 1e6 with a rounding unit of 0.06) - turns them into (count, mean, M2) and the rows meet pairwise in LDS by Chan's
// formula, in a tree whose shape depends on (HW, Gc) only. An image's result depends on that image alone, in a fixed order: no
// atomics, no cross-block reduction; the grid is one block per item (the loop runs more than once under the max_blocks cap only).
template <int DT>
__global__ __launch_bounds__(kInThreads) void instnorm_stats_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float* __restrict__ ws,
                                                                    int HW, int Cn, int xpitch, float eps, int groups,
                                                                    int items) {
    __shared__ float part[kInThreads][17];               // mean[8], M2[8], count; 17: the tree walks it with a stride of Gc rows
    const int t = threadIdx.x;
    const int Cn8 = Cn >> 3;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int n = item / groups;
        const int g0 = (item - n * groups) * kInGroup;
        const int Gc = min(kInGroup, Cn8 - g0);          // chunks of this group
        const int R = kInThreads / Gc;                   // rows in flight
        const int r = t / Gc, c = t - r * Gc;
        float mean[8], m2[8], cnt = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { mean[e] = 0.f; m2[e] = 0.f; }
        if (r < R && r < HW) {
            const size_t base = (size_t)n * HW * xpitch + (size_t)(g0 + c) * 8;
            float k[8], s1[8], s2[8];
            load8<DT>(x, base + (size_t)r * xpitch, k);
#pragma unroll
            for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
            int cn = 1;
#pragma unroll 4
            for (int hw = r + R; hw < HW; hw += R, ++cn) {
                float v[8];
                load8<DT>(x, base + (size_t)hw * xpitch, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = v[e] - k[e];
                    s1[e] += d;
                    s2[e] += d * d;
                }
            }
            cnt = (float)cn;
            const float inv = 1.f / cnt;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float dm = s1[e] * inv;
                const float q = s2[e] - s1[e] * dm;
                mean[e] = k[e] + dm;
                m2[e] = q < 0.f ? 0.f : q;               // (a NaN stays a NaN)
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { part[t][e] = mean[e]; part[t][8 + e] = m2[e]; }
        part[t][16] = cnt;
        __syncthreads();
        int P = 1;
        while (P < R) P <<= 1;
        for (int s = P >> 1; s >= 1; s >>= 1) {          // row r takes row r + s
            if (r < s && r + s < R) {
                const int o = t + s * Gc;
                float nb = part[o][16];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float na = cnt;
                    chan_merge(na, mean[e], m2[e], nb, part[o][e], part[o][8 + e]);
                }
                cnt += nb;
#pragma unroll
                for (int e = 0; e < 8; ++e) { part[t][e] = mean[e]; part[t][8 + e] = m2[e]; }
                part[t][16] = cnt;
            }
            __syncthreads();
        }
        if (r == 0) {
            const int c0 = (g0 + c) * 8;
            float g[8], b[8];
            load8<PCV_F32>(gamma, c0, g);
            load8<PCV_F32>(beta, c0, b);
            const float invn = 1.f / (float)HW;
            float* o = ws + ((size_t)n * Cn + c0) * 2;
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                f32x4 ab;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float var = m2[e + h] * invn;
                    const float a = g[e + h] * (1.f / sqrtf(var + eps));
                    ab[2 * h] = a;
                    ab[2 * h + 1] = b[e + h] - mean[e + h] * a;
                }
                *reinterpret_cast<f32x4*>(o + 2 * e) = ab;
            }
        }
        __syncthreads();                                 // `part` is free for the next item
    }
}

// y = act(x * a[n, c] + b[n, c]) below Cn, act(x) from Cn on; y dense. HBM-bound, 16 B/lane. A block covers 256 chunks of ONE image
// (bpi blocks per image), so the image index is a scalar and a lane pays one 32-bit division by C / 8; the coefficients (64 B per
// lane) come from a table of N * Cn * 8 bytes that stays in cache.
template <int DT>
__global__ __launch_bounds__(256) void instnorm_apply_kernel(const void* __restrict__ x, const float* __restrict__ ws,
                                                            void* __restrict__ y, unsigned nblocks, unsigned bpi, int HW, int C,
                                                            int Cn, int xpitch, int act_code, uint32_t* __restrict__ ovf) {
    const unsigned C8 = (unsigned)C / 8;
    const unsigned per_img = (unsigned)HW * C8;          // < 2^27: x lies inside the 2 GiB window
    const ActClamp act = make_act(act_code);
    F16Guard<DT> guard;
    for (unsigned bid = blockIdx.x; bid < nblocks; bid += gridDim.x) {
        const unsigned n = bid / bpi;
        const unsigned j = (bid - n * bpi) * 256 + threadIdx.x;
        if (j >= per_img) continue;
        const unsigned p = j / C8;
        const int c0 = (int)(j - p * C8) * 8;
        float v[8];
        load8<DT>(x, ((size_t)n * HW + p) * xpitch + c0, v);
        if (c0 < Cn) {
            const float* q = ws + ((size_t)n * Cn + c0) * 2;
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const f32x4 ab = *reinterpret_cast<const f32x4*>(q + 2 * e);
                v[e] = v[e] * ab[0] + ab[1];
                v[e + 1] = v[e + 1] * ab[2] + ab[3];
            }
        }
        apply_act8(v, act);
        guard.see(v);
        store8<DT>(y, ((size_t)n * per_img + j) * 8, v);
    }
    guard.commit(ovf);
}
