// resize_kernel.hpp - decoded uint8 frames of ANY size -> the network's input in one launch: PIL-exact antialiased bilinear resize
// of the shorter side (torchvision `Resize(size)` on a PIL image: what the reference's accuracy figures were produced with),
// centre crop, normalise, NHWC4, cast. The arithmetic, the blob and the band choice are resize_plan.hpp's; the kernel only does the
// integer part, so its uint8 values equal PIL's bit for bit, and the last stage is preprocess_u8_kernel's (preprocess_store_px).
//
// One block = one work item = (frame, band of output rows); frames differ in size, so items differ in cost: every item gets a
// fresh block and the dispatcher balances them (a grid-stride walk only under the test cap "max_blocks").
//   pass 1  the source rows the band's vertical taps touch, resampled horizontally for the W crop columns only, rounded to uint8
//           into LDS ([row][W * C] bytes, pitch rounded up to 4). One thread = one (row, column), all C channels; neighbouring lanes
//           read neighbouring, overlapping source bytes, so the wave's byte loads fall into a few cache lines.
//   pass 2  vertical taps out of LDS, clamp, then normalise + store. One thread = one output pixel (pad columns included).
// The uint8 intermediate never leaves the CU. All sums are int32: sum(kk) <= 2^22 + taps, times 255, is below 2^31.
#pragma once
#include "pcv_common.hpp"
#include "resize_plan.hpp"
#include "aux_kernels.hpp"

__device__ __forceinline__ int resize_clip8(int ss) {
    ss >>= pcv_resize::kPrecisionBits;
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// One work item with the channel count a compile-time constant (the byte loads of a pixel then need no predicate).
template <int OT, int C>
__device__ __forceinline__ void resize_item(const char* __restrict__ plan, const pcv_resize::ResizeFrame* __restrict__ f, int n_img,
                                            int item, int H, int W, unsigned char* __restrict__ stage, void* __restrict__ y,
                                            int wpitch, const float* __restrict__ mean, const float* __restrict__ inv_std,
                                            uint32_t* __restrict__ ovf) {
    using namespace pcv_resize;
    typedef const unsigned char __attribute__((address_space(1))) * GlobalBytes;        // the frame is global memory, not "generic"
    constexpr int kRound = 1 << (kPrecisionBits - 1);
    const int pitch = (W * C + 3) & ~3;
    const int band = f->band, hk = f->hk, vk = f->vk, Ws = f->Ws;
    const int y0 = (item - f->item0) * band;
    const int y1 = min(y0 + band, H);
    const int* ht = reinterpret_cast<const int*>(plan + f->htab);           // xmin[W], n[W], kk[W][hk]
    const int* vt = reinterpret_cast<const int*>(plan + f->vtab);           // xmin[H], n[H], kk[H][vk]
    const int r0 = vt[y0];
    const int rows = vt[y1 - 1] + vt[H + y1 - 1] - r0;                      // windows move monotonically: the last row ends last
    GlobalBytes src = (GlobalBytes)f->src;

    for (int i = threadIdx.x; i < rows * W; i += 256) {
        const int r = i / W, x = i - r * W;
        const int xmin = ht[x], n = ht[W + x];
        const int* kk = ht + 2 * W + (size_t)x * hk;
        GlobalBytes p = src + ((size_t)(r0 + r) * Ws + xmin) * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = kRound;
        for (int k = 0; k < n; ++k) {
            const int wgt = kk[k];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[(size_t)k * C + c] * wgt;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) stage[r * pitch + x * C + c] = (unsigned char)resize_clip8(acc[c]);
    }
    __syncthreads();

    for (int i = threadIdx.x; i < (y1 - y0) * wpitch; i += 256) {
        const int yy = i / wpitch, x = i - yy * wpitch;
        const int yo = y0 + yy;
        unsigned char b[4] = {0, 0, 0, 0};
        if (x < W) {
            const int n = vt[H + yo];
            const int* kk = vt + 2 * H + (size_t)yo * vk;
            const unsigned char* p = stage + (vt[yo] - r0) * pitch + x * C;
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = kRound;
            for (int k = 0; k < n; ++k) {
                const int wgt = kk[k];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += (int)p[k * pitch + c] * wgt;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) b[c] = (unsigned char)resize_clip8(acc[c]);
        }
        preprocess_store_px<OT>(b, x < W, C, mean, inv_std, y, (((size_t)n_img * H + yo) * wpitch + x) * 4, ovf);
    }
    __syncthreads();                                                        // the next item refills the staging
}

template <int OT>
__global__ __launch_bounds__(256) void resize_crop_u8_kernel(const char* __restrict__ plan, void* __restrict__ y, int wpitch,
                                                            const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                            uint32_t* __restrict__ ovf) {
    using namespace pcv_resize;
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const ResizeHeader* hd = reinterpret_cast<const ResizeHeader*>(plan);
    const ResizeFrame* frames = reinterpret_cast<const ResizeFrame*>(plan + sizeof(ResizeHeader));
    const int N = hd->N, C = hd->C, H = hd->H, W = hd->W, items = hd->items;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        // the frame of this item: the last one whose first item is <= item (block-uniform)
        int lo = 0, hi = N - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (frames[mid].item0 <= item) lo = mid; else hi = mid - 1;
        }
        const ResizeFrame* f = frames + lo;
        switch (C) {
            case 1: resize_item<OT, 1>(plan, f, lo, item, H, W, stage, y, wpitch, mean, inv_std, ovf); break;
            case 2: resize_item<OT, 2>(plan, f, lo, item, H, W, stage, y, wpitch, mean, inv_std, ovf); break;
            case 3: resize_item<OT, 3>(plan, f, lo, item, H, W, stage, y, wpitch, mean, inv_std, ovf); break;
            default: resize_item<OT, 4>(plan, f, lo, item, H, W, stage, y, wpitch, mean, inv_std, ovf); break;
        }
    }
}
