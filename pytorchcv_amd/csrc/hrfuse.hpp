// hrfuse.hpp - HRNet's multi-resolution exchange for ONE output branch as ONE launch.
//
// Replaces: the sum at the end of HRBlock.forward (reference pytorchcv/models/hrnet.py:126-134) - `y = y + self.fuse_layers[i][j](x[j])`
//           over the branches j, then `self.activ(y)` - including the `nn.Upsample(scale_factor=2 ** (j - i), mode="nearest")` of every
//           UpSamplingBlock on the way (hrnet.py:40-47): the upsampled tensors never exist.
//
//   y[n, h, w, c] = act( sum_{t = 0 .. nsrc-1} src_t[n, h >> shift_t, w >> shift_t, c] )
//
//   y      dense NHWC [N, H, W, C], C the physical pitch (a multiple of 8; pad channels of the sources are zero, so they come out zero)
//   src_t  dense NHWC [N, H >> shift_t, W >> shift_t, C]; H and W are exact multiples of 1 << shift_t
//
// The sum is fp32 in the order t = 0, 1, ... (the reference's j = 0 .. B-1), rounded ONCE to the storage type; fp16 results pass the
// range guard. The source pointers and shifts travel in the kernel argument struct: no pointer array on the device.
//
// HBM-bound, no reuse to organise: one thread owns one 8-channel chunk (16 bytes in 16 bit) of ONE output pixel. Lanes run over channel
// chunks first, then pixels, so a wave's fine loads and its stores are contiguous NHWC spans; the 2^shift x 2^shift output pixels that
// share a coarse pixel sit in neighbouring lanes and rows of the same few blocks, so all but the first of their loads are cache hits and
// HBM sees each coarse tensor once. A variant that gave a thread two horizontally adjacent pixels and loaded the coarse chunk once for
// both was measured and dropped: 7 - 29 % SLOWER at every shape with a coarse source (half as many threads in flight, and a lane's two
// stores a pixel apart), see profiles/experiments/hrfuse_kernel.md. NSRC is a template argument so that all loads of a pixel are
// issued before the first add. Fresh blocks, grid-stride only under the test cap (as se_scale_kernel).
#pragma once
#include "pcv_common.hpp"

constexpr int kHrMaxSrc = 4, kHrMaxShift = 3;

struct HrFuseParams {
    const void* src[kHrMaxSrc];
    int shift[kHrMaxSrc];
    void* y;
    int H, W, C8;         // output rows, columns, 8-channel chunks per pixel
    FastDiv dC8, dW, dH;
    uint32_t total;       // N * H * W * C8 work items
    int act;              // PCV_ACT_NONE / PCV_ACT_RELU
    uint32_t* ovf;        // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
};

template <int DT, int NSRC>
__global__ __launch_bounds__(256) void hr_fuse_kernel(const HrFuseParams p) {
    const ActClamp act = make_act(p.act);
    const int C = p.C8 * 8;
    F16Guard<DT> guard;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < p.total; i += gridDim.x * 256u) {
        const uint32_t pix = fastdiv(i, p.dC8);                         // (n * H + h) * W + w
        const int c0 = (int)(i - pix * (uint32_t)p.C8) * 8;
        const uint32_t row = fastdiv(pix, p.dW);                        // n * H + h
        const int w = (int)(pix - row * (uint32_t)p.W);
        const uint32_t n = fastdiv(row, p.dH);
        const int h = (int)(row - n * (uint32_t)p.H);

        float v[NSRC][8];
#pragma unroll
        for (int t = 0; t < NSRC; ++t) {
            const int s = p.shift[t];
            const int Hs = p.H >> s, Ws = p.W >> s;
            load8<DT>(p.src[t], (((size_t)n * Hs + (h >> s)) * Ws + (w >> s)) * C + c0, v[t]);
        }
#pragma unroll
        for (int t = 1; t < NSRC; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[0][e] += v[t][e];
        clamp8(v[0], act);
        guard.see(v[0]);
        store8<DT>(p.y, (size_t)i * 8, v[0]);
    }
    guard.commit(p.ovf);
}

// the instance for `nsrc` sources (1 .. 4, checked by the caller)
template <int DT> static void launch_hr_fuse(int nsrc, unsigned grid, hipStream_t st, const HrFuseParams& p) {
    switch (nsrc) {
        case 1: hr_fuse_kernel<DT, 1><<<grid, 256, 0, st>>>(p); break;
        case 2: hr_fuse_kernel<DT, 2><<<grid, 256, 0, st>>>(p); break;
        case 3: hr_fuse_kernel<DT, 3><<<grid, 256, 0, st>>>(p); break;
        default: hr_fuse_kernel<DT, 4><<<grid, 256, 0, st>>>(p); break;
    }
}
