// conv_device.hpp - what the dense convolution kernels that take `D3Params` share (d3q / d3w / d3c / d3k / d3i / d1i / p1r): the
// parameter block, a block's tile list, the barrier, and the EPILOGUE - v = acc * scale + shift -> act -> (+ skip tensor) -> post_act ->
// fp16 range check -> packed pair - written once. Every kernel header of the family includes this file and no sibling kernel.
#pragma once
#include "pcv_common.hpp"

struct D3Params {
    const void* x;          // NHWC [N,H,W,Cin], dense
    const void* w;          // packed weights [rows][Kpad], K = (r, slice, q), rows in MFMA order
    const void* res;        // residual NHWC [M, Cout] or null
    void* y;                // NHWC [M, Ypitch]
    const float* scale;     // [Cout] fp32, never null
    const float* shift;
    uint32_t x_bytes, w_bytes, y_bytes, res_bytes;
    int M;                  // N*H*W
    int Cout, Ypitch;
    int H, W, Cin, HW;
    FastDiv div_hw, div_w;
    int nk;                 // K-steps = 9 * Cin / 64 (a multiple of 3)
    int slices;             // Cin / 64
    int Kpad;
    int act, post_act;
    int nChTiles, nTiles;
    uint32_t* dbg;          // diagnostic builds only (-DD3X3_STAMPS)
    int stride, Hin, Win;   // 1x1 mode only: output pixel (n, ho, wo) reads input pixel (n, stride ho, stride wo) of an Hin x Win map
                            // (H, W, HW, div_hw, div_w then describe the OUTPUT map)
    uint32_t* ovf;          // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
    int tailN;              // p1r_conv.hpp only: tiles nTiles .. nTiles + tailN - 1 are split into 16-pixel units over the blocks (0: none)
    int dbgflags;           // timing experiments only (pcv_set_tuning("dbg", bits); results are WRONG with any bit set): 1 = output stores
                            // dropped (out-of-range offsets), 2 = no epilogue at all, 4 = loaders keep the first tile's row table, 8 = compute waves keep the
                            // first tile's column masks, 16 = row table built at the tile change (A/B of the look-ahead build; results stay right)
};

#if defined(__HIP_DEVICE_COMPILE__)
// The tile list of a block: [tile0, tend) of its XCD's contiguous range, stride = blocks per XCD (every wave computes the same).
struct D3Tiles {
    int tile0, tend, tstride, nMine;
};
__device__ __forceinline__ D3Tiles d3q_tiles(const D3Params& p) {
    D3Tiles t;
    const int perXcd = (p.nTiles + 7) >> 3;
    const int xcd = blockIdx.x & 7;
    t.tstride = gridDim.x >> 3;                               // host guarantees gridDim.x % 8 == 0
    t.tile0 = xcd * perXcd + (int)(blockIdx.x >> 3);
    t.tend = min(p.nTiles, (xcd + 1) * perXcd);
    t.nMine = t.tile0 < t.tend ? (t.tend - t.tile0 + t.tstride - 1) / t.tstride : 0;
    return t;
}
__device__ __forceinline__ void d3q_sync() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// ---- the epilogue's activations ---------------------------------------------------------------------------------------------------
// Activations none / ReLU / ReLU6 as BRANCH-FREE clamps to launch-uniform bounds (-inf / 0, +inf / 6; IEEE-754-2019 maximum /
// minimum: a NaN stays a NaN, max(v, -inf) = v and min(v, +inf) = v bit for bit): the uniform switch of `clampn` is a dozen scalar
// branches per pixel block, and a wave that is alone on its SIMD pays every one of them (d3c: 3 100 cycles per tile's epilogue).
// [alo, ahi]: the activation in front of the skip add; [plo, phi]: the one behind it; [clo, chi]: both at once - with nothing between
// the two activations clamp(clamp(v, alo, ahi), plo, phi) = clamp(v, max(alo, plo), min(ahi, phi)) for these bounds (0 / -inf below,
// 6 / +inf above), NaN and signed zero included.
struct EpiBounds {
    float alo, ahi, plo, phi, clo, chi;
};
__device__ __forceinline__ EpiBounds make_epi_bounds(int act, int post_act) {
    EpiBounds b;
    b.alo = (act == PCV_ACT_RELU || act == PCV_ACT_RELU6) ? 0.f : -INFINITY;
    b.ahi = act == PCV_ACT_RELU6 ? 6.f : INFINITY;
    b.plo = (post_act == PCV_ACT_RELU || post_act == PCV_ACT_RELU6) ? 0.f : -INFINITY;
    b.phi = post_act == PCV_ACT_RELU6 ? 6.f : INFINITY;
    b.clo = b.alo > b.plo ? b.alo : b.plo;
    b.chi = b.ahi < b.phi ? b.ahi : b.phi;
    return b;
}
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) {
    return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, lo), hi);
}
// The ResNet forms of a launch - ReLU only (no skip tensor), or no activation + skip tensor + ReLU - need ONE v_maximum3 per value
// where the general form clamps to both bounds (two instructions per clamp, infinite bounds included). Same values either way. d3i and
// d1i tell the two apart (`relu_only`, computed in the kernel) and run f(HR, RO) with the launch's form as compile-time constants:
// HR = a skip tensor, RO = the ReLU-only form.
template <typename F> __device__ __forceinline__ void epi_dispatch(bool has_res, bool relu_only, F&& f) {
    if (has_res) { if (relu_only) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
    else { if (relu_only) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

// ---- two values -------------------------------------------------------------------------------------------------------------------
// Two BN results (v = acc * scale + shift) of neighbouring channels -> act -> (+ the two 16-bit skip values of `skip`) -> post_act ->
// range check -> the packed pair. HR: the launch has a skip tensor; RO: the ReLU-only form (above).
template <int DT, bool HR, bool RO>
__device__ __forceinline__ uint32_t epi2(float v0, float v1, uint32_t skip, const EpiBounds& b, F16Guard<DT>& guard) {
    if constexpr (RO) {
        if constexpr (HR) {
            float lo, hi;
            unpack2<DT>(skip, lo, hi);
            v0 += lo;
            v1 += hi;
        }
        v0 = __builtin_elementwise_maximum(v0, 0.f);
        v1 = __builtin_elementwise_maximum(v1, 0.f);
    } else if constexpr (HR) {
        v0 = clamp_nan(v0, b.alo, b.ahi);
        v1 = clamp_nan(v1, b.alo, b.ahi);
        float lo, hi;
        unpack2<DT>(skip, lo, hi);
        v0 += lo;
        v1 += hi;
        v0 = clamp_nan(v0, b.plo, b.phi);
        v1 = clamp_nan(v1, b.plo, b.phi);
    } else {
        v0 = clamp_nan(v0, b.clo, b.chi);
        v1 = clamp_nan(v1, b.clo, b.chi);
    }
    guard.see2(v0, v1);
    return pack2<DT>(v0, v1);
}

// ---- eight values: the 8 consecutive channels of one pixel that a lane owns (accumulators c0: + 0..3, c1: + 4..7) ------------------------
// d3q / d3w (`clampn`'s uniform switch is affordable with three / two waves per SIMD):
//     bn8 -> clampn(act) -> add_skip8 -> clampn(post_act) -> guard.see -> four pack2 -> the 16-byte NHWC store.
// The steps are helpers, the sequence stays in the kernel: a helper with a branch inside (clampn, a guarded offset, a ternary on a
// run-time condition) compiles to different code once it is nested in another function, a straight-line one does not
// (profiles/experiments/kernel_helpers_refactor.md). bn8 / add_skip8: pcv_common.hpp (the fused-unit kernels use them too).
// BN scale / shift of channels chl .. chl + 7 (chl: a multiple of 4 inside [0, Cout - 8])
__device__ __forceinline__ void load_bn8(const D3Params& p, int chl, f32x4& s0, f32x4& s1, f32x4& h0, f32x4& h1) {
    s0 = *reinterpret_cast<const f32x4*>(p.scale + chl); s1 = *reinterpret_cast<const f32x4*>(p.scale + chl + 4);
    h0 = *reinterpret_cast<const f32x4*>(p.shift + chl); h1 = *reinterpret_cast<const f32x4*>(p.shift + chl + 4);
}

// d3c / d3k: tile t of 4-row tiles of one image -> channel tile, image, first output row
template <int ROWS> __device__ __forceinline__ void d3r_tile_pos(const D3Params& p, int tilesPerImage, int t, int& chTile, int& n, int& y0) {
    chTile = t % p.nChTiles;
    const int pt = t / p.nChTiles;
    n = pt / tilesPerImage;
    y0 = (pt - n * tilesPerImage) * ROWS;
}
#endif  // __HIP_DEVICE_COMPILE__
