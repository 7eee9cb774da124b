// mb_device.hpp - what the three kernels of the fused inverted-residual unit share (mbconv.hpp: block tiles, mbw.hpp: wave-private
// tiles, mbr.hpp: register-resident tiles): the parameter block, the LDS swizzles, the compile-time activation, and the STEPS the
// three spell alike - tile decode, the diagonal fragments of stage S2, the output offset of the epilogue (its
// BN and skip add are bn8 / add_skip8, pcv_common.hpp). Every kernel header of the family includes this file and no sibling kernel.
// As in conv_device.hpp the steps are shared and the sequence stays in each kernel. A helper is here only if every kernel that uses
// it still compiles to the text it had with its own copy; profiles/experiments/mb_device_refactor.md lists the ones that did not
// (the staging loops, the BN vector loads, a descriptor struct, bn8 outside mbr.hpp, the four-pack2 loop) and the kernels that therefore keep a copy.
#pragma once
#include "pcv_common.hpp"

struct MbParams {
    const void* x;            // [N,H,W,Cin]
    const void* res;          // [N,Ho,Wo,Cout] or null
    void* y;                  // [N,Ho,Wo,Cout]
    const void* w_exp;        // packed rows [round32(Cmid)][Kpad1]        (unused when EXPAND == false)
    const void* w_dw;         // [9][Cmid]
    const void* w_dwsp;       // compressed diagonal fragments [chunk][half][filter row][lane] 16 B (pack_dw_sparse_kernel; mbr.hpp)
    const void* w_proj;       // packed rows [round32(Cout)][Kpad2]
    const float *scale_e, *shift_e, *scale_d, *shift_d, *scale_p, *shift_p;
    uint32_t x_bytes, y_bytes, wexp_bytes, wdw_bytes, wproj_bytes;
    int N, H, W, Cin, Cmid, Cout, Ho, Wo;
    int Kpad1, Kpad2;
    int ka;                   // MFMA K-steps of the expand GEMM = ceil(Cin / 32) (<= 3)
    int nChunks;              // ceil(Cmid / 32)
    int nRowT;                // 16-row tiles of the project GEMM = round32(Cout) / 16. Host only: no kernel reads it (mbw / mbr take it as
                              // a template argument, the block kernel is compiled for 2); kept so that the offsets behind it stay put
    int tilesH, tilesW, nTiles;
    int nbufX;                // x tile buffers (2: the next tile is prefetched)
    int act_e, act_d, act_p, post;
    uint32_t* ovf;            // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
    uint32_t* dbg;            // diagnostic builds only (-DMBR_CYCLES): in-kernel stamps
};

// ---- LDS rows of 64 bytes = four 16-byte slots: the slot XOR of a row ----------------------------------------------------------------
// block kernel: f = [0,2,3,1][(row >> 2) & 3]
__device__ __forceinline__ int mb_swz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
// mbw / mbr: slot s of row r at s ^ (2 * bit 2 of r) - conflict-free for 16 consecutive rows at any base row (mbw.hpp)
template <bool SWZ> __device__ __forceinline__ int mb_swz64(int row) { return SWZ ? (row >> 1) & 2 : 0; }

// The activation behind the expand and the depthwise stage as a compile-time constant: with the launch-time code every one of the
// 11 + 4 unrolled applications per chunk was a nest of scalar branches (580 basic blocks), and nothing could be scheduled across them.
template <int ACT, int N> __device__ __forceinline__ void mb_act(float (&v)[N], const ActClamp& dyn) {
    if constexpr (ACT == PCV_ACT_RELU) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = __builtin_elementwise_maximum(v[e], 0.f);
    } else if constexpr (ACT == PCV_ACT_RELU6) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = __builtin_elementwise_minimum(__builtin_elementwise_maximum(v[e], 0.f), 6.f);
    } else {
        apply_actn<N>(v, dyn);
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
// tile t of a map cut into tilesH x tilesW tiles per image -> image, tile row, tile column
__device__ __forceinline__ void mb_tile_pos(int t, int tilesW, int tilesH, int& n, int& th, int& tw) {
    tw = t % tilesW;
    const int t2 = t / tilesW;
    th = t2 % tilesH;
    n = t2 / tilesH;
}

// ---- S2 on the dense MFMA: block-diagonal weights (mbconv.hpp, mbw.hpp) ----------------------------------------------------------------
// A (weights, rows = channels): lane (row fr, k quarter fq) holds tap (fq >> 1) of a tap pair, channels 8 (fq & 1) .. + 7 of the
// 16-channel half: non-zero only on the diagonal, i.e. element fr & 7 when (fr >> 3) == (fq & 1). Dword i of the lane's mask
// (filled in the kernel: as a helper that fills the array the same loop changed 24 mbw and all block instantiations):
__device__ __forceinline__ uint32_t mb_diag_bit(int fr, int fq, int i) {
    return ((fr >> 3) == (fq & 1) && i == ((fr & 7) >> 1)) ? 0xFFFFFFFFu : 0u;
}
// the A fragment from this lane's one 16-bit weight at w (a_sh = 16 (fr & 1): its half of the dword) under the mask am
template <typename FRAG> __device__ __forceinline__ FRAG mb_diag_frag(const char* w, int a_sh, const uint32_t (&am)[4]) {
    const uint32_t w16 = *reinterpret_cast<const uint16_t*>(w);
    const uint32_t val = w16 << a_sh;
    u32x4 a4;
#pragma unroll
    for (int i = 0; i < 4; ++i) a4[i] = val & am[i];
    return __builtin_bit_cast(FRAG, a4);
}

// ---- epilogue: v = acc * scale + shift -> act_p -> add_skip8 -> post_act -> range check -> four pack2 -> store at this offset ------------
// byte offset of channels ch .. ch + 7 of output pixel (n, ho, wo); a guarded offset is written `ok ? mb_out_off(...) : kOutOfRange`
// where `ok` is tested
__device__ __forceinline__ uint32_t mb_out_off(const MbParams& p, int n, int ho, int wo, int ch) {
    return (uint32_t)(((((long)n * p.Ho + ho) * p.Wo + wo) * p.Cout + ch) * 2);
}
#endif  // __HIP_DEVICE_COMPILE__
