// bnu.hpp - a whole ResNet bottleneck unit of the 56 x 56 stage in ONE launch, 16-bit storage, gfx950 MFMA:
//     y = post_act(act3(BN3(W3 . t2)) + skip),  t2 = act2(BN2(W2 (3x3, pad 1) * t1)),  t1 = act1(BN1(W1 . x))
// with skip = x (256 -> 64 -> 64 -> 256: the second and third unit of the stage) or, IDC form, skip = BN_id(W_id . x)
// (64 -> 64 -> 64 -> 256 with `identity_conv`: the first unit).
//
// Replaces: ResBottleneck.forward (conv1 -> conv2 -> conv3, reference resnet.py:136-140) and the `x + identity` + ReLU of
//           ResUnit.forward (resnet.py:221-229; identity_conv: resnet.py:214-216, 225-226) for the units of stage 1.
//
// Why. Run as separate launches a unit writes t1 and t2 (103 MB each at batch 256) and reads them back, and the 1x1 pair kernel
// that chains two units re-reads what it wrote: 1.1 - 1.2 GB per unit against 822 MB (x in once, y out once; IDC: 514 MB). The
// kernels involved already stream at the HBM rate, so only keeping t1 / t2 on the CU removes the traffic. With 64 mid channels
// W1 (256 x 64), W2 (9 x 64 x 64) and W3 (64 x 256) are 137 KB: they live in the registers of the eight waves as MFMA A
// fragments (120 registers per lane) for the whole persistent block.
//
// Decomposition: a block owns an (image, band of rows [r0, r1)) item and streams it top to bottom, one row per step, TWO phases
// (two barriers) per step s:
//   phase 1   conv1 on x row s -> BN, act, round -> t1 ring slot s & 3 (64-channel rows with a zero column at each end: LDS
//             position u holds pixel u - 1; a row outside the image is written as zeros), and, independent of it,
//             conv3 on t2 row s - 2 -> BN, act, + skip (x row s - 2, still in its ring slot), post_act, round -> 16-byte NHWC stores;
//   phase 2   the LDS-DMA pieces of x row s + 2 go out (into the slot row s - 2 has just left), then
//             conv2 on t1 rows s - 2 .. s -> BN, act, round -> the t2 row buffer (t2 row s - 1).
// s runs from r0 - 1 to r1 + 1: conv1 is recomputed for the two halo rows of a band, so an output element is the same number
// whatever the band split, the grid and the batch. Every x element is fetched once per item (band halo rows twice), every y
// element written once; nothing else touches HBM but the weights. The three rounding points are where the separate launches
// store. Each GEMM runs its K steps in one fixed order on one accumulator per 16 x 16 output block: conv1 K = 0 .. Cin - 1;
// conv2 (filter row, filter column, channel), as d3c_conv.hpp; conv3 K = 0 .. 63.
//
// Work split (mi = wave & 3, jp = wave >> 2): conv1 / conv2: 16 output channels (packed rows 16 mi ..) x pixel blocks 2 jp,
// 2 jp + 1 (pixel 16 j + fr; block 3 holds pixels 48 .. 55 only: its other lanes compute on whatever lies past the row and store
// nothing); conv3: 32 output channels (32 wave ..) x all four pixel blocks, so a lane ends with 8 consecutive channels of a pixel.
// Registers: 120 of weights + a ring of eight B fragments + accumulators = 248 - 256 per lane, two waves per SIMD, no spill.
// LDS images: the x ring is 56 pixels x Cin per slot, 16-byte chunk c of pixel px at slot c ^ (px & 15) (Cin = 64: c ^ ((px >> 1) & 7)),
// written by the DMA with the swizzle on the SOURCE side; t1 / t2 rows are 128 bytes per position, chunk c at c ^ ((u >> 1) & 7).
#pragma once
#include "conv_device.hpp"

struct BnuParams {
    const void* x;            // NHWC [N, H, 56, Cin]
    void* y;                  // NHWC [N, H, 56, 256]
    const void* w1;           // packed rows [64][Cin]
    const void* w2;           // packed rows [64][9 x 64], K = (filter row, filter column, channel)
    const void* w3;           // packed rows [256][64]
    const void* wid;          // IDC: packed rows [256][64]
    const float *scale1, *shift1, *scale2, *shift2, *scale3, *shift3, *scale_id, *shift_id;
    uint32_t w1_bytes, w2_bytes, w3_bytes, wid_bytes, y_bytes;
    int N, H;
    int band, nBands, nItems; // rows per band, bands per image, N * nBands
    int act1, act2, act3, post3;
    uint32_t* ovf;            // the context's fp16 overflow counter (pcv_common.hpp, F16Guard)
};

template <bool IDC> struct BnuCfg {
    static constexpr int THREADS = 512, NW = 8;
    static constexpr int W = 56, CM = 64, CO = 256, CIN = IDC ? 64 : 256;
    static constexpr int XPIX = CIN * 2;                      // bytes per pixel of x
    static constexpr int CPP = CIN / 8;                       // 16-byte chunks per pixel
    static constexpr int XROW = W * XPIX;                     // one ring slot: 28 672 B (IDC: 7 168)
    static constexpr int XSLOTS = 4;                          // rows s - 2 (skip), s - 1, s (conv1), s + 1 / s + 2 (in flight)
    static constexpr int NPIECE = XROW / 1024;                // 1 KB DMA pieces per row: 28 (IDC: 7)
    static constexpr int PPW = (NPIECE + NW - 1) / NW;        // pieces per wave and row: 4 (IDC: 1); the ones past NPIECE go to the dump KB
    static constexpr int TROW = 64 * 128;                     // one t1 / t2 row: 64 positions x 64 channels
    static constexpr int TSLOTS = 4;
    static constexpr int OFF_T1 = XSLOTS * XROW;
    static constexpr int OFF_T2 = OFF_T1 + TSLOTS * TROW;
    static constexpr int OFF_DUMP = OFF_T2 + TROW;
    static constexpr int OFF_BN = OFF_DUMP + 1024;            // fp32 scale / shift: conv1, conv2 (64 each), conv3 (256), IDC: identity conv (256)
    static constexpr int NBN = 2 * CM + 2 * CM + 2 * CO + (IDC ? 2 * CO : 0);
    static constexpr int LDS = OFF_BN + NBN * 4;              // 159 744 B (IDC: 75 776)
};

template <int DT, bool IDC>
__global__ __launch_bounds__(512, 2) void bnu_kernel(const BnuParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef BnuCfg<IDC> G;
    typedef typename Mma<DT>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int mi = wave & 3, jp = wave >> 2;
    if ((int)blockIdx.x >= p.nItems) return;

    const __amdgpu_buffer_rsrc_t yrsrc = buffer_rsrc(p.y, p.y_bytes);
    const __amdgpu_buffer_rsrc_t w1r = buffer_rsrc(p.w1, p.w1_bytes), w2r = buffer_rsrc(p.w2, p.w2_bytes);
    const __amdgpu_buffer_rsrc_t w3r = buffer_rsrc(p.w3, p.w3_bytes);
    const __amdgpu_buffer_rsrc_t widr = buffer_rsrc(IDC ? p.wid : p.w3, IDC ? p.wid_bytes : p.w3_bytes);

    // ---- BN constants and the zero columns of the t1 ring (positions 0 and 57 of every slot; nothing else ever writes them) ----
    float* const s1 = reinterpret_cast<float*>(smem + G::OFF_BN);
    float* const h1 = s1 + G::CM;
    float* const s2 = h1 + G::CM;
    float* const h2 = s2 + G::CM;
    float* const s3 = h2 + G::CM;
    float* const h3 = s3 + G::CO;
    float* const sid = h3 + G::CO;
    float* const hid = sid + G::CO;
    if (tid < G::CM) {
        s1[tid] = p.scale1[tid]; h1[tid] = p.shift1[tid];
        s2[tid] = p.scale2[tid]; h2[tid] = p.shift2[tid];
        const int slot = tid >> 4, pos = ((tid >> 3) & 1) ? G::W + 1 : 0, chunk = tid & 7;
        *reinterpret_cast<u32x4*>(smem + G::OFF_T1 + slot * G::TROW + pos * 128 + chunk * 16) = (u32x4){0u, 0u, 0u, 0u};
    }
    if (tid < G::CO) {
        s3[tid] = p.scale3[tid]; h3[tid] = p.shift3[tid];
        if constexpr (IDC) { sid[tid] = p.scale_id[tid]; hid[tid] = p.shift_id[tid]; }
    }

    // ---- weights -> registers (once per block) ----
    constexpr int K1S = G::CIN / 32;                            // K steps of conv1: 8 (IDC: 2)
    frag a1[K1S], a2[18], a3[2][2], aid[2][2];
#pragma unroll
    for (int ks = 0; ks < K1S; ++ks)
        a1[ks] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(
            w1r, (uint32_t)(((16 * mi + fr) * G::CIN + ks * 32 + 8 * fq) * 2), 0, 0));
#pragma unroll
    for (int kh = 0; kh < 18; ++kh)                              // K-half kh: tap kh >> 1, channels 32 (kh & 1) ..
        a2[kh] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(
            w2r, (uint32_t)(((16 * mi + fr) * (9 * G::CM) + (kh >> 1) * G::CM + (fq + 4 * (kh & 1)) * 8) * 2), 0, 0));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const uint32_t off = (uint32_t)(((32 * wave + 16 * i + fr) * G::CM + ks * 32 + 8 * fq) * 2);
            a3[i][ks] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(w3r, off, 0, 0));
            if constexpr (IDC) aid[i][ks] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(widr, off, 0, 0));
        }

    // ---- per-lane address pieces ----
    // Pixel block j holds pixels 16 j + fr: every swizzle key below depends on fr alone, so block j is block 0 + j x (16 pixels) and one
    // register serves all blocks. Block 3 has pixels 48 .. 55 only: its lanes fr >= 8 read whatever lies 8 pixels past the row (inside the
    // LDS allocation: the next slot or region), compute garbage in their own MFMA columns and store nothing (`live`).
    auto xkey = [](int px) { return IDC ? ((px >> 1) & 7) : (px & 15); };
    auto tkey = [](int u) { return (u >> 1) & 7; };
    constexpr uint32_t XBLK = 16 * G::XPIX, TBLK = 16 * 128;    // bytes per pixel block in the x ring / in a t1, t2 row
    // conv1 / conv2: pixel blocks 2 jp + jj; channels 32 (mi >> 1) + 8 fq + 4 (mi & 1) .. + 3 = half `mi & 1` of chunk 4 (mi >> 1) + fq
    const int cc = 4 * (mi >> 1) + fq, c0 = 8 * cc + 4 * (mi & 1);
    const int pxa = 32 * jp + fr;                               // this lane's pixel in block 2 jp
    const bool live12[2] = {true, pxa + 16 < G::W};
    const uint32_t xa = (uint32_t)(pxa * G::XPIX + ((fq ^ xkey(pxa)) << 4));                                   // + jj XBLK; K step ks: ^ (ks << 6)
    uint32_t ta[3];                                              // filter column q: position pxa + q; + jj TBLK; K-half h: ^ (h << 6)
#pragma unroll
    for (int q = 0; q < 3; ++q) ta[q] = (uint32_t)((pxa + q) * 128 + ((fq ^ tkey(pxa + q)) << 4));
    const uint32_t tw = (uint32_t)((pxa + 1) * 128 + ((cc ^ tkey(pxa + 1)) << 4) + 8 * (mi & 1));          // + jj TBLK
    const uint32_t t2w = (uint32_t)(pxa * 128 + ((cc ^ tkey(pxa)) << 4) + 8 * (mi & 1));                   // + jj TBLK
    // conv3: pixel blocks 0 .. 3 (pixel 16 j + fr), channels 32 wave + 8 fq .. + 7
    const int ch3 = 32 * wave + 8 * fq;
    const uint32_t t2r = (uint32_t)(fr * 128 + ((fq ^ tkey(fr)) << 4));                                     // + j TBLK; K step ks: ^ (ks << 6)
    // the skip: plain form, the lane's 16 bytes of x; IDC, the B fragment of x (K step ks: ^ (ks << 6)); + j XBLK
    const uint32_t xs = IDC ? (uint32_t)(fr * G::XPIX + ((fq ^ xkey(fr)) << 4)) : (uint32_t)(fr * G::XPIX + (((4 * wave + fq) ^ xkey(fr)) << 4));
    // x DMA: piece pc = wave + 8 i is the KB of ring chunks 64 pc .. 64 pc + 63; this lane's chunk P holds chunk (P % CPP) ^ key of pixel
    // P / CPP. A piece is 1024 / XPIX pixels, 8 pieces a multiple of 16 pixels: the key is the same for every i, the source is + 8 i KB.
    const uint32_t dsrc = (uint32_t)(((wave * 64 + lane) / G::CPP) * G::XPIX + (((wave * 64 + lane) % G::CPP) ^ xkey((wave * 64 + lane) / G::CPP)) * 16);
    static_assert((8 * 1024 / G::XPIX) % 16 == 0, "the swizzle key repeats every 8 pieces");

    const EpiBounds B1 = make_epi_bounds(p.act1, PCV_ACT_NONE), B2 = make_epi_bounds(p.act2, PCV_ACT_NONE);
    const EpiBounds B3 = make_epi_bounds(p.act3, p.post3);
    const uint32_t imgBytes = (uint32_t)(p.H * G::XROW);
    __amdgpu_buffer_rsrc_t xr = buffer_rsrc(p.x, 0u);           // the item's image (set per item)
    int r1 = 0;                                                  // the item's last row + 1

    // row `row` of the item's image into ring slot row & 3; a row the item does not read (outside the image, past the band's halo) or a
    // piece that does not exist fetches nothing (out-of-range source) and lands in the dump KB, so that every wave issues PPW pieces per call
    auto issue_row = [&](int row) __attribute__((always_inline)) {
        const bool rowok = row >= 0 && row < p.H && row <= r1;
#pragma unroll
        for (int i = 0; i < G::PPW; ++i) {
            const int pc = wave + G::NW * i;
            const bool ok = rowok && pc < G::NPIECE;
            const uint32_t voff = ok ? (uint32_t)(row * G::XROW + i * G::NW * 1024) + dsrc : kOutOfRange;
            char* const dst = ok ? smem + (row & 3) * G::XROW + pc * 1024 : smem + G::OFF_DUMP;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, PCV_LDS(dst), 16, voff, 0, 0, 0);
        }
    };

    // B fragments come from LDS through a ring of RING values, each requested RD MFMAs ahead of its use (straight-line code, every index
    // a compile-time constant): left to the scheduler a fragment was requested one MFMA ahead, and every MFMA waited out the LDS latency.
    constexpr int RD = 6, RING = 8;
    // The ResNet forms of the three epilogues - ReLU behind conv1 / conv2; no activation, skip add, ReLU behind conv3 - as compile-time
    // variants (one v_maximum3 per value instead of clamps to both bounds: conv_device.hpp, epi2's RO form). Same values either way.
    const bool ro1 = p.act1 == PCV_ACT_RELU, ro2 = p.act2 == PCV_ACT_RELU, ro3 = p.act3 == PCV_ACT_NONE && p.post3 == PCV_ACT_RELU;

    // two accumulators (this wave's 16 channels x its two pixel blocks) -> BN, activation, round -> 8 bytes per live lane at dst + off[jj]
    auto epi12 = [&](auto ROc, const f32x4 (&acc)[2], const float* sp, const float* hp, const EpiBounds& B, char* dst,
                     uint32_t off) __attribute__((always_inline)) {
        constexpr bool RO = decltype(ROc)::value;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(sp + c0), sh = *reinterpret_cast<const f32x4*>(hp + c0);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            F16Guard<DT> guard;                                  // per pixel block: a dead lane's garbage must not count as an overflow
            u32x2 o;
            o[0] = epi2<DT, false, RO>(acc[jj][0] * sc[0] + sh[0], acc[jj][1] * sc[1] + sh[1], 0u, B, guard);
            o[1] = epi2<DT, false, RO>(acc[jj][2] * sc[2] + sh[2], acc[jj][3] * sc[3] + sh[3], 0u, B, guard);
            if (live12[jj]) *reinterpret_cast<u32x2*>(dst + off + jj * TBLK) = o;
            guard.commit(p.ovf, live12[jj]);
        }
    };

    // ---- conv1 on x row s -> t1 ring slot s & 3 ----
    auto conv1 = [&](int s) __attribute__((always_inline)) {
        char* const t1w = smem + G::OFF_T1 + (s & 3) * G::TROW;
        if (s < 0 || s >= p.H) {                                 // the zero padding above / below the image
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
                if (live12[jj]) *reinterpret_cast<u32x2*>(t1w + tw + jj * TBLK) = (u32x2){0u, 0u};
            return;
        }
        const char* const xb = smem + (s & 3) * G::XROW;
        constexpr int NST = 2 * K1S, RD1 = RD < NST ? RD : NST;   // step st: K step st >> 1, pixel block st & 1
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
        frag bq[RING];
        auto rd = [&](auto STc) __attribute__((always_inline)) {
            constexpr int st = decltype(STc)::value;
            bq[st % RING] = *reinterpret_cast<const frag*>(xb + (xa ^ (uint32_t)((st >> 1) << 6)) + (st & 1) * XBLK);
        };
        static_for<RD1>(rd);
        static_for<NST>([&](auto STc) __attribute__((always_inline)) {
            constexpr int st = decltype(STc)::value;
            if constexpr (st + RD1 < NST) rd(std::integral_constant<int, st + RD1>{});
            acc[st & 1] = Mma<DT>::run(a1[st >> 1], bq[st % RING], acc[st & 1]);
            __builtin_amdgcn_sched_barrier(0);                   // (the scheduler otherwise sinks every read down to its MFMA again)
        });
        if (ro1) epi12(std::true_type{}, acc, s1, h1, B1, t1w, tw);
        else epi12(std::false_type{}, acc, s1, h1, B1, t1w, tw);
    };

    // ---- conv2 on t1 rows s - 2 .. s -> the t2 row buffer (row s - 1) ----
    auto conv2 = [&](int s) __attribute__((always_inline)) {
        const char* const tb0 = smem + G::OFF_T1 + ((s - 2) & 3) * G::TROW;
        const char* const tb1 = smem + G::OFF_T1 + ((s - 1) & 3) * G::TROW;
        const char* const tb2 = smem + G::OFF_T1 + (s & 3) * G::TROW;
        constexpr int NST = 36;                                   // step st: K-half st >> 1 (tap (r, q), channel half h), pixel block st & 1
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
        frag bq[RING];
        auto rd = [&](auto STc) __attribute__((always_inline)) {
            constexpr int st = decltype(STc)::value;
            constexpr int kh = st >> 1, r = (kh >> 1) / 3, q = (kh >> 1) - 3 * r, h = kh & 1;
            const char* const tb = r == 0 ? tb0 : (r == 1 ? tb1 : tb2);
            bq[st % RING] = *reinterpret_cast<const frag*>(tb + (ta[q] ^ (uint32_t)(h << 6)) + (st & 1) * TBLK);
        };
        static_for<RD>(rd);
        static_for<NST>([&](auto STc) __attribute__((always_inline)) {
            constexpr int st = decltype(STc)::value;
            if constexpr (st + RD < NST) rd(std::integral_constant<int, st + RD>{});
            acc[st & 1] = Mma<DT>::run(a2[st >> 1], bq[st % RING], acc[st & 1]);
            __builtin_amdgcn_sched_barrier(0);
        });
        if (ro2) epi12(std::true_type{}, acc, s2, h2, B2, smem + G::OFF_T2, t2w);
        else epi12(std::false_type{}, acc, s2, h2, B2, smem + G::OFF_T2, t2w);
    };

    // ---- conv3 on the t2 row buffer (row `row`) + skip from x ring slot row & 3 -> y; two pixel blocks at a time ----
    auto conv3_half = [&](auto ROc, auto JHc, const char* xb, int mRow) __attribute__((always_inline)) {
        constexpr bool RO = decltype(ROc)::value;
        constexpr int j0 = 2 * decltype(JHc)::value;
        const char* const tb = smem + G::OFF_T2;
        frag b[2][2];                                             // [K step][pixel block]
        u32x4 skip[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) b[ks][jj] = *reinterpret_cast<const frag*>(tb + (t2r ^ (uint32_t)(ks << 6)) + (j0 + jj) * TBLK);
        if constexpr (!IDC) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) skip[jj] = *reinterpret_cast<const u32x4*>(xb + xs + (j0 + jj) * XBLK);
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    acc[i][jj] = Mma<DT>::run(a3[i][ks], b[ks][jj], ks == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[i][jj]);
        F16Guard<DT> guard[2];                                    // per pixel block: a dead lane's garbage must not count as an overflow
        if constexpr (IDC) {
            // skip = round(BN_id(W_id . x0)): rounded where the identity convolution's own launch would have stored it
            const f32x4 si0 = *reinterpret_cast<const f32x4*>(sid + ch3), si1 = *reinterpret_cast<const f32x4*>(sid + ch3 + 4);
            const f32x4 hi0 = *reinterpret_cast<const f32x4*>(hid + ch3), hi1 = *reinterpret_cast<const f32x4*>(hid + ch3 + 4);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                frag bx[2];                                       // the B fragments of x for the identity convolution
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) bx[ks] = *reinterpret_cast<const frag*>(xb + (xs ^ (uint32_t)(ks << 6)) + (j0 + jj) * XBLK);
                f32x4 ad[2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        ad[i] = Mma<DT>::run(aid[i][ks], bx[ks], ks == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : ad[i]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float v0 = ad[0][2 * e] * si0[2 * e] + hi0[2 * e], v1 = ad[0][2 * e + 1] * si0[2 * e + 1] + hi0[2 * e + 1];
                    const float v2 = ad[1][2 * e] * si1[2 * e] + hi1[2 * e], v3 = ad[1][2 * e + 1] * si1[2 * e + 1] + hi1[2 * e + 1];
                    guard[jj].see2(v0, v1);
                    guard[jj].see2(v2, v3);
                    skip[jj][e] = pack2<DT>(v0, v1);
                    skip[jj][2 + e] = pack2<DT>(v2, v3);
                }
            }
        }
        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(s3 + ch3), sc1 = *reinterpret_cast<const f32x4*>(s3 + ch3 + 4);
        const f32x4 sh0 = *reinterpret_cast<const f32x4*>(h3 + ch3), sh1 = *reinterpret_cast<const f32x4*>(h3 + ch3 + 4);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const f32x4 &c0v = acc[0][jj], &c1v = acc[1][jj];
            u32x4 o;
            o[0] = epi2<DT, true, RO>(c0v[0] * sc0[0] + sh0[0], c0v[1] * sc0[1] + sh0[1], skip[jj][0], B3, guard[jj]);
            o[1] = epi2<DT, true, RO>(c0v[2] * sc0[2] + sh0[2], c0v[3] * sc0[3] + sh0[3], skip[jj][1], B3, guard[jj]);
            o[2] = epi2<DT, true, RO>(c1v[0] * sc1[0] + sh1[0], c1v[1] * sc1[1] + sh1[1], skip[jj][2], B3, guard[jj]);
            o[3] = epi2<DT, true, RO>(c1v[2] * sc1[2] + sh1[2], c1v[3] * sc1[3] + sh1[3], skip[jj][3], B3, guard[jj]);
            const int px = 16 * (j0 + jj) + fr;
            const uint32_t off = px < G::W ? nhwc_off(mRow + px, G::CO, ch3) : kOutOfRange;     // (the host keeps y below 2 GiB)
            __builtin_amdgcn_raw_buffer_store_b128(o, yrsrc, off, 0, 0);
            guard[jj].commit(p.ovf, px < G::W);
        }
    };
    auto conv3 = [&](int row, int mRow) __attribute__((always_inline)) {      // mRow: flat pixel index of the row's first pixel
        const char* const xb = smem + (row & 3) * G::XROW;
        if (ro3) {
            conv3_half(std::true_type{}, std::integral_constant<int, 0>{}, xb, mRow);
            conv3_half(std::true_type{}, std::integral_constant<int, 1>{}, xb, mRow);
        } else {
            conv3_half(std::false_type{}, std::integral_constant<int, 0>{}, xb, mRow);
            conv3_half(std::false_type{}, std::integral_constant<int, 1>{}, xb, mRow);
        }
    };

    // A bare s_barrier orders nothing: a wave's LDS stores (t1, t2, the constants) must have retired before it arrives (lgkmcnt(0));
    // N: how many of its youngest vector-memory operations - the DMA pieces just issued - may still be in flight
    auto sync = [&](auto Nc) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(decltype(Nc)::value) : "memory");
        d3q_sync();
    };

    // ---- the persistent loop over (image, band) items ----
    for (int it = blockIdx.x; it < p.nItems; it += gridDim.x) {
        const int n = it / p.nBands, r0 = (it - n * p.nBands) * p.band;
        r1 = r0 + p.band < p.H ? r0 + p.band : p.H;
        xr = buffer_rsrc(reinterpret_cast<const char*>(p.x) + (size_t)n * imgBytes, imgBytes);
        // (every wave passed the barrier behind the previous item's last step: the ring is free; the first time it orders the
        // zero columns and BN constants above before their readers)
        issue_row(r0 - 1);
        issue_row(r0);
        sync(std::integral_constant<int, 0>{});
        for (int s = r0 - 1; s <= r1 + 1; ++s) {
            // phase 1: reads x rows s and s - 2 and the t2 row buffer, writes t1 slot s & 3
            if (s <= r1) conv1(s);
            if (s >= r0 + 2) conv3(s - 2, (n * p.H + s - 2) * G::W);
            sync(std::integral_constant<int, 63>{});             // (63: no wait on vector memory - the y stores stay in flight)
            // phase 2: reads t1 rows s - 2 .. s, writes the t2 row buffer; x row s + 2 replaces row s - 2
            issue_row(s + 2);
            if (s >= r0 + 1 && s <= r1) conv2(s);
            // x row s + 1 (issued one step ago, or in the prologue) has landed: everything but the PPW pieces just issued is done
            sync(std::integral_constant<int, G::PPW>{});
        }
    }
#endif  // __HIP_DEVICE_COMPILE__
}
