// pcv_common.hpp - shared device helpers for the gfx950 kernels (element types, activations, fast division).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "../../include/pcv_amd.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define PCV_LDS(p) ((__attribute__((address_space(3))) void*)(p))

// ---- small device helpers ------------------------------------------------------------------------------
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order: a loop whose index is a compile-time constant in
// every iteration (register-array indices, `if constexpr` per step)
template <typename F, int... I> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}
// at most N of this wave's vector-memory operations (LDS-DMA pieces included) are still in flight; opaque to the compiler's own
// wait-count pass (where that pass must see the wait, a kernel uses __builtin_amdgcn_s_waitcnt)
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// A byte offset no buffer descriptor here covers (the host keeps every tensor below 2 GiB): a load at it returns zeros, a store is
// dropped - the range check stands in for a branch.
constexpr uint32_t kOutOfRange = 0x80000000u;
// byte offset of channel ch0 of row m in a 16-bit NHWC tensor of `pitch` channels per pixel. The arithmetic runs in m's type: int
// where the host bounds the tensor by 2 GiB, size_t where the kernel does not rely on that. A guarded offset is written
// `ok ? nhwc_off(m, pitch, ch0) : kOutOfRange` where `ok` is tested (as a bool argument the condition compiles differently).
template <typename I> __device__ __forceinline__ uint32_t nhwc_off(I m, int pitch, int ch0) {
    return (uint32_t)((m * pitch + ch0) * 2);
}
#if defined(__HIP_DEVICE_COMPILE__)      // (buffer-resource types are device-only)
// raw buffer descriptor over `bytes` bytes at p (num_records = bytes: every access is range-checked against it)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
#endif

// ---- one MFMA K-half (16 x 16 output block, 32 elements of K; fp32 storage: 16) per storage type -------------
template <int DT> struct Mma;
template <> struct Mma<PCV_BF16> {
    typedef s16x8 frag;
    static __device__ __forceinline__ f32x4 run(const frag& a, const frag& b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<PCV_F16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x4 run(const frag& a, const frag& b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<PCV_F32> {
    // exact-f32 MFMA (v_mfma_f32_16x16x4_f32): the 16-byte chunk held by lane group q carries k = 4q+e, and
    // MFMA e (0..3) sums element e over the four lane groups - the same k association on both operands.
    typedef f32x4 frag;
    static __device__ __forceinline__ f32x4 run(const frag& a, const frag& b, f32x4 c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
        return c;
    }
};

// ---- element traits: storage type tag -> bytes, conversions -------------------------------------------
template <int DT> struct Elem;
template <> struct Elem<PCV_F32> { static constexpr int BYTES = 4; };
template <> struct Elem<PCV_BF16> { static constexpr int BYTES = 2; };
template <> struct Elem<PCV_F16> { static constexpr int BYTES = 2; };

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t b16) { return __uint_as_float(b16 << 16); }

// fp32 -> bf16 (round-to-nearest-even; a plain cast lowers to v_cvt_pk_bf16_f32 and keeps NaN a NaN)
__device__ __forceinline__ uint32_t pack2_bf16(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
    typedef __attribute__((ext_vector_type(2))) float f2;
    f2 v = {lo, hi};
    bf2 r = __builtin_convertvector(v, bf2);
    return *reinterpret_cast<uint32_t*>(&r);
}
__device__ __forceinline__ uint32_t pack2_f16(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    typedef __attribute__((ext_vector_type(2))) float f2;
    f2 v = {lo, hi};
    h2 r = __builtin_convertvector(v, h2);
    return *reinterpret_cast<uint32_t*>(&r);
}
// fp16 only: round the pair FIRST, then clamp the packed pair to [0, upper] (upper = two fp16 values, e.g. 0x46004600 = 6.0) with
// v_pk_maximum3_f16 / v_pk_minimum3_f16 - two instructions for two values where the fp32 clamp takes four. Same bits as clamping
// in fp32 and rounding afterwards: rounding is monotonic and 0 / 6 are fp16 values (a value beyond fp16's range rounds to +-inf and
// is clamped to upper / 0 like its fp32 original); both forms propagate NaN (IEEE-754-2019 maximum / minimum).
__device__ __forceinline__ uint32_t pack2_clamp_f16(float lo, float hi, uint32_t upper) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    typedef __attribute__((ext_vector_type(2))) float f2;
    f2 v = {lo, hi};
    h2 r = __builtin_convertvector(v, h2);
    const h2 zero = {(_Float16)0.f, (_Float16)0.f};
    r = __builtin_elementwise_maximum(r, zero);
    r = __builtin_elementwise_minimum(r, __builtin_bit_cast(h2, upper));
    return __builtin_bit_cast(uint32_t, r);
}
template <int DT> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    if constexpr (DT == PCV_BF16) return pack2_bf16(lo, hi);
    else return pack2_f16(lo, hi);
}
// unpack the two 16-bit elements of a dword
template <int DT> __device__ __forceinline__ void unpack2(uint32_t w, float& lo, float& hi) {
    if constexpr (DT == PCV_BF16) {
        lo = __uint_as_float(w << 16);
        hi = __uint_as_float(w & 0xFFFF0000u);
    } else {
        typedef __attribute__((ext_vector_type(2))) _Float16 h2;
        h2 v = *reinterpret_cast<h2*>(&w);
        lo = (float)v[0];
        hi = (float)v[1];
    }
}
template <int DT> __device__ __forceinline__ float load_elem(const void* base, size_t idx) {
    if constexpr (DT == PCV_F32) return reinterpret_cast<const float*>(base)[idx];
    else if constexpr (DT == PCV_BF16) return bf16_bits_to_f32(reinterpret_cast<const uint16_t*>(base)[idx]);
    else return (float)reinterpret_cast<const _Float16*>(base)[idx];
}
template <int DT> __device__ __forceinline__ void store_elem(void* base, size_t idx, float v) {
    if constexpr (DT == PCV_F32) reinterpret_cast<float*>(base)[idx] = v;
    else if constexpr (DT == PCV_BF16) reinterpret_cast<uint16_t*>(base)[idx] = (uint16_t)(pack2_bf16(v, 0.f) & 0xFFFFu);
    else reinterpret_cast<_Float16*>(base)[idx] = (_Float16)v;
}

// ---- fp16 range guard ------------------------------------------------------------------------------------
// fp16 storage rounds |v| >= 65520 to infinity, and a ReLU6 / sigmoid / h-sigmoid behind it clamps that infinity back into
// range: an overflow inside a net would come out as plausible finite logits. So every kernel that rounds fp32 results to fp16
// checks the magnitudes it rounds (one v_max3_f32 per two values; NaNs are ignored - they propagate by themselves) and bumps the context's overflow counter when one crossed fp16's range. pcv_fp16_guard_begin / _end
// (include/pcv_amd.h) turn a counter change during a forward into NaN logits. Compiled out for bf16 / fp32 storage.
//   A guard object is STAGE-LOCAL: declared where a kernel starts rounding a batch of results (an epilogue, one chunk of a fused
//   unit) and `commit()`ted at the end of that stage - one atomic from one lane if anything crossed the range. Two forms, measured
//   per kernel (MobileNetV3-large, fp16 against bf16, rocprofv3):
//     SCALAR = false: a per-lane running maximum in ONE vector register, one wave ballot at commit (4 VALU per eight values). The
//       default: generic / stem / depthwise / elementwise kernels (igemm h-swish layers +5 % against +9 % with the scalar form).
//     SCALAR = true: the verdict of every group is a wave ballot OR-ed into a scalar register pair - no vector state at all, one
//       compare more per group. For the register-bound fused-unit kernels (mbw.hpp: 233-256 registers): there the extra vector
//       register of the other form spilled inside the chunk loop (the wide dynamic-activation instance +45 % instead of +5 %).
//   (Declared at kernel scope instead of per stage, either form lived across the K loops and spilled 140-320 bytes.)
constexpr float kF16Overflow = 65520.f;
template <int OT, bool SCALAR = false> struct F16Guard {
    float m;
    unsigned long long hit;
    __device__ __forceinline__ F16Guard() : m(0.f), hit(0ull) {}
    __device__ __forceinline__ void note(float t) {
#ifndef PCV_NO_F16_GUARD      // timing experiments only (make EXTRA=-DPCV_NO_F16_GUARD): what the range check costs
        if constexpr (SCALAR) hit |= __builtin_amdgcn_ballot_w64(t >= kF16Overflow);
        else m = fmaxf(m, t);
#endif
    }
    __device__ __forceinline__ void see2(float a, float b) {
        if constexpr (OT == PCV_F16) note(fmaxf(fabsf(a), fabsf(b)));
    }
    template <int N> __device__ __forceinline__ void see(const float (&v)[N]) {
        static_assert(N % 2 == 0, "pairs");
        if constexpr (OT == PCV_F16) {
            float t = fmaxf(fabsf(v[0]), fabsf(v[1]));
#pragma unroll
            for (int e = 2; e < N; e += 2) t = fmaxf(fmaxf(fabsf(v[e]), fabsf(v[e + 1])), t);
            note(t);
        }
    }
    // `live`: false for a lane whose values are never stored and may be garbage (per-lane form only)
    __device__ __forceinline__ void commit(uint32_t* counter, bool live = true) {
        if constexpr (OT == PCV_F16) {
            const unsigned long long h = SCALAR ? hit : __builtin_amdgcn_ballot_w64(live && m >= kF16Overflow);
            if (h != 0ull && counter != nullptr) {
                const unsigned active = (unsigned)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true));      // one lane of those here
                if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == active) atomicAdd(counter, 1u);
            }
            m = 0.f;
            hit = 0ull;
        }
    }
};

// ---- activations (reference: pytorchcv/models/common/activ.py) ------------------------------------------
__device__ __forceinline__ float apply_act(float v, int act) {
    switch (act) {
        case PCV_ACT_RELU: return __builtin_elementwise_maximum(v, 0.f);           // activ.py:64 (NaN stays NaN, as in torch)
        case PCV_ACT_RELU6: return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, 0.f), 6.f);   // activ.py:81
        case PCV_ACT_SIGMOID: return __builtin_amdgcn_rcpf(1.f + __expf(-v));        // activ.py:132 (v_rcp_f32: 1 ulp)
        case PCV_ACT_SWISH: return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));      // activ.py:20-21
        case PCV_ACT_HSIGMOID: return v != v ? v : fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);      // activ.py:29-30
        case PCV_ACT_HSWISH: return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);    // activ.py:46-47
        case PCV_ACT_CLAMP01: return v != v ? v : fminf(fmaxf(v, 0.f), 1.f);             // ghostnet.py:23-24 (NaN stays NaN, as in torch.clamp)
        default: return v;
    }
}
// The common activations (none / relu / relu6) with launch-uniform codes: no activation is no instruction, ReLU is one
// v_maximum3_f32, ReLU6 adds one v_minimum3_f32 - gfx950's IEEE-754-2019 maximum / minimum, which PROPAGATE NaN like torch's
// relu / hardtanh (v_max_f32 / v_med3_f32 return the non-NaN operand, which would turn a NaN accumulator - corrupt weights,
// overflowed activations - into 0 and hide it from every isfinite check downstream). One uniform branch per group, none per element.
struct ActClamp {
    float lo, hi;
    bool slow;
    int code;
};
// true when a value that went through `act` (and nothing unbounded after it) lies in [0, 6]: the fp16 range check is skipped
__device__ __forceinline__ bool act_bounded(int act) { return act == PCV_ACT_RELU6 || act == PCV_ACT_SIGMOID || act == PCV_ACT_HSIGMOID; }
__device__ __forceinline__ ActClamp make_act(int act) {
    ActClamp a;
    a.code = act;
    a.slow = act > PCV_ACT_RELU6;
    a.lo = (act == PCV_ACT_RELU || act == PCV_ACT_RELU6) ? 0.f : -INFINITY;
    a.hi = act == PCV_ACT_RELU6 ? 6.f : INFINITY;
    return a;
}
template <int N> __device__ __forceinline__ void clampn(float (&v)[N], const ActClamp& a) {
    if (a.code == PCV_ACT_NONE) return;
    if (a.code == PCV_ACT_RELU) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = __builtin_elementwise_maximum(v[e], 0.f);
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = __builtin_elementwise_minimum(__builtin_elementwise_maximum(v[e], 0.f), 6.f);
    }
}
// the non-clamp activations: ONE uniform switch around a straight unrolled run per case (a switch per element costs eight
// scalar compare/branch sequences in every epilogue group)
template <int N> __device__ __forceinline__ void apply_slow_actn(float (&v)[N], int code) {
    switch (code) {
        case PCV_ACT_SIGMOID:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = __builtin_amdgcn_rcpf(1.f + __expf(-v[e]));
            break;
        case PCV_ACT_SWISH:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = v[e] * __builtin_amdgcn_rcpf(1.f + __expf(-v[e]));
            break;
        case PCV_ACT_HSIGMOID:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = v[e] != v[e] ? v[e] : fminf(fmaxf(v[e] + 3.f, 0.f), 6.f) * (1.f / 6.f);
            break;
        case PCV_ACT_HSWISH:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = v[e] * fminf(fmaxf(v[e] + 3.f, 0.f), 6.f) * (1.f / 6.f);
            break;
        default:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = apply_act(v[e], code);
    }
}
template <int N> __device__ __forceinline__ void apply_actn(float (&v)[N], const ActClamp& a) {
    if (a.slow) apply_slow_actn<N>(v, a.code);
    else clampn<N>(v, a);
}
__device__ __forceinline__ void clamp8(float (&v)[8], const ActClamp& a) { clampn<8>(v, a); }
__device__ __forceinline__ void apply_act8(float (&v)[8], const ActClamp& a) { apply_actn<8>(v, a); }

// ---- eight values of an epilogue: the 8 consecutive channels of one pixel that a lane owns (accumulators c0: + 0..3, c1: + 4..7) ----------
// v = acc * scale + shift, and the 16 bytes of a skip tensor added to it. Straight-line steps; the sequence around them (activations,
// range check, pack, store) stays in each kernel (conv_device.hpp, mb_device.hpp).
__device__ __forceinline__ void bn8(float (&v)[8], const f32x4& c0, const f32x4& c1, const f32x4& s0, const f32x4& s1, const f32x4& h0,
                                    const f32x4& h1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = c0[e] * s0[e] + h0[e];
        v[4 + e] = c1[e] * s1[e] + h1[e];
    }
}
template <int DT> __device__ __forceinline__ void add_skip8(float (&v)[8], const u32x4& skip) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float lo, hi;
        unpack2<DT>(skip[e], lo, hi);
        v[2 * e] += lo;
        v[2 * e + 1] += hi;
    }
}

// ---- exact unsigned division by a launch-time constant, n < 2^31 ----------------------------------------
struct FastDiv {
    uint32_t d, magic, shift;
};
static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    if (d <= 1) { f.magic = 0; f.shift = 0; return f; }
    uint32_t sh = 0;
    while ((1ull << (sh + 1)) < d) ++sh;          // 2^sh < d <= 2^(sh+1)
    f.shift = sh;
    f.magic = (uint32_t)(((1ull << (32 + sh)) + d - 1) / d);
    return f;
}
__device__ __forceinline__ uint32_t fastdiv(uint32_t n, const FastDiv& f) {
    return f.d <= 1 ? n : (__umulhi(n, f.magic) >> f.shift);
}

// XCD-aware logical tile id: blocks b and b+8 share an XCD (observed round-robin dispatch), so give each XCD a
// contiguous run of logical tiles. Bijective for any tile count (cdna_hip_programming.md section 5, T1).
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nwg) {
    const uint32_t q = nwg >> 3, r = nwg & 7u, xcd = b & 7u, idx = b >> 3;
    const uint32_t start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

// eight consecutive elements at a plain pointer as fp32 and back (the element-wise kernels, the 8-channel depthwise chunks)
template <int DT> __device__ __forceinline__ void load8(const void* base, size_t eidx, float (&v)[8]) {
    if constexpr (DT == PCV_F32) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + eidx);
        const f32x4 b = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + eidx + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
    } else {
        const u32x4 r = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(base) + eidx);
#pragma unroll
        for (int e = 0; e < 4; ++e) unpack2<DT>(r[e], v[2 * e], v[2 * e + 1]);
    }
}
// (nt: a launch-uniform streaming store - the line is not kept for a reader that never comes; fp32 stores never took it)
template <int DT> __device__ __forceinline__ void store8(void* base, size_t eidx, const float (&v)[8], bool nt = false) {
    if constexpr (DT == PCV_F32) {
        float* p = reinterpret_cast<float*>(base) + eidx;
        *reinterpret_cast<f32x4*>(p) = (f32x4){v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + 4) = (f32x4){v[4], v[5], v[6], v[7]};
    } else {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack2<DT>(v[2 * e], v[2 * e + 1]);
        u32x4* q = reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(base) + eidx);
        if (nt) __builtin_nontemporal_store(o, q);
        else *q = o;
    }
}
