// dw_device.hpp - what the depthwise kernels share (dwconv.hpp, mixconv.hpp, ghost.hpp), where one thread owns CPT consecutive
// channels of one output column:
//   * the raw CPT-channel chunk of a range-checked buffer load (1, 2, 4 or 8 dwords) and its unpack to packed fp32 pairs;
//   * loadn / storen at plain pointers for 2, 4 and 8 channels (the 8-channel case is load8 / store8 of pcv_common.hpp);
//   * pk_fma_acc / pk_mul: v_pk_fma_f32 / v_pk_mul_f32 by name;
//   * dw_decode: flat thread index -> (chunk, column, strip, image) and the strip's rows;
//   * dw_load_taps / dw_load_bn: the taps and the folded scale / shift of the thread's channels as fp32 pairs;
//   * dw_bn / dw_act / dw_add_res: the epilogue's pieces, in the order every kernel applies them;
//   * dw_stream_rows: the row-streaming core (dwconv5_kernel of dwconv.hpp, every window class of mixconv.hpp).
// The two register-window 3x3 kernels (dwconv_kernel, ghost_dw_kernel) keep their own tap / scale / shift loads and row-fetch
// lambda, and the ghost kernel its residual add: through the shared functions their code changed
// (profiles/experiments/dw_device_refactor.md has the helper-by-helper record).
#pragma once
#include <type_traits>
#include <utility>
#include "pcv_common.hpp"

// raw CPT-channel chunk as it comes from memory: ND = CPT dwords at fp32, CPT / 2 at 16 bit. The dwords stay in the vector
// registers the load wrote (a scalar array here costs the stride-1 3x3 kernel 14 %: measured).
template <int ND> struct RawVec;
template <> struct RawVec<8> { u32x4 q[2]; __device__ __forceinline__ uint32_t get(int i) const { return q[i >> 2][i & 3]; } };
template <> struct RawVec<4> { u32x4 q[1]; __device__ __forceinline__ uint32_t get(int i) const { return q[0][i]; } };
template <> struct RawVec<2> { u32x2 q[1]; __device__ __forceinline__ uint32_t get(int i) const { return q[0][i]; } };
template <> struct RawVec<1> { uint32_t q[1]; __device__ __forceinline__ uint32_t get(int) const { return q[0]; } };
template <int DT, int CPT> struct RawChunk : RawVec<(DT == PCV_F32 ? CPT : CPT / 2)> {};

#if defined(__HIP_DEVICE_COMPILE__)
template <int DT, int CPT>
__device__ __forceinline__ void raw_load(const __amdgpu_buffer_rsrc_t& rsrc, uint32_t off, RawChunk<DT, CPT>& r) {
    constexpr int ND = DT == PCV_F32 ? CPT : CPT / 2;
    if constexpr (ND == 8) {
        r.q[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
        r.q[1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 16, 0);
    } else if constexpr (ND == 4) {
        r.q[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
    } else if constexpr (ND == 2) {
        r.q[0] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
    } else {
        r.q[0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
    }
}
#endif

// CPT channels as CPT/2 packed pairs: the FMAs lower to v_pk_fma_f32 (two lanes of fp32 per instruction)
template <int DT, int CPT> __device__ __forceinline__ void raw_to_f32x2(const RawChunk<DT, CPT>& r, f32x2 (&v)[CPT / 2]) {
#pragma unroll
    for (int e = 0; e < CPT / 2; ++e) {
        if constexpr (DT == PCV_F32) {
            v[e] = (f32x2){__uint_as_float(r.get(2 * e)), __uint_as_float(r.get(2 * e + 1))};
        } else {
            float lo, hi;
            unpack2<DT>(r.get(e), lo, hi);
            v[e] = (f32x2){lo, hi};
        }
    }
}

// load / store CPT = 2, 4 or 8 consecutive elements as fp32 (plain pointers: taps, scale / shift, residual, output)
template <int DT, int CPT> __device__ __forceinline__ void loadn(const void* base, size_t eidx, float (&v)[CPT]) {
    if constexpr (CPT == 8) {
        load8<DT>(base, eidx, v);
    } else if constexpr (DT == PCV_F32 && CPT == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + eidx);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = a[e];
    } else if constexpr (DT == PCV_F32) {
        const f32x2 a = *reinterpret_cast<const f32x2*>(reinterpret_cast<const float*>(base) + eidx);
        v[0] = a[0];
        v[1] = a[1];
    } else if constexpr (CPT == 4) {
        const u32x2 r = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(base) + eidx);
        unpack2<DT>(r[0], v[0], v[1]);
        unpack2<DT>(r[1], v[2], v[3]);
    } else {
        unpack2<DT>(*reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(base) + eidx), v[0], v[1]);
    }
}
// nt (a launch-uniform streaming store) is taken by the 4-channel stores of both widths and by the 8-channel 16-bit store; the
// 8-channel fp32 store and both 2-channel stores ignore it. Which launches pass it is written at the calls.
template <int DT, int CPT> __device__ __forceinline__ void storen(void* base, size_t eidx, const float (&v)[CPT], bool nt = false) {
    if constexpr (CPT == 8) {
        store8<DT>(base, eidx, v, nt);
    } else if constexpr (DT == PCV_F32 && CPT == 4) {
        f32x4* q = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + eidx);
        const f32x4 o = {v[0], v[1], v[2], v[3]};
        if (nt) __builtin_nontemporal_store(o, q);
        else *q = o;
    } else if constexpr (DT == PCV_F32) {
        *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(base) + eidx) = (f32x2){v[0], v[1]};
    } else if constexpr (CPT == 4) {
        u32x2* q = reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(base) + eidx);
        const u32x2 o = {pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3])};
        if (nt) __builtin_nontemporal_store(o, q);
        else *q = o;
    } else {
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(base) + eidx) = pack2<DT>(v[0], v[1]);
    }
}
// the same as packed fp32 pairs
template <int DT, int CPT> __device__ __forceinline__ void loadn2(const void* base, size_t eidx, f32x2 (&v)[CPT / 2]) {
    float f[CPT];
    loadn<DT, CPT>(base, eidx, f);
#pragma unroll
    for (int e = 0; e < CPT / 2; ++e) v[e] = (f32x2){f[2 * e], f[2 * e + 1]};
}

// acc += a * b on two fp32 lanes per instruction. hipcc scalarises most `__builtin_elementwise_fma` on float2 here, so the
// instruction is named directly (pure register-to-register, no memory, no hazards with the surrounding VALU code).
__device__ __forceinline__ void pk_fma_acc(f32x2& acc, const f32x2& a, const f32x2& b) {
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ f32x2 pk_mul(const f32x2& a, const f32x2& b) {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Thread decode. Lanes run over channel chunks first, then output columns (every wave-level access is one contiguous NHWC span),
// then row strips of TH output rows, then images.
struct DwThread {
    int chunk, wo, n;
    int ho_begin, ho_end;     // the strip's output rows
};
__device__ __forceinline__ DwThread dw_decode(long idx, int nchunk, int Wo, int nseg, int TH, int Ho) {
    DwThread t;
    t.chunk = (int)(idx % nchunk);
    long r = idx / nchunk;
    t.wo = (int)(r % Wo);
    r /= Wo;
    const int seg = (int)(r % nseg);
    t.n = (int)(r / nseg);
    t.ho_begin = seg * TH;
    t.ho_end = min(Ho, t.ho_begin + TH);
    return t;
}

// taps [NT][pitch] in DT -> wgt[k] = the pairs of channels [c, c + CPT) of tap k; scale / shift [.] fp32 -> sc, sf
template <int DT, int NT, int CPT>
__device__ __forceinline__ void dw_load_taps(const void* w, int pitch, int c, f32x2 (&wgt)[NT][CPT / 2]) {
#pragma unroll
    for (int k = 0; k < NT; ++k) loadn2<DT, CPT>(w, (size_t)k * pitch + c, wgt[k]);
}
template <int CPT>
__device__ __forceinline__ void dw_load_bn(const float* scale, const float* shift, int c, f32x2 (&sc)[CPT / 2], f32x2 (&sf)[CPT / 2]) {
    loadn2<PCV_F32, CPT>(scale, c, sc);
    loadn2<PCV_F32, CPT>(shift, c, sf);
}

// epilogue pieces: v = acc * scale + shift; the activation (FAST: a clamp - none / relu / relu6; else every code, whose
// transcendental code stays out of the hot build); v += residual. Then guard.see(v) unless bounded, and storen.
template <int CPT>
__device__ __forceinline__ void dw_bn(const f32x2 (&acc)[CPT / 2], const f32x2 (&sc)[CPT / 2], const f32x2 (&sf)[CPT / 2], float (&v)[CPT]) {
#pragma unroll
    for (int e = 0; e < CPT / 2; ++e) {
        f32x2 t2 = sf[e];
        pk_fma_acc(t2, acc[e], sc[e]);
        v[2 * e] = t2[0];
        v[2 * e + 1] = t2[1];
    }
}
template <bool FAST, int CPT> __device__ __forceinline__ void dw_act(float (&v)[CPT], const ActClamp& a) {
    if constexpr (FAST) clampn(v, a); else apply_actn(v, a);
}
template <int DT, int CPT> __device__ __forceinline__ void dw_add_res(const void* res, size_t eoff, float (&v)[CPT]) {
    float r[CPT];
    loadn<DT, CPT>(res, eoff, r);
#pragma unroll
    for (int e = 0; e < CPT; ++e) v[e] += r[e];
}

// ---- the row-streaming core ---------------------------------------------------------------------------------------------------------
// A thread keeps ONE input row of its KS columns plus one accumulator per in-flight output row (NSLOT = ceil(KS / S) of them) and
// feeds input row t of the strip into output row (t - dy) / S through filter row dy: KS loads per output row like the register
// window of dwconv_kernel, without KS * KS input chunks live beside the KS * KS taps (200 registers at 5x5, which spilled).
// Where the taps live - fp32 pairs (KS <= 7), packed 16-bit pairs unpacked on use, or re-read per filter row through the vector L1 -
// is mixconv.hpp's table; the 9x9 / 11x11 forms hand their input row over by register copies instead of the static ring.
struct DwStream {
    const void* x;
    uint32_t x_bytes;
    const void* w;            // the taps [KS * KS][wpitch] in DT; the thread's channels start at column wc
    int wpitch, wc;
    const float* scale;
    const float* shift;
    const void* res;          // RES only
    void* y;
    int H, W, C, Ho, Wo;
    int pt, pl;               // top / left padding
    int act, post_act;        // post_act: RES only
    uint32_t* ovf;
};
// RES: the epilogue with the optional residual and post-activation (dwconv5_kernel); without it the activation alone (MixConv)
template <int DT, int KS, int S, bool FAST, int CPT, bool RES>
__device__ __forceinline__ void dw_stream_rows(const DwStream& a, const DwThread& th, const int c0) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NV = CPT / 2;
    constexpr int ES = Elem<DT>::BYTES;
    constexpr int NSLOT = (KS + S - 1) / S;        // output rows in flight
    constexpr int PERIOD = S * NSLOT;              // input rows after which the (phase -> slot) pattern repeats
    const int n = th.n, wo = th.wo, ho_begin = th.ho_begin;
    const int nrows = th.ho_end - th.ho_begin;

    constexpr bool WREG = KS <= 7;                 // taps resident in registers (else: fetched per filter row, see mixconv.hpp)
    const char* wbase = static_cast<const char*>(a.w);
    const int span = a.wpitch, cr = a.wc;
    f32x2 wgt[WREG ? KS * KS : 1][NV];
    if constexpr (WREG) dw_load_taps<DT, KS * KS, CPT>(wbase, span, cr, wgt);
    // 9 x 9 / 11 x 11 at 16 bit: the taps stay resident too, but as they are stored - one dword per pair - and are unpacked on use
    constexpr bool WPK = !WREG && DT != PCV_F32;
    uint32_t wpk[WPK ? KS * KS : 1];
    if constexpr (WPK) {
        static_assert(CPT == 2, "one dword per tap");
#pragma unroll
        for (int k = 0; k < KS * KS; ++k) wpk[k] = *reinterpret_cast<const uint32_t*>(wbase + ((size_t)k * span + cr) * ES);
    }
    f32x2 sc[NV], sf[NV];
    dw_load_bn<CPT>(a.scale, a.shift, c0, sc, sf);
    const ActClamp act = make_act(a.act), pact = make_act(RES ? a.post_act : PCV_ACT_NONE);
    F16Guard<DT> guard;
    bool bounded;
    if constexpr (RES) bounded = act_bounded(a.post_act) || (a.post_act == PCV_ACT_NONE && a.res == nullptr && act_bounded(a.act));
    else bounded = act_bounded(a.act);

    // per-column byte offsets (relative to the row start) or out of range: a padded tap reads zeros, no branches
    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(a.x, a.x_bytes);
    const int wi0 = wo * S - a.pl;
    uint32_t coloff[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q)
        coloff[q] = (unsigned)(wi0 + q) < (unsigned)a.W ? (uint32_t)(((wi0 + q) * a.C + c0) * ES) : kOutOfRange;
    const uint32_t rowbytes = (uint32_t)(a.W * a.C * ES);
    const uint32_t imgoff = (uint32_t)n * (uint32_t)a.H * rowbytes;
    auto fetch_row = [&](int hi, bool need, RawChunk<DT, CPT> (&row)[KS]) {      // need: false for rows beyond the strip
        const bool rowok = need && (unsigned)hi < (unsigned)a.H;
        const uint32_t rbase = imgoff + (uint32_t)hi * rowbytes;
#pragma unroll
        for (int q = 0; q < KS; ++q)
            raw_load<DT, CPT>(xrsrc, (rowok && coloff[q] != kOutOfRange) ? rbase + coloff[q] : kOutOfRange, row[q]);
    };

    f32x2 acc[NSLOT][NV];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s)
#pragma unroll
        for (int e = 0; e < NV; ++e) acc[s][e] = (f32x2){0.f, 0.f};

    const int hi_first = ho_begin * S - a.pt;
    const int nsteps = (nrows - 1) * S + KS;       // input rows this strip touches
    // input rows live in a ring with one slot per phase of the unroll period: the row of step t sits in ring[t % PERIOD] and the
    // row PD steps ahead is requested into its own (static) slot - no register copies, nothing waits on the newest loads
    // (the 9 x 9 and 11 x 11 classes keep two rows only - the current one and the next, handed over by register copies: a ring of
    // PERIOD static slots stays live as a whole across the conditional phases, 264 registers for 11 x 11 at fp32, and their ~100
    // packed FMAs per step cover the one row of latency that the copy leaves)
    constexpr int PD = WREG ? 2 : 1;
    RawChunk<DT, CPT> ring[WREG ? PERIOD : 2][KS];
    if constexpr (WREG) {
#pragma unroll
        for (int d = 0; d < PD; ++d) fetch_row(hi_first + d, d < nsteps, ring[d]);
    } else {
        fetch_row(hi_first, true, ring[1]);
    }
    int t = 0;
    while (t < nsteps) {
        static_for<PERIOD>([&](auto PHC) {
            constexpr int PH = decltype(PHC)::value;
            if (t < nsteps) {
                constexpr int CUR = WREG ? PH : 0;
                if constexpr (WREG) {
                    fetch_row(hi_first + t + PD, t + PD < nsteps, ring[(PH + PD) % PERIOD]);
                } else {
#pragma unroll
                    for (int q = 0; q < KS; ++q) ring[0][q] = ring[1][q];
                    fetch_row(hi_first + t + 1, t + 1 < nsteps, ring[1]);
                }
                f32x2 xv[KS][NV];
#pragma unroll
                for (int q = 0; q < KS; ++q) raw_to_f32x2<DT, CPT>(ring[CUR][q], xv[q]);
#pragma unroll
                for (int dy = 0; dy < KS; ++dy) {
                    const int d = PH - dy;                                 // S * (output row), modulo the unroll period
                    if (S == 1 || (d & 1) == 0) {                          // stride 2: this input row only meets every other filter row
                        const int slot = (((S == 1 ? d : d / 2) % NSLOT) + NSLOT) % NSLOT;
                        if (t - dy >= 0) {
                            if constexpr (WREG) {
#pragma unroll
                                for (int q = 0; q < KS; ++q)
#pragma unroll
                                    for (int e = 0; e < NV; ++e) pk_fma_acc(acc[slot][e], xv[q][e], wgt[dy * KS + q][e]);
                            } else if constexpr (WPK) {
#pragma unroll
                                for (int q = 0; q < KS; ++q) {
                                    // (a copy the compiler cannot see through: the unpacked pair is loop-invariant, and hoisted out
                                    // of the row loop the pairs would take the 2 x KS x KS registers this form exists to save)
                                    uint32_t wv = wpk[dy * KS + q];
                                    asm volatile("" : "+v"(wv));
                                    float lo, hi;
                                    unpack2<DT>(wv, lo, hi);
                                    const f32x2 w2 = {lo, hi};
                                    pk_fma_acc(acc[slot][0], xv[q][0], w2);
                                }
                            } else {
                                // (the offset is made opaque per step: the taps are loop-invariant, and hoisted out of the row loop
                                // they would all be live at once again - the registers this form exists to save)
                                uint32_t wcol = (uint32_t)cr;
                                asm volatile("" : "+v"(wcol));
                                f32x2 wrow[KS][NV];
#pragma unroll
                                for (int q = 0; q < KS; ++q) loadn2<DT, CPT>(wbase, (size_t)(dy * KS + q) * span + wcol, wrow[q]);
#pragma unroll
                                for (int q = 0; q < KS; ++q)
#pragma unroll
                                    for (int e = 0; e < NV; ++e) pk_fma_acc(acc[slot][e], xv[q][e], wrow[q][e]);
                                __builtin_amdgcn_sched_barrier(0);      // one filter row of taps in flight, not all the step's
                            }
                        }
                    }
                }
                // the output row whose last filter row (dy = KS - 1) was this input row is complete
                {
                    const int d = PH - (KS - 1);
                    if (S == 1 || (d & 1) == 0) {
                        const int slot = (((S == 1 ? d : d / 2) % NSLOT) + NSLOT) % NSLOT;
                        const int o2 = t - (KS - 1);
                        if (o2 >= 0) {
                            const int o = o2 / S;
                            if (o < nrows) {
                                const size_t eoff = (((size_t)n * a.Ho + ho_begin + o) * a.Wo + wo) * a.C + c0;
                                float v[CPT];
                                dw_bn<CPT>(acc[slot], sc, sf, v);
                                dw_act<FAST>(v, act);
                                if constexpr (RES) {
                                    if (a.res != nullptr) dw_add_res<DT, CPT>(a.res, eoff, v);
                                    if (a.post_act != PCV_ACT_NONE) dw_act<FAST>(v, pact);
                                }
                                if (!bounded) guard.see(v);
                                // (dw_flags bit 0, non-temporal stores, has never reached the 2- and 4-channel stores of these kernels: kept)
                                storen<DT, CPT>(a.y, eoff, v);
                            }
#pragma unroll
                            for (int e = 0; e < NV; ++e) acc[slot][e] = (f32x2){0.f, 0.f};
                        }
                    }
                }
                ++t;
            }
        });
    }
    guard.commit(a.ovf);
#endif  // __HIP_DEVICE_COMPILE__
}
