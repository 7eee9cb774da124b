// classify_kernel.hpp - what follows the logits: top-k ids / values / softmax probabilities, the label's rank and its negative
// log-likelihood, one launch for the batch. The reference keeps this out of tree (the imgclsmob scripts); what it replaces are the
// Top1 / Top5 columns of the reference README and of models/common/model_metainfos.csv, which those scripts produced with
// torch.topk - whose order among equal logits is unspecified. Here ONE total order "a precedes b" defines every output:
//     NaN above +inf; otherwise the larger value first; equal values by lower index first; all NaNs tie; -0.0 ties with +0.0.
// A float maps to a sortable uint32 (NaN canonicalised to the top, -0 to +0) and an entry to the 64-bit key (ukey << 32) | ~index,
// so "a precedes b" is key(a) > key(b), keys of one row are distinct, and no key is 0 (the smallest ukey, -inf's, is 0x007FFFFF).
//
// One workgroup per row, the row staged in LDS once; every pass below walks LDS with stride NT and ends in one block reduction:
//   pass A   arg-best = the largest key. Its value is the row maximum m (a NaN, if the row has one: everything after it is NaN then,
//            which is what torch.softmax gives - NaN, +inf and all -inf rows are NOT special-cased, inf - inf does it).
//   pass B   sum of expf(x - m) over the whole row, fp32 (top_prob / nll only).
//   pass C   rank = how many keys are larger than the label's (exact for every k at once: top-k error = count(rank >= k)).
//   picks    pick 0 is pass A's; pick p is the largest key strictly below pick p-1 - k-1 more passes, k <= 32.
// NT = 64 (one wave, no barrier inside a reduction) for rows of at most 1024 entries, 256 above. The reductions are xor butterflies
// inside a wave (both partners compute the same commutative operation, so all lanes agree) and a fixed left-to-right walk over the
// waves' results: no atomics, and a row's outputs do not depend on where the row sits in the batch or on the grid size.
#pragma once
#include "pcv_common.hpp"

constexpr int kClassifyMaxJ = 16384;            // a row is 64 KB of LDS
constexpr int kClassifyMaxK = 32;
constexpr int kClassifyRedBytes = 32;           // 4 waves x 8 bytes in front of the row

__device__ __forceinline__ uint32_t classify_ukey(float x) {
    uint32_t b = __float_as_uint(x);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;                // every NaN
    if (b == 0x80000000u) b = 0u;                                           // -0 ties with +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long classify_key(float x, int i) {
    return ((unsigned long long)classify_ukey(x) << 32) | (unsigned long long)(~(uint32_t)i);
}
__device__ __forceinline__ int classify_index(unsigned long long key) { return (int)(~(uint32_t)key); }

struct ClassifyMax {
    __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; }
};
struct ClassifyAdd {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// every thread of the block gets the result; `red` is the block's 4-slot scratch
template <int NT, class T, class Op>
__device__ __forceinline__ T classify_reduce(T v, Op op, void* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o));
    if (NT > 64) {
        T* r = static_cast<T*>(red);
        __syncthreads();                                                    // the previous reduction's readers are done
        if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
        __syncthreads();
        v = r[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v = op(v, r[w]);
    }
    return v;
}

template <int NT>
__global__ __launch_bounds__(NT) void classify_kernel(const float* __restrict__ logits, int N, int J, int k, int* __restrict__ top_idx,
                                                      uint32_t* __restrict__ top_val, float* __restrict__ top_prob,
                                                      const long long* __restrict__ labels, int* __restrict__ rank,
                                                      float* __restrict__ nll) {
    extern __shared__ __attribute__((aligned(16))) unsigned char classify_lds[];
    void* red = classify_lds;
    float* row = reinterpret_cast<float*>(classify_lds + kClassifyRedBytes);
    const int tid = threadIdx.x;
    const bool need_sum = top_prob != nullptr || nll != nullptr;
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const float* x = logits + (size_t)n * J;
        __syncthreads();                                                    // the previous row's readers are done
        for (int i = tid; i < J; i += NT) row[i] = x[i];
        __syncthreads();

        unsigned long long best = 0;
        for (int i = tid; i < J; i += NT) best = ClassifyMax()(best, classify_key(row[i], i));
        best = classify_reduce<NT>(best, ClassifyMax(), red);
        const float m = row[classify_index(best)];

        float sum = 0.0f;
        if (need_sum) {
            for (int i = tid; i < J; i += NT) sum += expf(row[i] - m);
            sum = classify_reduce<NT>(sum, ClassifyAdd(), red);
        }

        if (labels != nullptr && (rank != nullptr || nll != nullptr)) {
            const long long lab = labels[n];
            const bool ok = lab >= 0 && lab < (long long)J;                 // block-uniform
            if (rank != nullptr) {
                int before = J;
                if (ok) {
                    const unsigned long long kl = classify_key(row[lab], (int)lab);
                    before = 0;
                    for (int i = tid; i < J; i += NT) before += classify_key(row[i], i) > kl ? 1 : 0;
                    before = classify_reduce<NT>(before, ClassifyAdd(), red);
                }
                if (tid == 0) rank[n] = before;
            }
            if (nll != nullptr && tid == 0) nll[n] = ok ? logf(sum) + m - row[lab] : __uint_as_float(0x7F800000u);
        }

        unsigned long long pick = best;
        for (int p = 0; p < k; ++p) {
            if (p > 0) {                                                    // k <= J: there is always an entry after the previous pick
                unsigned long long b = 0;
                for (int i = tid; i < J; i += NT) {
                    const unsigned long long key = classify_key(row[i], i);
                    b = (key < pick && key > b) ? key : b;
                }
                pick = classify_reduce<NT>(b, ClassifyMax(), red);
            }
            if (tid == 0) {
                const int idx = classify_index(pick);
                const size_t o = (size_t)n * k + p;
                if (top_idx != nullptr) top_idx[o] = idx;
                if (top_val != nullptr) top_val[o] = __float_as_uint(row[idx]);     // the input's bits, NaN payload and sign of zero kept
                if (top_prob != nullptr) top_prob[o] = expf(row[idx] - m) / sum;
            }
        }
    }
}
