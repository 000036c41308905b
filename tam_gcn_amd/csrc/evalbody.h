// Device bodies shared by the training-side kernels of stemhead.hip (ce_fwd_kernel, score_fuse_kernel) and the evaluation-side
// kernels of evalmeter.hip (eval_accumulate_kernel, score_sweep_kernel).  One definition each, so that a loss the meter
// accumulates is the loss tamgcn_ce_fwd returns for the same rows, bit for bit, and an alpha sweep fuses as tamgcn_score_fuse does.
#pragma once
#include "common.h"

constexpr int CE_NT = 256;                      // the ONE workgroup of the cross-entropy kernels: thread -> rows n = tid, tid + 256, ...
constexpr long long CE_IGNORE_INDEX = -100;     // torch's default ignore_index

// kept = rows with a label in [0, K), nbad = rows with any other label than ignore_index, over rows [0, N); all threads get both
struct CeCount { int kept, nbad; };
__device__ __forceinline__ CeCount ce_count_labels(const long long* labels, int N, int K, int* cnt, int* bad) {
    int kept = 0, nbad = 0;
    for (int n = threadIdx.x; n < N; n += CE_NT) {
        const long long y = labels[n];
        if (y >= 0 && y < K) ++kept;
        else if (y != CE_IGNORE_INDEX) ++nbad;
    }
    cnt[threadIdx.x] = kept;
    bad[threadIdx.x] = nbad;
    __syncthreads();
    for (int o = CE_NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) { cnt[threadIdx.x] += cnt[threadIdx.x + o]; bad[threadIdx.x] += bad[threadIdx.x + o]; }
        __syncthreads();
    }
    return {cnt[0], bad[0]};
}

// log-sum-exp of one row by max-shift: lse = m + log(s), s the shifted sum (the gradient needs m and s too)
struct CeRow { float m, s, lse; };
__device__ __forceinline__ CeRow ce_row_lse(const float* l, int K) {
    float m = l[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, l[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(l[k] - m);
    return {m, s, m + logf(s)};
}

// sum of the threads' fp64 partial sums in a fixed order; valid in thread 0 (red[0])
__device__ __forceinline__ double ce_block_sum(double acc, double* red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = CE_NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ float ce_mean(double total, int kept, int nbad) {
    return (nbad || kept == 0) ? __builtin_nanf("") : (float)(total / (double)kept);
}

// ---- score fusion: term s of fused[k] is w[s] * (softmax ? softmax_k(x) : x[k]), added with separate roundings ----
__device__ __forceinline__ void fuse_softmax_stats(const float* x, int K, int softmax, float& mx, float& inv) {
    mx = 0.f;
    inv = 1.f;
    if (softmax) {
        mx = x[0];
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
        float den = 0.f;
        for (int k = 0; k < K; ++k) den += expf(x[k] - mx);
        inv = 1.f / den;
    }
}
// separate multiply and add (no fma contraction): numpy evaluates score_a + (alpha * score_b) with both roundings.
// __fmul_rn / __fadd_rn are plain * and + in the HIP headers and, once inlined, were contracted to one v_fmac_f32 (one rounding);
// the pragma takes the contract flag off this function's operations, which the inliner keeps.
__device__ __forceinline__ float fuse_add(float f, float ws, const float* x, int k, int softmax, float mx, float inv) {
#pragma clang fp contract(off)
    const float term = softmax ? expf(x[k] - mx) * inv : x[k];
    const float prod = ws * term;
    return f + prod;
}
