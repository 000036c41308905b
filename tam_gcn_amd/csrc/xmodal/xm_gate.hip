// The gate layer of the cross-modal head: att = sigmoid(a1 W2^T + b2) and its backward (dW2, db2, da1).
#include "xm_common.h"

// dW2 (R, Hd) = dz2^T a1 and db2 = sum_n dz2: one wave per 16 x 16 tile of dW2, the whole contraction (the N clips, in order) in
// that wave.  Both operands have the clip as their leading dimension: dword loads, 16 lanes wide.  The waves of the first
// column tile also sum their 16 columns of dz2 for db2, clip by clip.
__global__ __launch_bounds__(256) void xm_gate_wgrad(const float* __restrict__ dz2, const float* __restrict__ a1, int N, int Hd, int R,
                                                      float* __restrict__ dW2, float* __restrict__ db2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int nct = (Hd + 15) / 16, tile = blockIdx.x * 4 + wave;
    const int rt = tile / nct, ct = tile - rt * nct;
    if (rt >= (R + 15) / 16) return;                       // no barrier below
    const int rr = min(rt * 16 + i, R - 1), cc = min(ct * 16 + i, Hd - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < N; kb += 16) {
        const int k = kb + 4 * q;
        acc = xm_mma16(xm_frag_colk(dz2, R, rr, k, N), xm_frag_colk(a1, Hd, cc, k, N), acc);
    }
    const int col = ct * 16 + i;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = rt * 16 + 4 * q + reg;
        if (row < R && col < Hd) dW2[(size_t)row * Hd + col] = acc[reg];
    }
    if (ct == 0 && lane < 16 && rt * 16 + lane < R) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += dz2[(size_t)n * R + rt * 16 + lane];
        db2[rt * 16 + lane] = s;
    }
}

extern "C" int tamgcn_xm_gate_fwd(const float* a1, const float* W2, const float* b2, int N, int Hd, int R, float* att, void* stream) {
    XM_CHECK_N("tamgcn_xm_gate_fwd", N);
    XM_CHECK_W("tamgcn_xm_gate_fwd", "Hd", Hd);
    XM_CHECK_W("tamgcn_xm_gate_fwd", "R", R);
    XM_CHECK_P16("tamgcn_xm_gate_fwd", "a1", a1);
    XM_CHECK_P16("tamgcn_xm_gate_fwd", "W2", W2);
    XM_CHECK_P16("tamgcn_xm_gate_fwd", "b2", b2);
    XM_CHECK_P16("tamgcn_xm_gate_fwd", "att", att);
    const dim3 grid(ceil_div(R, 16), ceil_div(ceil_div(N, 16), 4));
    hipLaunchKernelGGL((xm_gemm_ksplit<true, true>), grid, dim3(256), 0, (hipStream_t)stream, a1, W2, b2, N, R, Hd, att);
    XM_LAUNCH_CHECK("tamgcn_xm_gate_fwd");
    return 0;
}

extern "C" int tamgcn_xm_gate_bwd(const float* dz2, const float* a1, const float* W2, int N, int Hd, int R,
                                  float* dW2, float* db2, float* da1, void* stream) {
    XM_CHECK_N("tamgcn_xm_gate_bwd", N);
    XM_CHECK_W("tamgcn_xm_gate_bwd", "Hd", Hd);
    XM_CHECK_W("tamgcn_xm_gate_bwd", "R", R);
    XM_CHECK_P16("tamgcn_xm_gate_bwd", "dz2", dz2);
    XM_CHECK_P16("tamgcn_xm_gate_bwd", "a1", a1);
    XM_CHECK_P16("tamgcn_xm_gate_bwd", "W2", W2);
    XM_CHECK_P16("tamgcn_xm_gate_bwd", "dW2", dW2);
    XM_CHECK_P16("tamgcn_xm_gate_bwd", "db2", db2);
    XM_CHECK_P16("tamgcn_xm_gate_bwd", "da1", da1);
    const int tiles = ceil_div(R, 16) * ceil_div(Hd, 16);
    hipLaunchKernelGGL(xm_gate_wgrad, dim3(ceil_div(tiles, 4)), dim3(256), 0, (hipStream_t)stream, dz2, a1, N, Hd, R, dW2, db2);
    XM_LAUNCH_CHECK("tamgcn_xm_gate_bwd (dW2)");
    const dim3 grid(ceil_div(Hd, 16), ceil_div(ceil_div(N, 16), 4));
    hipLaunchKernelGGL((xm_gemm_ksplit<false, false>), grid, dim3(256), 0, (hipStream_t)stream, dz2, W2, (const float*)nullptr, N, Hd, R, da1);
    XM_LAUNCH_CHECK("tamgcn_xm_gate_bwd (da1)");
    return 0;
}
