// The hidden layer of the cross-modal head: a1 = relu(BatchNorm1d(f W1^T + b1)) in one launch, and its backward.
// A workgroup owns 16 hidden units for ALL N clips: their pre-activations (forward) or gradients (backward) live in LDS as
// [N][16] (64 KB at N = 1024), so the per-unit sums over the batch never leave the workgroup -- no partial sums in memory, no
// second launch, no atomics, and a summation order that depends on N alone.
#include "xm_common.h"

constexpr int XM_RED = 512;                       // two 16 x 16 tables of partial column sums
static inline size_t xm_hidden_lds(int N) { return sizeof(float) * ((size_t)N * 16 + XM_RED + 32); }

// sum over the 16 row groups of a [16][16] table of partial sums (group-major), for the 16 columns, by threads 0..15
__device__ __forceinline__ float xm_colsum16(const float* red, int col) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g * 16 + col];
    return t;
}

__global__ __launch_bounds__(256) void xm_hidden_fwd_kernel(const float* __restrict__ f, const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float* rmean, float* rvar,
                                                             long long* nbt, int N, int D, int Hd, int training, float momentum, float eps,
                                                             float* __restrict__ a1, float* __restrict__ xhat, float* __restrict__ mean,
                                                             float* __restrict__ invstd) {
    extern __shared__ __attribute__((aligned(16))) float xm_lds[];
    float* zs = xm_lds;                           // [N][16]
    float* red = zs + (size_t)N * 16;             // [16][16]
    float* stat = red + XM_RED;                   // mean[16], invstd[16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int h0 = blockIdx.x * 16;
    {   // z = f W1^T + b1 for this workgroup's 16 units: the waves take the row tiles of 16 clips in turn
        const int hc = min(h0 + i, Hd - 1);
        const float bias = b1[hc];
        for (int rt = wave; rt * 16 < N; rt += 4) {
            const int r = min(rt * 16 + i, N - 1);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int kb = 0; kb < D; kb += 16) {
                const int k = kb + 4 * q;
                acc = xm_mma16(xm_frag_rowk(f, D, r, k, D), xm_frag_rowk(W1, D, hc, k, D), acc);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int n = rt * 16 + 4 * q + reg;
                if (n < N) zs[n * 16 + i] = acc[reg] + bias;
            }
        }
    }
    __syncthreads();
    const int col = threadIdx.x & 15, grp = threadIdx.x >> 4, h = h0 + col, hv = min(h, Hd - 1);
    if (training) {                               // uniform over the grid
        float s = 0.f;
        for (int n = grp; n < N; n += 16) s += zs[n * 16 + col];
        red[grp * 16 + col] = s;
        __syncthreads();
        if (threadIdx.x < 16) stat[col] = xm_colsum16(red, col) / (float)N;
        __syncthreads();
        const float mu = stat[col];
        float v = 0.f;
        for (int n = grp; n < N; n += 16) {
            const float d = zs[n * 16 + col] - mu;
            v = fmaf(d, d, v);
        }
        red[grp * 16 + col] = v;
        __syncthreads();
        if (threadIdx.x < 16) {
            const float ss = xm_colsum16(red, col);
            const float is = 1.f / sqrtf(ss / (float)N + eps);
            stat[16 + col] = is;
            if (h < Hd) {
                mean[h] = mu;
                invstd[h] = is;
                rmean[h] = (1.f - momentum) * rmean[h] + momentum * mu;
                rvar[h] = (1.f - momentum) * rvar[h] + momentum * (ss / (float)(N - 1));
            }
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
    } else if (threadIdx.x < 16) {
        const float mu = rmean[hv], is = 1.f / sqrtf(rvar[hv] + eps);
        stat[col] = mu;
        stat[16 + col] = is;
        if (h < Hd) {
            mean[h] = mu;
            invstd[h] = is;
        }
    }
    __syncthreads();
    if (h < Hd) {
        const float mu = stat[col], is = stat[16 + col], ga = gamma[h], be = beta[h];
        for (int n = grp; n < N; n += 16) {
            const float xh = (zs[n * 16 + col] - mu) * is;
            xhat[(size_t)n * Hd + h] = xh;
            a1[(size_t)n * Hd + h] = fmaxf(fmaf(ga, xh, be), 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void xm_hidden_bwd_kernel(const float* __restrict__ da1, const float* __restrict__ a1, const float* __restrict__ xhat,
                                                             const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ f, int N, int D, int Hd, int training,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dW1,
                                                             float* __restrict__ db1, float* __restrict__ dz1) {
    extern __shared__ __attribute__((aligned(16))) float xm_lds[];
    float* zs = xm_lds;                           // [N][16]: dy, then dz1
    float* red = zs + (size_t)N * 16;             // two [16][16] tables
    float* stat = red + XM_RED;                   // dbeta[16], dgamma[16]
    const int h0 = blockIdx.x * 16;
    const int col = threadIdx.x & 15, grp = threadIdx.x >> 4, h = h0 + col, hv = min(h, Hd - 1);
    {   // dy = da1 through the ReLU mask of the saved forward; dbeta = sum dy, dgamma = sum dy xhat
        float sb = 0.f, sg = 0.f;
        for (int n = grp; n < N; n += 16) {
            const size_t o = (size_t)n * Hd + hv;
            const float dy = a1[o] > 0.f ? da1[o] : 0.f;
            zs[n * 16 + col] = dy;
            sb += dy;
            sg = fmaf(dy, xhat[o], sg);
        }
        red[grp * 16 + col] = sb;
        red[256 + grp * 16 + col] = sg;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const float sb = xm_colsum16(red, col), sg = xm_colsum16(red + 256, col);
        stat[col] = sb;
        stat[16 + col] = sg;
        if (h < Hd) {
            dbeta[h] = sb;
            dgamma[h] = sg;
        }
    }
    __syncthreads();
    {   // dz1, kept in LDS for the weight gradient below, and db1 = sum dz1
        const float sc = gamma[hv] * invstd[hv], mb = stat[col] / (float)N, mg = stat[16 + col] / (float)N;
        float s1 = 0.f;
        for (int n = grp; n < N; n += 16) {
            const size_t o = (size_t)n * Hd + hv;
            const float dy = zs[n * 16 + col];
            const float dz = training ? sc * (dy - mb - xhat[o] * mg) : sc * dy;
            zs[n * 16 + col] = dz;
            if (h < Hd) dz1[o] = dz;
            s1 += dz;
        }
        red[grp * 16 + col] = s1;
    }
    __syncthreads();
    if (threadIdx.x < 16 && h < Hd) db1[h] = xm_colsum16(red, col);
    // dW1[h0 + row][d] = sum_n dz1[n][row] f[n][d]: A from LDS, B with the clip as its leading dimension; a wave per column tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    for (int ct = wave; ct * 16 < D; ct += 4) {
        const int dc = min(ct * 16 + i, D - 1);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < N; kb += 16) {
            const int k = kb + 4 * q;
            f32x4 a;
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = k + j < N ? zs[(k + j) * 16 + i] : 0.f;
            acc = xm_mma16(a, xm_frag_colk(f, D, dc, k, N), acc);
        }
        const int d = ct * 16 + i;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = h0 + 4 * q + reg;
            if (row < Hd && d < D) dW1[(size_t)row * D + d] = acc[reg];
        }
    }
}

static int xm_hidden_dims(const char* fn, int N, int D, int Hd, int training) {
    XM_CHECK(N >= 1 && N <= XM_MAX_N, "%s: N = %d outside 1..%d", fn, N, XM_MAX_N);
    XM_CHECK(!training || N >= 2, "%s: training mode needs N >= 2 clips (batch statistics of one value per channel)", fn);
    XM_CHECK(D >= 4 && D % 4 == 0, "%s: D = %d is not a positive multiple of 4", fn, D);
    XM_CHECK(Hd >= 4 && Hd % 4 == 0, "%s: Hd = %d is not a positive multiple of 4", fn, Hd);
    return 0;
}

extern "C" int tamgcn_xm_hidden_fwd(const float* f, const float* W1, const float* b1, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, long long* num_batches_tracked,
                                    int N, int D, int Hd, int training, float momentum, float eps,
                                    float* a1, float* xhat, float* mean, float* invstd, void* stream) {
    if (xm_hidden_dims("tamgcn_xm_hidden_fwd", N, D, Hd, training)) return -1;
    XM_CHECK(momentum >= 0.f && momentum <= 1.f, "tamgcn_xm_hidden_fwd: momentum %g outside 0..1", (double)momentum);
    XM_CHECK(eps >= 0.f, "tamgcn_xm_hidden_fwd: eps %g is negative", (double)eps);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "f", f);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "W1", W1);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "b1", b1);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "gamma", gamma);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "beta", beta);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "running_mean", running_mean);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "running_var", running_var);
    XM_CHECK(!training || (num_batches_tracked != nullptr && (((uintptr_t)num_batches_tracked) & 7) == 0),
             "tamgcn_xm_hidden_fwd: num_batches_tracked is NULL or not 8-byte aligned (training mode)");
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "a1", a1);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "xhat", xhat);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "mean", mean);
    XM_CHECK_P16("tamgcn_xm_hidden_fwd", "invstd", invstd);
    tg_launch_lds<xm_hidden_fwd_kernel>(xm_hidden_lds(XM_MAX_N), dim3(ceil_div(Hd, 16)), dim3(256), xm_hidden_lds(N), (hipStream_t)stream, f, W1,
                                        b1, gamma, beta, running_mean, running_var, num_batches_tracked, N, D, Hd, training, momentum, eps, a1,
                                        xhat, mean, invstd);
    XM_LAUNCH_CHECK("tamgcn_xm_hidden_fwd");
    return 0;
}

extern "C" int tamgcn_xm_hidden_bwd(const float* da1, const float* a1, const float* xhat, const float* invstd, const float* gamma,
                                    const float* f, const float* W1, int N, int D, int Hd, int training,
                                    float* dgamma, float* dbeta, float* dW1, float* db1, float* dz1, float* df, void* stream) {
    if (xm_hidden_dims("tamgcn_xm_hidden_bwd", N, D, Hd, training)) return -1;
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "da1", da1);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "a1", a1);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "xhat", xhat);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "invstd", invstd);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "gamma", gamma);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "f", f);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "W1", W1);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "dgamma", dgamma);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "dbeta", dbeta);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "dW1", dW1);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "db1", db1);
    XM_CHECK_P16("tamgcn_xm_hidden_bwd", "dz1", dz1);
    XM_CHECK(xm_al16(df), "tamgcn_xm_hidden_bwd: df is not 16-byte aligned");
    tg_launch_lds<xm_hidden_bwd_kernel>(xm_hidden_lds(XM_MAX_N), dim3(ceil_div(Hd, 16)), dim3(256), xm_hidden_lds(N), (hipStream_t)stream, da1,
                                        a1, xhat, invstd, gamma, f, N, D, Hd, training, dgamma, dbeta, dW1, db1, dz1);
    XM_LAUNCH_CHECK("tamgcn_xm_hidden_bwd");
    if (df) {                                     // df = dz1 W1, a contraction over all hidden units: across the workgroups above
        const dim3 grid(ceil_div(D, 16), ceil_div(ceil_div(N, 16), 4));
        hipLaunchKernelGGL((xm_gemm_ksplit<false, false>), grid, dim3(256), 0, (hipStream_t)stream, dz1, W1, (const float*)nullptr, N, D, Hd, df);
        XM_LAUNCH_CHECK("tamgcn_xm_hidden_bwd (df)");
    }
    return 0;
}
