// The streaming kernels of the cross-modal head: the gated average pool over the image map and its backward.  f_attended, the
// gated copy of the (N, R, H, W) map the reference writes and reads again, never exists: g = att * mean_p f_rgb.
#include "xm_common.h"

// m[row] = mean_p f_rgb[row][p], g = att * m; rows = N * R.  Sixteen lanes share a row: lane j adds elements j, j + 16, ... in
// that order and the sixteen partial sums meet in a fixed butterfly, so the bits depend on P alone -- not on where f_rgb
// starts, which may be any dword (rows of 49 floats are dword aligned whatever the base).  A wave reads four neighbouring rows,
// one contiguous span; no load is wider than the element it uses, so nothing past the last element of f_rgb is touched.
__global__ __launch_bounds__(256) void xm_pool_fwd_kernel(const float* __restrict__ f_rgb, const float* __restrict__ att, int rows, int P,
                                                           float* __restrict__ m, float* __restrict__ g) {
    const int row = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    const bool live = row < rows;
    float s = 0.f;
    if (live) {
        const float* p = f_rgb + (size_t)row * P;
        for (int e = j; e < P; e += 16) s += p[e];
    }
    s = wave_sum16(s);
    if (live && j == 0) {
        const float mv = s / (float)P;
        m[row] = mv;
        g[row] = att[row] * mv;
    }
}

// dz2 = dg * m * att * (1 - att) over the N * R rows, and the broadcast df_rgb[row][p] = dg[row] * att[row] / P over the flat
// map: thread t stores the t-th 16-byte aligned piece of df_rgb, `lead` elements in (the base is dword aligned only); the
// pieces before the first and after the last aligned one are stored element by element by the threads that follow.
__global__ __launch_bounds__(256) void xm_pool_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ m, const float* __restrict__ att,
                                                           int rows, int P, float* __restrict__ dz2, float* __restrict__ df_rgb, int lead,
                                                           int nvec, int total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < rows) {
        const float a = att[t];
        dz2[t] = dg[t] * m[t] * a * (1.f - a);
    }
    if (df_rgb == nullptr) return;
    const float fp = (float)P;
    if (t < nvec) {
        const int e = lead + 4 * t;
        int row = e / P, rem = e - row * P;
        float v = dg[row] * att[row] / fp;
        f32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            o[c] = v;
            if (++rem == P && c < 3) {                 // the next element opens the next row (row + 1 < rows: e + c + 1 < total)
                rem = 0;
                ++row;
                v = dg[row] * att[row] / fp;
            }
        }
        *reinterpret_cast<f32x4*>(df_rgb + e) = o;
    } else {
        const int u = t - nvec;                        // 0 .. lead - 1: the head;  then the tail after the last aligned piece
        const int e = u < lead ? u : 4 * nvec + u;
        if (e < total) {
            const int row = e / P;
            df_rgb[e] = dg[row] * att[row] / fp;
        }
    }
}

static int xm_pool_dims(const char* fn, int N, int R, int P) {
    XM_CHECK(N >= 1 && N <= XM_MAX_N, "%s: N = %d outside 1..%d", fn, N, XM_MAX_N);
    XM_CHECK(R >= 4 && R % 4 == 0, "%s: R = %d is not a positive multiple of 4", fn, R);
    XM_CHECK(P >= 1, "%s: P = %d, at least one position is needed", fn, P);
    XM_CHECK((long long)N * R * P < (1ll << 31), "%s: N * R * P = %lld, the map must have fewer than 2^31 elements", fn, (long long)N * R * P);
    return 0;
}

extern "C" int tamgcn_xm_pool_fwd(const float* f_rgb, const float* att, int N, int R, int P, float* m, float* g, void* stream) {
    if (xm_pool_dims("tamgcn_xm_pool_fwd", N, R, P)) return -1;
    XM_CHECK(f_rgb != nullptr && xm_al4(f_rgb), "tamgcn_xm_pool_fwd: f_rgb is NULL or not 4-byte aligned");
    XM_CHECK_P16("tamgcn_xm_pool_fwd", "att", att);
    XM_CHECK_P16("tamgcn_xm_pool_fwd", "m", m);
    XM_CHECK_P16("tamgcn_xm_pool_fwd", "g", g);
    const int rows = N * R;
    hipLaunchKernelGGL(xm_pool_fwd_kernel, dim3(ceil_div(rows, 16)), dim3(256), 0, (hipStream_t)stream, f_rgb, att, rows, P, m, g);
    XM_LAUNCH_CHECK("tamgcn_xm_pool_fwd");
    return 0;
}

extern "C" int tamgcn_xm_pool_bwd(const float* dg, const float* m, const float* att, int N, int R, int P, float* dz2, float* df_rgb,
                                  void* stream) {
    if (xm_pool_dims("tamgcn_xm_pool_bwd", N, R, P)) return -1;
    XM_CHECK_P16("tamgcn_xm_pool_bwd", "dg", dg);
    XM_CHECK_P16("tamgcn_xm_pool_bwd", "m", m);
    XM_CHECK_P16("tamgcn_xm_pool_bwd", "att", att);
    XM_CHECK_P16("tamgcn_xm_pool_bwd", "dz2", dz2);
    XM_CHECK(xm_al4(df_rgb), "tamgcn_xm_pool_bwd: df_rgb is not 4-byte aligned");
    const int rows = N * R, total = rows * P;
    int lead = 0, nvec = 0, work = rows;
    if (df_rgb) {
        lead = (int)((4 - ((((uintptr_t)df_rgb) >> 2) & 3)) & 3);
        if (lead > total) lead = total;
        nvec = (total - lead) / 4;
        const int ends = total - 4 * nvec;              // head and tail elements, at most 6
        if (nvec + ends > work) work = nvec + ends;
    }
    hipLaunchKernelGGL(xm_pool_bwd_kernel, dim3(ceil_div(work, 256)), dim3(256), 0, (hipStream_t)stream, dg, m, att, rows, P, dz2, df_rgb,
                       lead, nvec, total);
    XM_LAUNCH_CHECK("tamgcn_xm_pool_bwd");
    return 0;
}
