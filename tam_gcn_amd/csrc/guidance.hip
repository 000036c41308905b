// Skeleton guidance (include/tamgcn.h "guidance"; tam_gcn_amd/guidance.py; reference visual.py:53-87 and
// models/resnet_gcn_attention.py:82-85): what the reference does on the host between extract_feature and the plot, as three
// launches that read the block stack's output h (N*M, C, T', V) where it lies.  The permuted (N, C, T', V, M) copy is never made.
//
//   tamgcn_guidance_reduce   ONE read of h.  A workgroup owns 64 (t, v) columns of one row n*M + m: lane l of every wave owns column
//                            64*chunk + l, the four waves split the channels in four contiguous ranges.  A load is 64 consecutive
//                            floats of one channel; the lane keeps x*x summed in a register (the channel L2 norm of its column), and
//                            the 64 values of the channel meet in a fixed butterfly (the pooled feature's partial sum, one float per
//                            (workgroup, channel) in csum).  The four waves' sums of squares are added in wave order through LDS;
//                            the workgroup's smallest and largest intensity go to minmax.  A second small launch adds the csum
//                            partials of a clip in (m, chunk) order.  No atomics anywhere: two calls are bit-equal.
//   tamgcn_guidance_weights  one workgroup per clip: the call's global min / max from the partials (exact in any order), the person
//                            choice from fp64 sums taken in a fixed order, then one wave per target joint counts ranks inside the
//                            joint's T' values (index breaks ties, so exactly min(k, T') are taken) and averages the k largest.
//   tamgcn_guidance_apply    out = rgb * row factor, one wave per image row; the row factor is the 1-D bilinear interpolation of the
//                            225-row striped map, computed from the (N, J) weights (the map is never materialised).  16-byte lanes
//                            between a scalar head and tail where rgb and out share their alignment modulo 16, 4-byte lanes otherwise.
#include "common.h"
#include <math.h>

namespace {

constexpr int GR_COLS = 64;       // columns of a workgroup of the reduction: one per lane
constexpr int GR_WAVES = 4;       // its waves split the channels
constexpr int GW_TMAX = 1024;     // frames a joint's column may have (rank counting inside one wave, column in LDS)
constexpr int GW_WAVES = 4;
constexpr int GA_ROWS = 225;      // the reference's map: 225 rows in stripes of 45
constexpr int GA_STRIPE = 45;

__device__ __forceinline__ float wave_min64(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum64d(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(GR_WAVES * 64) void guidance_reduce_kernel(const float* __restrict__ h, int C, int P, int M, int nchunk,
                                                                        float* __restrict__ intensity, float* __restrict__ csum,
                                                                        float* __restrict__ minmax) {
    __shared__ float ss_part[GR_WAVES][GR_COLS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int chunk = blockIdx.x % nchunk, row = blockIdx.x / nchunk;
    const int p = chunk * GR_COLS + lane;
    const bool ok = p < P;
    const int Cq = (C + GR_WAVES - 1) / GR_WAVES;
    const int c0 = w * Cq, c1 = min(C, c0 + Cq);
    const float* src = h + (long long)row * C * P + (ok ? p : 0);
    float* cs = csum + (long long)blockIdx.x * C;
    float ss = 0.f;
    int c = c0;
    for (; c + 4 <= c1; c += 4) {                                            // four loads in flight per lane
        float x0 = src[(long long)c * P], x1 = src[(long long)(c + 1) * P], x2 = src[(long long)(c + 2) * P], x3 = src[(long long)(c + 3) * P];
        if (!ok) x0 = x1 = x2 = x3 = 0.f;
        ss = fmaf(x0, x0, ss); ss = fmaf(x1, x1, ss); ss = fmaf(x2, x2, ss); ss = fmaf(x3, x3, ss);
        const float s0 = wave_sum64(x0), s1 = wave_sum64(x1), s2 = wave_sum64(x2), s3 = wave_sum64(x3);
        if (lane == 0) { cs[c] = s0; cs[c + 1] = s1; cs[c + 2] = s2; cs[c + 3] = s3; }
    }
    for (; c < c1; ++c) {
        float x = src[(long long)c * P];
        if (!ok) x = 0.f;
        ss = fmaf(x, x, ss);
        const float s = wave_sum64(x);
        if (lane == 0) cs[c] = s;
    }
    ss_part[w][lane] = ss;
    __syncthreads();
    if (w == 0) {
        const float tot = ((ss_part[0][lane] + ss_part[1][lane]) + ss_part[2][lane]) + ss_part[3][lane];
        const float I = sqrtf(tot);
        if (ok) intensity[((long long)(row / M) * P + p) * M + row % M] = I;
        const float mn = wave_min64(ok ? I : INFINITY), mx = wave_max64(ok ? I : -INFINITY);
        if (lane == 0) { minmax[2 * blockIdx.x] = mn; minmax[2 * blockIdx.x + 1] = mx; }
    }
}

// pooled[n][c] = (sum over m, chunk -- in that order -- of csum[(n M + m) nchunk + chunk][c]) / (P M)
__global__ __launch_bounds__(256) void guidance_pool_kernel(const float* __restrict__ csum, int C, int parts_per_clip, float count,
                                                            float* __restrict__ pooled) {
    const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (c >= C) return;
    const float* p = csum + (long long)n * parts_per_clip * C + c;
    float s = 0.f;
    for (int i = 0; i < parts_per_clip; ++i) s += p[(long long)i * C];
    pooled[(long long)n * C + c] = s / count;
}

__global__ __launch_bounds__(GW_WAVES * 64) void guidance_weights_kernel(const float* __restrict__ intensity, const float* __restrict__ minmax,
                                                                         int nparts, int Tp, int V, int M, const int* __restrict__ joints,
                                                                         int J, int k, float* __restrict__ weights) {
    __shared__ float fred[2][GW_WAVES];
    __shared__ double dred[2][GW_WAVES];
    __shared__ float col[GW_WAVES][GW_TMAX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = blockIdx.x;
    const int P = Tp * V;
    // the whole call's extremes (the reference normalises over the batch it was given, visual.py:58-59)
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < nparts; i += GW_WAVES * 64) {
        mn = fminf(mn, minmax[2 * i]);
        mx = fmaxf(mx, minmax[2 * i + 1]);
    }
    mn = wave_min64(mn);
    mx = wave_max64(mx);
    if (lane == 0) { fred[0][w] = mn; fred[1][w] = mx; }
    __syncthreads();
    mn = fminf(fminf(fred[0][0], fred[0][1]), fminf(fred[0][2], fred[0][3]));
    mx = fmaxf(fmaxf(fred[1][0], fred[1][1]), fmaxf(fred[1][2], fred[1][3]));
    const float range = mx - mn;
    const bool norm = range != 0.f;                                          // max == min: the intensity stays as it is (:58)
    const float* In = intensity + (long long)n * P * M;
    // person 1 only if its mean is strictly larger (:71-74); both sums in one fixed order, so a bitwise copy ties
    int person = 0;
    if (M > 1) {
        double s0 = 0.0, s1 = 0.0;
        for (int p = tid; p < P; p += GW_WAVES * 64) {
            const float a = In[(long long)p * M], b = In[(long long)p * M + 1];
            s0 += (double)(norm ? 255.f * (a - mn) / range : a);
            s1 += (double)(norm ? 255.f * (b - mn) / range : b);
        }
        s0 = wave_sum64d(s0);
        s1 = wave_sum64d(s1);
        if (lane == 0) { dred[0][w] = s0; dred[1][w] = s1; }
        __syncthreads();
        s0 = ((dred[0][0] + dred[0][1]) + dred[0][2]) + dred[0][3];
        s1 = ((dred[1][0] + dred[1][1]) + dred[1][2]) + dred[1][3];
        person = s0 < s1 ? 1 : 0;
    }
    const int kk = min(k, Tp);
    for (int j0 = 0; j0 < J; j0 += GW_WAVES) {                               // the same trip count in every wave: barriers inside
        const int j = j0 + w;
        const int v = j < J ? joints[j] : -1;
        const bool live = v >= 0 && v < V;
        if (live)
            for (int t = lane; t < Tp; t += 64) {
                const float a = In[((long long)t * V + v) * M + person];
                col[w][t] = norm ? 255.f * (a - mn) / range : a;
            }
        __syncthreads();
        if (j < J) {
            double acc = 0.0;
            if (live)
                for (int t = lane; t < Tp; t += 64) {
                    const float x = col[w][t];
                    int rank = 0;                                            // values ahead of x: larger, or equal and earlier
                    for (int s = 0; s < Tp; ++s) {
                        const float y = col[w][s];
                        rank += (y > x || (y == x && s < t)) ? 1 : 0;
                    }
                    if (rank < kk) acc += (double)x;
                }
            acc = wave_sum64d(acc);
            if (lane == 0) weights[(long long)n * J + j] = live ? (float)(acc / (double)kk) / 127.f : 0.f;
        }
        __syncthreads();
    }
}

// row y of the resized map of clip n: bilinear, align_corners = False, over the 225 rows whose stripe j holds wn[j]
__device__ __forceinline__ float guidance_row_factor(const float* __restrict__ wn, int J, int F, int y, float scale) {
    const float src = fmaxf(scale * ((float)y + 0.5f) - 0.5f, 0.f);
    const int i0 = min((int)src, GA_ROWS - 1), i1 = min(i0 + 1, GA_ROWS - 1);
    const float l1 = src - (float)i0, l0 = 1.f - l1;
    const int ja = i0 / GA_STRIPE, jb = i1 / GA_STRIPE;
    const float a = (ja < J && ja < F) ? wn[ja] : 0.f, b = (jb < J && jb < F) ? wn[jb] : 0.f;
    return l0 * a + l1 * b;
}

__global__ __launch_bounds__(256) void guidance_apply_kernel(const float* __restrict__ weights, int J, int F, const float* __restrict__ rgb,
                                                             int Crgb, int H, int W, int rows_rgb, int rows_all, float scale, int same_align,
                                                             float* __restrict__ out, float* __restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), nwaves = gridDim.x * 4;
    for (int r = wave; r < rows_all; r += nwaves) {
        const bool is_map = r >= rows_rgb;
        const int rr = is_map ? r - rows_rgb : r;
        const int y = rr % H, n = is_map ? rr / H : rr / (H * Crgb);
        const float fac = guidance_row_factor(weights + (long long)n * J, J, F, y, scale);
        const float* s = is_map ? nullptr : rgb + (long long)rr * W;
        float* d = (is_map ? map : out) + (long long)rr * W;
        if (is_map || same_align) {
            const int head = min(W, (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2));
            const int nv = (W - head) >> 2, tail = head + 4 * nv;
            if (lane < head) d[lane] = s ? s[lane] * fac : fac;
            for (int i = lane; i < nv; i += 64) {
                f32x4 x = {1.f, 1.f, 1.f, 1.f};
                if (s) x = *reinterpret_cast<const f32x4*>(s + head + 4 * i);
                *reinterpret_cast<f32x4*>(d + head + 4 * i) = x * fac;
            }
            if (tail + lane < W) d[tail + lane] = s ? s[tail + lane] * fac : fac;
        } else {
            for (int i = lane; i < W; i += 64) d[i] = s[i] * fac;
        }
    }
}

}  // namespace

extern "C" int tamgcn_guidance_parts(int N, int M, int Tp, int V) {
    if (N < 1 || M < 1 || Tp < 1 || V < 1) return -1;
    const long long parts = (long long)N * M * (((long long)Tp * V + GR_COLS - 1) / GR_COLS);
    return parts < (1ll << 24) ? (int)parts : -1;
}

extern "C" int tamgcn_guidance_reduce(const float* h, int N, int M, int C, int Tp, int V, float* intensity, float* pooled, float* csum,
                                      float* minmax, void* stream) {
    const char* who = "tamgcn_guidance_reduce";
    TG_CHECK(h && intensity && pooled && csum && minmax, "%s: null pointer", who);
    TG_CHECK(N >= 1 && N <= 65535 && M >= 1 && C >= 1 && Tp >= 1 && V >= 2 && V <= 32, "%s: bad dims N=%d M=%d C=%d T'=%d V=%d (2 <= V <= 32)", who, N,
             M, C, Tp, V);
    TG_CHECK((long long)N * M * C * Tp * V < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    const int parts = tamgcn_guidance_parts(N, M, Tp, V);
    TG_CHECK(parts > 0 && (long long)parts * C < (1ll << 31), "%s: too many partial sums (N=%d M=%d C=%d T'=%d V=%d)", who, N, M, C, Tp, V);
    const int P = Tp * V, nchunk = (P + GR_COLS - 1) / GR_COLS;
    hipLaunchKernelGGL(guidance_reduce_kernel, dim3(parts), dim3(GR_WAVES * 64), 0, (hipStream_t)stream, h, C, P, M, nchunk, intensity, csum, minmax);
    tamgcn_note_kernel("guidance_reduce_kernel");
    TG_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(guidance_pool_kernel, dim3(ceil_div(C, 256), N), dim3(256), 0, (hipStream_t)stream, csum, C, M * nchunk,
                       (float)((long long)P * M), pooled);
    TG_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int tamgcn_guidance_weights(const float* intensity, const float* minmax, int nparts, int N, int Tp, int V, int M, const int* joints,
                                       int J, int k, float* weights, void* stream) {
    const char* who = "tamgcn_guidance_weights";
    TG_CHECK(intensity && minmax && joints && weights, "%s: null pointer", who);
    TG_CHECK(N >= 1 && Tp >= 1 && Tp <= GW_TMAX && V >= 2 && V <= 32 && M >= 1 && J >= 1 && J <= 4096 && k >= 1 && nparts >= 1,
             "%s: bad dims N=%d T'=%d (1..%d) V=%d (2..32) M=%d J=%d k=%d nparts=%d", who, N, Tp, GW_TMAX, V, M, J, k, nparts);
    TG_CHECK((long long)N * Tp * V * M < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    hipLaunchKernelGGL(guidance_weights_kernel, dim3(N), dim3(GW_WAVES * 64), 0, (hipStream_t)stream, intensity, minmax, nparts, Tp, V, M, joints, J, k,
                       weights);
    tamgcn_note_kernel("guidance_weights_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int tamgcn_guidance_apply(const float* weights, int N, int J, int frames, const float* rgb, int Crgb, int H, int W, float* out, float* map,
                                     void* stream) {
    const char* who = "tamgcn_guidance_apply";
    TG_CHECK(weights && (out || map), "%s: null pointer", who);
    TG_CHECK((rgb != nullptr) == (out != nullptr), "%s: rgb and out go together", who);
    TG_CHECK(N >= 1 && J >= 1 && frames >= 0 && H >= 1 && W >= 1 && (!out || Crgb >= 1), "%s: bad dims N=%d J=%d frames=%d Crgb=%d H=%d W=%d", who, N, J,
             frames, Crgb, H, W);
    TG_CHECK(((uintptr_t)rgb & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)map & 3) == 0, "%s: a pointer is not 4-byte aligned", who);
    const long long rows_rgb = out ? (long long)N * Crgb * H : 0, rows_all = rows_rgb + (map ? (long long)N * H : 0);
    TG_CHECK(rows_all < (1ll << 31), "%s: 2^31 image rows or more", who);
    const int same_align = (((uintptr_t)rgb ^ (uintptr_t)out) & 15) == 0;
    const int grid = (int)((rows_all + 3) / 4 < 2048 ? (rows_all + 3) / 4 : 2048);
    hipLaunchKernelGGL(guidance_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, weights, J, frames, rgb, Crgb, H, W, (int)rows_rgb,
                       (int)rows_all, (float)GA_ROWS / (float)H, same_align, out, map);
    tamgcn_note_kernel("guidance_apply_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}
