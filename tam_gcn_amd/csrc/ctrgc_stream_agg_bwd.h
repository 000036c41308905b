// The aggregation backward w.r.t. x3: dx3_s[t][v] = sum_u dy[t][u] E_s[u][v].
// A body FRAGMENT of ctrgc_stream_body.h (read that first): pasted by #include into the __global__ function that is this kernel.
// In scope there: the template argument ST, the policy type G and `const G g`, and (V a template or a kernel argument)
//     int N, Cout, T, V; const SrcDev dy; const float* E; float* dx3, * db3_part
    constexpr int PE = G::PE, BT = STREAM_BT, NPF = (BT * G::VMAX / 4 + 255) / 256;
    constexpr int JW = G::NUT >= 2 ? G::NUT / 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[ST][4];
    float* Es = smem;                         // [ST][v][PE] (transposed)
    float* Zs = Es + ST * G::VP * PE;            // [BT][PE]
    const int n = blockIdx.x / Cout, c = blockIdx.x - n * Cout;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const bool active = G::NUT >= 2 || wave < 2;
    const int tt = G::NUT >= 2 ? wave >> 1 : wave & 1, vb = G::NUT >= 2 ? (wave & 1) * JW : 0;
    const int CH4 = BT * V / 4;
    const long long TV = (long long)T * V;
    if constexpr (G::PADS && !G::FILL_WITH_E) for (int e = tid; e < BT * PE; e += 256) Zs[e] = 0.f;
    g.template stage_E<ST, true>(E, Cout, n, c, Es, BT * PE);
    const int ch = dy.coff + c;
    const float c1 = dy.coef ? dy.coef[ch] : 1.f;
    const float c2 = (dy.coef && dy.x2) ? dy.coef[dy.ctot + ch] : 0.f;
    const float c0 = dy.coef ? dy.coef[2 * dy.ctot + ch] : 0.f;
    const long long dyb = ((long long)n * dy.ctot + ch) * TV;

    float4 p1[NPF], p2[NPF];
    auto prefetch = [&](int t0) {
        const int valid = min(BT, T - t0) * V;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int r = tid + i * 256;
            const bool ok = r < CH4 && g.in_clip(r * 4, valid, t0, T);
            p1[i] = ok ? reinterpret_cast<const float4*>(dy.x1 + dyb + (long long)t0 * V)[r] : make_float4(0.f, 0.f, 0.f, 0.f);
            p2[i] = (ok && dy.x2) ? reinterpret_cast<const float4*>(dy.x2 + dyb + (long long)t0 * V)[r] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    prefetch(0);
    float sb[ST];
#pragma unroll
    for (int s = 0; s < ST; ++s) sb[s] = 0.f;
    for (int t0 = 0; t0 < T; t0 += BT) {
        __syncthreads();
        const int valid = min(BT, T - t0) * V;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int r = tid + i * 256;
            if (r < CH4) {
#include "ctrgc_stream_prologue4.h"
                g.scatter4(Zs, PE, r * 4, make_float4(o[0], o[1], o[2], o[3]));
            }
        }
        __syncthreads();
        if (t0 + BT < T) prefetch(t0 + BT);
        if (active) {
            f32x4 acc[ST][JW];
#pragma unroll
            for (int s = 0; s < ST; ++s)
#pragma unroll
                for (int v = 0; v < JW; ++v) acc[s][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* ar = Zs + (tt * 16 + j) * PE + kq;
#pragma unroll
            for (int k4 = 0; k4 < g.k4(); ++k4) {
                const float av = ar[k4 * 4];
#pragma unroll
                for (int s = 0; s < ST; ++s)
#pragma unroll
                    for (int v = 0; v < JW; ++v) acc[s][v] = mfma16(av, Es[(s * G::VP + (vb + v) * 16 + j) * PE + k4 * 4 + kq], acc[s][v]);
            }
#pragma unroll
            for (int s = 0; s < ST; ++s) {
                float* orow = dx3 + (((long long)n * ST + s) * Cout + c) * TV;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = t0 + tt * 16 + kq * 4 + r;
                    if (t < T) {
#pragma unroll
                        for (int v = 0; v < JW; ++v) {
                            const int vv = (vb + v) * 16 + j;
                            if (G::FULL || vv < V) {
                                orow[(long long)t * V + vv] = acc[s][v][r];
                                sb[s] += acc[s][v][r];
                            }
                        }
                    }
                }
            }
        }
    }
    if (db3_part) {
#pragma unroll
        for (int s = 0; s < ST; ++s) {
            const float t = wave_sum64(sb[s]);
            if (lane == 0) red[s][wave] = t;
        }
        __syncthreads();
        if (tid < ST) db3_part[(long long)n * ST * Cout + tid * Cout + c] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    }
