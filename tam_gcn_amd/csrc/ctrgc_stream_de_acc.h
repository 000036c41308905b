// The dE accumulation: dE_s[u][v] = sum_t dy[t][u] x3_s[t][v], workgroup = (n, c).
// A body FRAGMENT of ctrgc_stream_body.h (read that first): pasted by #include into the __global__ function that is this kernel.
// In scope there: the template argument ST, the policy type G and `const G g`, and (V a template or a kernel argument)
//     int N, Cout, T, V; const float* x3; const SrcDev dy; float* dE
    constexpr bool ONE = G::NUT == 1;         // a single joint tile: wave s owns subset s
    constexpr int P = G::VP + 16, NUT = G::NUT, UW = NUT < 4 ? NUT : 4, VWAVES = ONE ? 1 : 4 / UW, VPW = NUT / VWAVES;
    constexpr int NS = ONE ? 1 : ST;          // subsets a wave accumulates
    constexpr int BT = STREAM_BT, NPX = (ST * BT * G::VMAX / 4 + 255) / 256, NPY = (BT * G::VMAX / 4 + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Zs = smem;                         // [BT][P]      dy chunk (prologue applied)
    float* Xs = Zs + BT * P;                  // [ST][BT][P]
    const int n = blockIdx.x / Cout, c = blockIdx.x - n * Cout;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const bool active = !ONE || wave < ST;
    const int ut = ONE ? 0 : wave % UW, vb = ONE ? 0 : (wave / UW) * VPW, sb = ONE ? (wave < ST ? wave : 0) : 0;
    const int CH4 = BT * V / 4, VV = V * V;
    const long long TV = (long long)T * V;
    const int ch = dy.coff + c;
    const float c1 = dy.coef ? dy.coef[ch] : 1.f;
    const float c2 = (dy.coef && dy.x2) ? dy.coef[dy.ctot + ch] : 0.f;
    const float c0 = dy.coef ? dy.coef[2 * dy.ctot + ch] : 0.f;
    const long long dyb = ((long long)n * dy.ctot + ch) * TV;
    if constexpr (G::PADS) for (int e = tid; e < (ST + 1) * BT * P; e += 256) smem[e] = 0.f;   // joint pads stay zero

    float4 px[NPX], p1[NPY], p2[NPY];
    auto prefetch = [&](int t0) {
        const int valid = min(BT, T - t0) * V;
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            const int e = tid + i * 256, ec = g.idle0(e, ST * CH4), s = g.subset_of(ec, CH4), r = ec - s * CH4;
            const bool ok = e < ST * CH4 && g.in_clip(r * 4, valid, t0, T);
            px[i] = ok ? reinterpret_cast<const float4*>(x3 + (((long long)n * ST + s) * Cout + c) * TV + (long long)t0 * V)[r]
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NPY; ++i) {
            const int r = tid + i * 256;
            const bool ok = r < CH4 && g.in_clip(r * 4, valid, t0, T);
            p1[i] = ok ? reinterpret_cast<const float4*>(dy.x1 + dyb + (long long)t0 * V)[r] : make_float4(0.f, 0.f, 0.f, 0.f);
            p2[i] = (ok && dy.x2) ? reinterpret_cast<const float4*>(dy.x2 + dyb + (long long)t0 * V)[r] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    prefetch(0);
    f32x4 acc[NS][VPW];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int v = 0; v < VPW; ++v) acc[s][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < T; t0 += BT) {
        __syncthreads();
        const int valid = min(BT, T - t0) * V;
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            const int e = tid + i * 256, s = g.subset_of(e, CH4), r = e - s * CH4;
            if (e < ST * CH4) {
                float4 t = px[i];
                g.cut4(t, r * 4, valid);
                if constexpr (G::AL) { int tl, v; g.divV(r * 4, tl, v); *reinterpret_cast<float4*>(Xs + (s * BT + tl) * P + v) = t; }
                else g.scatter4(Xs + s * BT * P, P, r * 4, t);
            }
        }
#pragma unroll
        for (int i = 0; i < NPY; ++i) {
            const int r = tid + i * 256;
            if (r < CH4) {
#include "ctrgc_stream_prologue4.h"
                const float4 t = make_float4(o[0], o[1], o[2], o[3]);
                if constexpr (G::AL) { int tl, u; g.divV(r * 4, tl, u); *reinterpret_cast<float4*>(Zs + tl * P + u) = t; }
                else g.scatter4(Zs, P, r * 4, t);
            }
        }
        __syncthreads();
        if (t0 + BT < T) prefetch(t0 + BT);
        if (active) {
#pragma unroll
            for (int k4 = 0; k4 < BT / 4; ++k4) {
                const float av = Zs[(k4 * 4 + kq) * P + ut * 16 + j];          // A[i = u][k = t]
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VPW; ++v)
                        acc[s][v] = mfma16(av, Xs[((sb + s) * BT + k4 * 4 + kq) * P + (vb + v) * 16 + j], acc[s][v]);   // B[k = t][j = v]
            }
        }
    }
    if (active) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float* o = dE + (((long long)n * ST + sb + s) * Cout + c) * VV;
#pragma unroll
            for (int v = 0; v < VPW; ++v)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int uu = ut * 16 + kq * 4 + r, vv = (vb + v) * 16 + j;
                    if (G::FULL || (uu < V && vv < V)) o[uu * V + vv] = acc[s][v][r];
                }
        }
    }
