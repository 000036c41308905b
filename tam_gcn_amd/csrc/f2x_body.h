// The four stage bodies of the small-batch eval families whose frames are padded to VP = (V + 3) & ~3 floats: f2v.hip (the
// joint count a template parameter) and f2g.hip (a kernel argument).  One text, written against a GEOMETRY POLICY `Geo`:
//
//   constexpr in both   VP QF NC NCT PB PH (what the frame pitch fixes), NIT NB (register-array sizes of the e stage),
//                       STATIC_V
//   geo.V geo.EC geo.ECT geo.PD geo.EPC geo.ES geo.KC
//                       static constexpr members of f2v's FvGeo<V> -- every use folds to a constant and the kernels are the
//                       ones a body written for that V alone would give -- and data members of f2g's FgGeo<VP>, computed from
//                       the kernel's arguments.
//   Args                the family's kernel-argument struct: f2_common.h's for f2v, f2g's own (the same fields and V, kc, in the
//                       order its kernels were compiled with: moving a field moves the scalar loads and, with them, the
//                       schedule -- profiles/f2_family_merge_resources.txt).
//
// The layout, in the numbers of V = 25, VP = 28 (at 17 and 18 VP = 20, a frame is five 16-byte pieces, a tile 80 columns):
//
//   alignment   a (n, c) row of T*25 floats starts on a 16-byte boundary only by accident (300 -> 150 -> 75 frames).  Only the
//               block's input and output keep that contiguous (N, C, T, V) form.  Everything the family allocates for itself
//               (E, the four workspaces, the frame sums) has frames of VP = 28 floats: every row and every frame is 16-byte
//               aligned, and the staging of those is f2's float4 copy with 20 -> 28.  The block input is read in 16-byte
//               pieces from dword-aligned addresses (full rate on gfx950, tools/probes/unaligned_probe.hip), seven per frame; the
//               seventh reaches 12 bytes past the frame -- into the next one or, at the very end, into the allocator's slack --
//               and those three lanes are REPLACED by zeros (a select, never a product) before anything consumes them.
//   tile count  four frames at pitch 28 are 112 columns = exactly 7 MFMA tiles (6.25 at pitch 25).  The 12 pad columns of a tile
//               hold zeros (or, in the workspaces, finite values that only ever meet other pad columns: every product here keeps
//               columns apart, the aggregation over joints and the stores to the block output stop at v < V).
//   LDS         f2's tiling needs 204 KB (gcn, Cin = 256) and 189 KB (tcn, l8).  Here the gcn stage holds K in chunks of
//               geo.KC rows (153 KB with the three E runs of 22 KB) and the tcn stage runs the convolutional residual and the
//               temporal taps one after the other through ONE region (152 KB at Cin = 256).  The host computes every request
//               and refuses above F2_LDS_MAX.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 (exact fp32), the K blocks of a product dealt round-robin to the waves, the partial tiles
// summed through LDS in a fixed order, no atomics: two runs are bit-equal, and so are the two families on one problem.
#pragma once
#include "f2_common.h"

namespace {

// Rows [0, rows) of an LDS tile [rows][PB] <- rows [0, K) of an activation, frames tl*fstep (tl < bt); everything else zero.
// PADDED: the source has frames of VP floats (the family's own buffers: aligned pieces, pad columns copied as they are).
// Otherwise frames of V floats from a dword-aligned address: the last piece of a frame keeps its first V - (VP - 4) lanes
// (1..3 of them where V % 4 != 0; all four where f2g runs a multiple of four).
template <bool PADDED, class Geo>
__device__ __forceinline__ void f2x_stage(const Geo geo, float* Bs, const float* src, long long rs, int K, int rows, int bt, int fstep, int tid) {
    constexpr int U = 8, QF = Geo::QF, QT = F2_BT * QF;
    const int FP = PADDED ? Geo::VP : geo.V, last = geo.V - (Geo::VP - 4);
    for (int e0 = tid; e0 < rows * QT; e0 += U * F2_NT) {
        float4 t[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int e = e0 + i * F2_NT;
            const int k = e / QT, r = e - k * QT;
            const int tl = r / QF, q = r - tl * QF;
            t[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < rows * QT && k < K && tl < bt) {
                t[i] = *reinterpret_cast<const float4*>(src + k * rs + (long long)tl * fstep * FP + 4 * q);
                if (!PADDED && q == QF - 1) {                      // lanes past the frame: the next frame or the slack behind the tensor
                    if (last < 2) t[i].y = 0.f;
                    if (last < 3) t[i].z = 0.f;
                    if (last < 4) t[i].w = 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int e = e0 + i * F2_NT;
            const int k = e / QT, r = e - k * QT;
            if (e < rows * QT) *reinterpret_cast<float4*>(Bs + k * Geo::PB + 4 * r) = t[i];
        }
    }
}

// ---- E for 16 channels of one (sample, subset): E[c][u][v] at [c][u * VP + v], pad columns zero
template <class Geo, class Args>
__device__ __forceinline__ void f2x_e_body(const Geo geo, const Args& a) {
    constexpr int NT = F2_NT, PX = F2_PX, VP = Geo::VP, QF = Geo::QF, NB = Geo::NB, NIT = Geo::NIT;
    const int V = geo.V, EC = geo.EC, ECT = geo.ECT, PD = geo.PD;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.Cin + 15) & ~15, R2 = 2 * a.R, R2p = R2 < 16 ? 16 : R2, Rp = (a.R + 15) & ~15;
    float* XB = smem;                    // [Kp][PX]   xbar, columns >= V zero
    float* PQ = XB + Kp * PX;            // [R2p][PX]  p rows 0..R-1, q rows R..2R-1
    float* Pp = PQ + R2p * PX;           // [64][PX]   partial pq tiles
    float* Ds = Pp + 64 * PX;            // [Rp][PD]   D; before that: [ntp][Kp][VP] partial frame sums
    const int nct = a.Cout / 16;
    const int s = blockIdx.x / nct, c0 = (blockIdx.x - s * nct) * 16, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V;
    const int NTP = a.ntp;
    // pq product: (row tiles x K parts) over the waves; the row tiles round UP, a wave past the K parts multiplies zeros (f2.hip)
    const int nrt = (R2p + 15) / 16, nparts = 4 / nrt;
    const int prt = wave % nrt, ppart = wave / nrt;
    const float* a12 = ppart < nparts && prt * 16 + j < R2 ? a.w12 + ((long long)s * R2 + prt * 16 + j) * a.Cin : nullptr;
    float b12r[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) b12r[i] = tid + i * NT < R2 * V ? a.b12[s * R2 + (tid + i * NT) / V] : 0.f;
    const float alpha = a.alpha[0];
    float aw[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, b4r[4], Avr[NIT];
    {
        const float* arow = a.w4 + ((long long)s * a.Cout + c0 + j) * a.R;
        f2_load_a(arow, a.R, 0, kq, a.vec4 != 0, aw[0]);
        if (a.R > 16) f2_load_a(arow, a.R, 16, kq, a.vec4 != 0, aw[1]);
#pragma unroll
        for (int r = 0; r < 4; ++r) b4r[r] = a.b4[s * a.Cout + c0 + kq * 4 + r];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int col = (wave + 4 * i) * 16 + j, u = col / VP, v = col - u * VP;
            Avr[i] = (col < EC && v < V) ? a.A[s * V * V + u * V + v] : 0.f;
        }
    }
    // 1. xbar: from the producer's per-tile frame sums ([N][tiles][Cin][VP]) when it left them, else from x.  Fixed order.
    {
        float* XP = Ds;
        const float inv = 1.f / (float)a.T;
        if (a.xpart) {
            const int ntt = (a.T + F2_BT - 1) / F2_BT, tpg = (ntt + NTP - 1) / NTP;
            const float* xp = a.xpart + (long long)n * ntt * a.Cin * VP;
            const int cnt = NTP * a.Cin * QF;
            for (int e0 = tid; e0 < cnt; e0 += 8 * NT) {
                float4 acc[8];
                int off[8], g8[8];
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int e = e0 + p * NT;
                    const int g = e / (a.Cin * QF), rem = e - g * a.Cin * QF;
                    const int ci = rem / QF, v4 = (rem - ci * QF) * 4;
                    acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                    off[p] = ci * VP + v4;
                    g8[p] = e < cnt ? g : NTP;                      // NTP * tpg >= ntt: an out-of-range pair never loads
                }
                for (int i = 0; i < tpg; ++i) {
                    float4 q[8];
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        const int tile = g8[p] * tpg + i;
                        q[p] = tile < ntt ? *reinterpret_cast<const float4*>(xp + (long long)tile * a.Cin * VP + off[p]) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int p = 0; p < 8; ++p) { acc[p].x += q[p].x; acc[p].y += q[p].y; acc[p].z += q[p].z; acc[p].w += q[p].w; }
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int e = e0 + p * NT;
                    if (e < cnt) *reinterpret_cast<float4*>(XP + (g8[p] * Kp) * VP + off[p]) = acc[p];
                }
            }
        } else {                                                   // rows of V floats: element loads, the frame phases, frame order
            const float* xb = a.x + (long long)n * a.Cin * TV;
            for (int e = tid; e < NTP * a.Cin * VP; e += NT) {
                const int tp = e / (a.Cin * VP), rem = e - tp * a.Cin * VP;
                const int ci = rem / VP, v = rem - ci * VP;
                float acc = 0.f;
                if (v < V) {
                    const float* p = xb + ci * TV + v;
                    for (int t = tp; t < a.T; t += 8 * NTP) {
                        float q[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) q[i] = t + i * NTP < a.T ? p[(long long)(t + i * NTP) * V] : 0.f;
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc += q[i];
                    }
                }
                XP[(tp * Kp + ci) * VP + v] = acc;
            }
        }
        __syncthreads();
        for (int e = tid; e < Kp * (PX / 4); e += NT) {
            const int ci = e / (PX / 4), v4 = (e - ci * (PX / 4)) * 4;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ci < a.Cin && v4 < V) {
                for (int tp = 0; tp < NTP; ++tp) {
                    const float4 q = *reinterpret_cast<const float4*>(XP + (tp * Kp + ci) * VP + v4);
                    o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
                }
                o.x *= inv; o.y *= inv; o.z *= inv; o.w *= inv;
                if (v4 + 1 >= V) o.y = 0.f;                        // pad joints of a caller's xpart are not trusted
                if (v4 + 2 >= V) o.z = 0.f;
                if (v4 + 3 >= V) o.w = 0.f;
            }
            *reinterpret_cast<float4*>(XB + ci * PX + v4) = o;
        }
        __syncthreads();
    }
    // 2. p, q = W12_s xbar + b12_s: (2R x Cin) x (Cin x V)
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        f2_gemm16<2>(acc, a12, a.Cin, a.vec12 != 0, ppart, Kp >> 4, nparts, kq, [&](int k, int ct) { return XB[k * PX + ct * 16 + j]; });
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Pp[((ppart * nrt + prt) * 16 + kq * 4 + r) * PX + ct * 16 + j] = acc[ct][r];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + i * NT;
            if (e < R2 * V) {
                const int row2 = e / V, v = e - row2 * V;
                const int rt2 = row2 >> 4, rr = row2 & 15;
                float t = b12r[i];
                for (int p = 0; p < nparts; ++p) t += Pp[((p * nrt + rt2) * 16 + rr) * PX + v];
                PQ[row2 * PX + v] = t;
            }
        }
        __syncthreads();
    }
    // 3. D[r][u*VP + v] = tanh(p[r][u] - q[r][v]); rows R..Rp, pad joints and the columns up to the last tile's end zero
    for (int e = tid; e < Rp * ECT * 16; e += NT) {
        const int r = e / (ECT * 16), uv = e - r * (ECT * 16);
        const int u = uv / VP, v = uv - u * VP;
        Ds[r * PD + uv] = (r < a.R && u < V && v < V) ? fast_tanh(PQ[r * PX + u] - PQ[(a.R + r) * PX + v]) : 0.f;
    }
    __syncthreads();
    // 4. E tile = alpha (W4 D + b4) + A: 16 channels x EC, column tiles over the four waves, K = R <= 32
    {
        float* Eg = a.E + (((long long)n * a.S + s) * a.Cout + c0) * EC;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int ct = wave + 4 * it;
            if (ct < ECT) {                                        // wave-uniform
                const int col = ct * 16 + j;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) acc = mfma16(aw[0][i], Ds[(4 * kq + i) * PD + col], acc);
                if (a.R > 16) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = mfma16(aw[1][i], Ds[(16 + 4 * kq + i) * PD + col], acc);
                }
                const bool real = col - (col / VP) * VP < V;
                if (col < EC) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Eg[(long long)(kq * 4 + r) * EC + col] = real ? alpha * (acc[r] + b4r[r]) + Avr[it] : 0.f;
                }
            }
        }
    }
}

// ---- x3 GEMM + aggregation + BatchNorm + residual for 8 channels x 4 frames; K staged in chunks of geo.KC rows
template <class Geo, class Args>
__device__ __forceinline__ void f2x_gcn_body(const Geo geo, const Args& a) {
    constexpr int PB = Geo::PB, CT = F2_CT, VP = Geo::VP, NCT = Geo::NCT;
    const int V = geo.V, EC = geo.EC, ES = geo.ES, EPC = geo.EPC, KC = geo.KC;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.Cin + 15) & ~15, Kc = Kp < KC ? Kp : KC;
    float* Xs = smem;                    // [Kc][PB]      one K chunk of the x tile
    float* X3 = Xs + Kc * PB;            // [2][32][PB]   partial products: rows s*8 + c (s < 3), 24 + c = down(x)
    float* Es = X3 + 2 * 32 * PB;        // [3][ES]       E_s[c][u][VP]
    const int nct = a.Cout / CT;
    const int ctile = blockIdx.x % nct, tt = blockIdx.x / nct, n = blockIdx.y;
    const int c0 = ctile * CT, t0 = tt * F2_BT, bt = min(F2_BT, a.T - t0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V, TVP = (long long)a.T * VP;
    // E runs travel by LDS-DMA under the staging and the GEMM (the barriers below drain them)
    for (int p = wave; p < 3 * EPC; p += 4) {
        const int s = p / EPC, q = p - s * EPC;
        int f = q * 256 + lane * 4;
        if (f > CT * EC - 4) f = CT * EC - 4;                     // lanes past the run re-read its last slot into the padding
        const float* g = a.E + (((long long)n * a.S + s) * a.Cout + c0) * EC + f;
        __builtin_amdgcn_global_load_lds((tg_gptr)g, (tg_lptr)(Es + s * ES + q * 256), 16, 0, 0);
    }
    const int rt = wave & 1, kh = wave >> 1;
    const float* arow;
    bool vec;
    {
        const int row = rt * 16 + j, sidx = row >> 3, c = row & 7;
        arow = sidx < 3 ? a.w3 + ((long long)sidx * a.Cout + c0 + c) * a.Cin
                        : (a.res_mode == 2 ? a.wd + (long long)(c0 + c) * a.Cin : nullptr);
        vec = sidx < 3 ? a.vec3 != 0 : a.vecd != 0;
    }
    {
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Kp; k0 += KC) {
            const int rows = min(KC, Kp - k0);
            if (k0) __syncthreads();                               // the previous chunk has been consumed
            f2x_stage<false>(geo, Xs, a.x + ((long long)n * a.Cin + k0) * TV + (long long)t0 * V, TV, a.Cin - k0, rows, bt, 1, tid);
            __syncthreads();
            f2_gemm16<NCT>(acc, arow, a.Cin, vec, (k0 >> 4) + kh, (k0 + rows) >> 4, 2, kq,
                           [&](int k, int ct) { return Xs[(k - k0) * PB + ct * 16 + j]; });
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) X3[((kh * 32) + rt * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
    }
    __syncthreads();
    // aggregation: thread = (channel c, frame t, joint group ug): u = ug, ug + 8, ...
    {
        const int c = tid >> 5, t = (tid >> 3) & 3, ug = tid & 7;
        float x3v[3 * VP];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const float b = a.b3[s * a.Cout + c0 + c];
#pragma unroll
            for (int v4 = 0; v4 < VP; v4 += 4) {
                const f32x4 p0 = *reinterpret_cast<const f32x4*>(X3 + (s * 8 + c) * PB + t * VP + v4);
                const f32x4 p1 = *reinterpret_cast<const f32x4*>(X3 + (32 + s * 8 + c) * PB + t * VP + v4);
#pragma unroll
                for (int i = 0; i < 4; ++i) x3v[s * VP + v4 + i] = p0[i] + p1[i] + b;
            }
        }
        const float sy = a.sy[c0 + c], ty = a.ty[c0 + c];
        const float bd = a.res_mode == 2 ? a.bd[c0 + c] : 0.f;
        if (t < bt) {
            const long long o0 = ((long long)n * a.Cout + c0 + c) * TVP + (long long)(t0 + t) * VP;
            for (int u = ug; u < V; u += 8) {
                float z = 0.f;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const float* er = Es + s * ES + c * EC + u * VP;
#pragma unroll
                    for (int v4 = 0; v4 < VP; v4 += 4) {
                        f32x4 e = *reinterpret_cast<const f32x4*>(er + v4);
                        // the pad joints take no part (E's pad columns are not trusted): left out at compile time, or
                        // replaced by zeros -- a select -- in the last piece.  An FMA with a zero leaves z as it is.
                        if constexpr (Geo::STATIC_V) {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (v4 + i < V) z = fmaf(e[i], x3v[s * VP + v4 + i], z);
                        } else {
                            if (v4 == VP - 4) {
                                if (VP - 3 >= V) e[1] = 0.f;
                                if (VP - 2 >= V) e[2] = 0.f;
                                if (VP - 1 >= V) e[3] = 0.f;
                            }
#pragma unroll
                            for (int i = 0; i < 4; ++i) z = fmaf(e[i], x3v[s * VP + v4 + i], z);
                        }
                    }
                }
                const float y = fmaf(sy, z, ty);
                float res = 0.f;
                const int col = t * VP + u;
                if (a.res_mode == 1) res = a.x[((long long)n * a.Cin + c0 + c) * TV + (long long)(t0 + t) * V + u];
                else if (a.res_mode == 2) res = X3[(24 + c) * PB + col] + X3[(32 + 24 + c) * PB + col] + bd;
                a.sum[o0 + u] = y + res;
                a.diff[o0 + u] = res - y;
            }
            if (ug < VP - V) {                                     // pad joints of the workspaces: zeros
                a.sum[o0 + V + ug] = 0.f;
                a.diff[o0 + V + ug] = 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 16 rows x 4 frames of a pointwise product with the block's epilogues; x, add and out have frames of VP floats (V itself
// does not enter: the pad columns are computed along)
// ---------------------------------------------------------------------------------------------------------------------
template <class Geo, class Args>
__device__ __forceinline__ void f2x_gemm_body(const Geo geo, const Args& a) {
    constexpr int NT = F2_NT, PB = Geo::PB, NCT = Geo::NCT, VP = Geo::VP, QT = F2_BT * Geo::QF;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.K + 15) & ~15;
    float* Bs = smem;                    // [Kp][PB]
    float* Pp = Bs + Kp * PB;            // [4][16][PB]
    const int nmt = a.M / 16;
    const int mtile = blockIdx.x % nmt, tt = blockIdx.x / nmt, n = blockIdx.y;
    const int m0 = mtile * 16, t0 = tt * F2_BT, bt = min(F2_BT, a.T - t0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TVP = (long long)a.T * VP;
    const float* arow = a.w + (long long)(m0 + j) * a.K;
    f2x_stage<true>(geo, Bs, a.x + (long long)n * a.K * TVP + (long long)t0 * VP, TVP, a.K, Kp, bt, 1, tid);
    __syncthreads();
    {
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f2_gemm16<NCT>(acc, arow, a.K, a.vec != 0, wave, Kp >> 4, 4, kq, [&](int k, int ct) { return Bs[k * PB + ct * 16 + j]; });
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Pp[(wave * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
    }
    __syncthreads();
    for (int e = tid; e < 16 * QT; e += NT) {
        const int row = e / QT, c4 = (e - row * QT) * 4;
        if (c4 >= bt * VP) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(Pp + row * PB + c4);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(Pp + (w * 16 + row) * PB + c4);
            v += p;
        }
        const float b = a.b[m0 + row];
        const long long o = ((long long)n * a.M + m0 + row) * TVP + (long long)t0 * VP + c4;
        float4 r;
        if (a.mode == 0) {
            const float4 ad = *reinterpret_cast<const float4*>(a.add + o);
            r.x = fmaxf(ad.x + fast_tanh(v[0] + b), 0.f); r.y = fmaxf(ad.y + fast_tanh(v[1] + b), 0.f);
            r.z = fmaxf(ad.z + fast_tanh(v[2] + b), 0.f); r.w = fmaxf(ad.w + fast_tanh(v[3] + b), 0.f);
        } else {
            const float lo = (m0 + row < a.relu_rows) ? 0.f : -__builtin_inff();
            r.x = fmaxf(v[0] + b, lo); r.y = fmaxf(v[1] + b, lo); r.z = fmaxf(v[2] + b, lo); r.w = fmaxf(v[3] + b, lo);
        }
        *reinterpret_cast<float4*>(a.out + o) = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// MS-TCN after its entry convs + the block's residual and ReLU: 16 output channels x 4 output frames.  h has frames of VP
// floats; the block input x and the output are contiguous (N, C, T, V).  g: the group of a grouped launch, else 0.
// ---------------------------------------------------------------------------------------------------------------------
template <class Geo, class Args>
__device__ __forceinline__ void f2x_tcn_body(const Geo geo, const Args& a, const int g) {
    constexpr int NT = F2_NT, PB = Geo::PB, PH = Geo::PH, NCT = Geo::NCT, VP = Geo::VP, QF = Geo::QF, QT = F2_BT * Geo::QF;
    const int V = geo.V;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = a.res_mode == 2 ? (a.Cin + 15) & ~15 : 0;
    float* Pp = smem;                    // [4][16][PB]
    float* Ot = Pp + 4 * 16 * PB;        // [16][PB]      finished tile
    float* Us = Ot + 16 * PB;            // first [Kp][PB]: strided frames of the block input (convolutional residual), then
                                         // [Cb][PH]: this branch's entry output with the temporal halo
    const int nmt = a.Cout / 16;
    const int mtile = blockIdx.x % nmt, tt = blockIdx.x / nmt, n = blockIdx.y;
    const int c0 = mtile * 16, t0 = tt * F2_BT, bt = min(F2_BT, a.T2 - t0);
    const int branch = c0 / a.Cb, cb0 = c0 - branch * a.Cb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V, TVP = (long long)a.T * VP, TV2 = (long long)a.T2 * V;
    const bool temporal = branch < a.nb;
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.res_mode == 2) {
        f2x_stage<false>(geo, Us, a.x + (long long)n * a.Cin * TV + (long long)t0 * a.stride * V, TV, a.Cin, Kp, bt, a.stride, tid);
        __syncthreads();
        f2_gemm16<NCT>(acc, a.wr + (long long)g * a.Cout * a.Cin + (long long)(c0 + j) * a.Cin, a.Cin, a.vecr != 0, wave, Kp >> 4, 4, kq,
                       [&](int k, int ct) { return Us[k * PB + ct * 16 + j]; });
        if (temporal) __syncthreads();                             // (block-uniform) the region is staged again below
    }
    if (temporal) {
        const int d = a.dil[branch];
        const int pad = ((a.ks - 1) * d) / 2, tlo = t0 * a.stride - pad;
        const int nfr = (F2_BT - 1) * a.stride + (a.ks - 1) * d + 1;
        const float* hb = a.h + ((long long)n * a.Cout + branch * a.Cb) * TVP;
        const int cnt = a.Cb * nfr * QF;
        for (int e0 = tid; e0 < cnt; e0 += 8 * NT) {
            float4 q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = e0 + i * NT;
                const int ci = e / (nfr * QF), rem = e - ci * nfr * QF;
                const int f = rem / QF, v4 = (rem - f * QF) * 4;
                const int t = tlo + f;
                q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < cnt && t >= 0 && t < a.T) q[i] = *reinterpret_cast<const float4*>(hb + ci * TVP + (long long)t * VP + v4);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = e0 + i * NT;
                const int ci = e / (nfr * QF), rem = e - ci * nfr * QF;
                if (e < cnt) *reinterpret_cast<float4*>(Us + ci * PH + rem * 4) = q[i];
            }
        }
        __syncthreads();
        int boff[NCT];                                             // this lane's columns: (frame tl, joint v) of tile ct -> tap 0 inside a halo row
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int col = ct * 16 + j, tl = col / VP, v = col - tl * VP;
            boff[ct] = tl * a.stride * VP + v;
        }
        const int K = a.Cb * a.ks;
        f2_gemm16<NCT>(acc, a.wt[branch] + (long long)g * a.Cb * K + (long long)(cb0 + j) * K, K, a.vect != 0, wave, (K + 15) >> 4, 4, kq, [&](int k, int ct) {
            const int kk = k < K ? k : 0;                          // (the A element is zero there)
            const int ci = kk / a.ks, tap = kk - ci * a.ks;
            return Us[ci * PH + tap * d * VP + boff[ct]];
        });
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) Pp[(wave * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
    __syncthreads();
    const int Ch = (a.nb + 1) * a.Cb;
    for (int e = tid; e < 16 * QT; e += NT) {
        const int row = e / QT, c4 = (e - row * QT) * 4;
        const int tl = c4 / VP, v = c4 - tl * VP;
        if (tl >= bt) continue;
        f32x4 sum = *reinterpret_cast<const f32x4*>(Pp + row * PB + c4);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(Pp + (w * 16 + row) * PB + c4);
            sum += p;
        }
        const int c = c0 + row, cb = cb0 + row, tq = t0 + tl, ts = tq * a.stride;
        f32x4 val;
        if (temporal) {
            const float b = a.bt[branch][g * a.Cb + cb];
            val = (f32x4){b, b, b, b};
        } else if (branch == a.nb) {                               // MaxPool2d((3,1), stride, pad 1) of the ReLU'd entry output, then its BatchNorm
            const float* hp = a.h + ((long long)n * a.Cout + c) * TVP + v;
            f32x4 m = *reinterpret_cast<const f32x4*>(hp + (long long)ts * VP);
            if (ts - 1 >= 0) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(hp + (long long)(ts - 1) * VP);
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = fmaxf(m[i], q[i]);
            }
            if (ts + 1 < a.T) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(hp + (long long)(ts + 1) * VP);
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = fmaxf(m[i], q[i]);
            }
            const float sp = a.sp[g * a.Cb + cb], tp = a.tp[g * a.Cb + cb];
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] = fmaf(sp, m[i], tp);
        } else {                                                   // plain branch: computed with the entry convs (rows >= Ch of h)
            val = *reinterpret_cast<const f32x4*>(a.h + ((long long)n * a.Cout + Ch + cb) * TVP + (long long)ts * VP + v);
        }
        val += sum;
        if (a.res_mode == 1) {                                     // rows of V floats: elements, none past the frame
            const float* xr = a.x + ((long long)n * a.Cin + c) * TV + (long long)tq * V + v;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v + i < V) val[i] += xr[i];
        } else if (a.res_mode == 2) {
            const float b = a.br[g * a.Cout + c];
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] += b;
        }
        float4 r = make_float4(fmaxf(val[0], 0.f), v + 1 < V ? fmaxf(val[1], 0.f) : 0.f, v + 2 < V ? fmaxf(val[2], 0.f) : 0.f,
                               v + 3 < V ? fmaxf(val[3], 0.f) : 0.f);
        *reinterpret_cast<float4*>(Ot + row * PB + c4) = r;
    }
    __syncthreads();
    for (int e = tid; e < 16 * bt * V; e += NT) {                  // the block output: contiguous rows, element stores
        const int row = e / (bt * V), rem = e - row * (bt * V);
        const int tl = rem / V, v = rem - tl * V;
        a.out[((long long)n * a.Cout + c0 + row) * TV2 + (long long)t0 * V + rem] = Ot[row * PB + tl * VP + v];
    }
    if (a.xpart && tid < 16 * QF) {
        const int row = tid / QF, v4 = (tid - row * QF) * 4;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int tl = 0; tl < bt; ++tl) {
            const float4 q = *reinterpret_cast<const float4*>(Ot + row * PB + tl * VP + v4);
            o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
        }
        const int ntt = (a.T2 + F2_BT - 1) / F2_BT;
        *reinterpret_cast<float4*>(a.xpart + (((long long)n * ntt + tt) * a.Cout + c0 + row) * VP + v4) = o;
    }
}

}  // namespace
