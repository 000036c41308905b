// f2: the eval-mode TCN_GCN_unit for SMALL batches (the inference callers -- ensemble evaluation
// ensemble/ensemble_ctrgcn_resnet_eval.py:147-183, the frozen backbone of models/resnet_gcn_attention.py:82-85,
// visual.py:53-55 -- run model(data) on 1..16 clips).  At batch 1 an activation is 266 KB at every depth (C*T is constant
// down the network) and a block is 65 MFLOP: the training-size kernels (one workgroup per (sample, 64 channels, 16 frames),
// K loops with one DMA round trip per chunk) put 4..16 workgroups on a 256-CU chip and take 12..60 us each, 118 launches per
// forward.  This family cuts a block along its all-channel dependencies instead -- five launches, every one of them
// 50..130 workgroups per sample, operands staged ONCE per workgroup (an activation tile is <= 86 KB: it fits LDS whole) and
// no K-loop pipeline to fill:
//
//   f2_e     (n, subset, 16 channels)   xbar = mean_t x; p, q = W1/W2 xbar + b; D = tanh(p_u - q_v); E = alpha (W4 D + b4) + A
//                                       (models/ctrgcn.py:172-175 with conv1/conv2 commuted with the mean)
//   f2_gcn   (n, 8 channels, 4 frames)  x3 = W3 x + b3 for the tile's 24 rows and down(x) for its 8 (one 32-row MFMA product),
//                                       z = sum_s E_s x3_s, y = bn(z); writes y + res and res - y   (:176, :252-257)
//   f2_gemm  (n, 16 rows, 4 frames)     mode 0: g = relu(y + res + tanh(bn(Wo diff)))               (:219-223, :258-261)
//                                       mode 1: h = relu(bn(W_in g)) rows, plain-branch rows unclamped (:95-99, :121-124)
//   f2_tcn   (n, 16 channels, 4 frames) temporal branches (k x 1, dilated, strided), pooled branch, plain branch, residual
//                                       (identity / 1x1 strided conv), ReLU                           (:101-119, :145-146, :281-283)
//
// BatchNorm is folded into the weights by the caller (eval mode: a per-channel affine of the running statistics).
// All GEMMs: v_mfma_f32_16x16x4_f32 (exact fp32), A rows straight from global memory (L2-resident weights, 16 bytes per lane
// and 16-k block, prefetched one block ahead), B = the LDS tile, the K blocks of a product dealt round-robin to the waves and
// the partial tiles summed through LDS in a fixed order (deterministic).  V = 20 only.
#include "f2_common.h"

namespace {

constexpr int F2_V = 20, F2_VV = 400, F2_NCT = 5, F2_PB = 84;   // 4 frames (F2_BT) x 20 joints = 80 columns = 5 MFMA tiles
// pitch 84: the four k rows (4*kq + i) a fragment read touches sit 4*84 = 16 (mod 64) banks apart: conflict-free

// f2_load_a and f2_load_group are f2_common.h's.  This family's form of its f2_gemm16: the first group of A fragments (blocks
// kb0, kb0 + kbstep, ...) is in `a` already, requested by the caller ahead of whatever B waits for (the staging of the tile);
// K is taken whole (nkb blocks).
template <int NCT, class BF>
__device__ __forceinline__ void f2_gemm16_pre(f32x4 (&acc)[NCT], float (&a)[F2_G][4], const float* arow, int K, bool vec, int kb0, int kbstep, int kq, BF bf) {
    constexpr int G = F2_G;
    const int nkb = (K + 15) >> 4;
    float an[G][4];
    for (int kb = kb0; kb < nkb; kb += G * kbstep) {
        f2_load_group(arow, K, vec, kb + G * kbstep, nkb, kbstep, kq, an);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int b = kb + g * kbstep;
            if (b < nkb) {                                         // wave-uniform: a whole block of 4 x NCT MFMAs
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = b * 16 + 4 * kq + i;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) acc[ct] = mfma16(a[g][i], bf(k, ct), acc[ct]);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) a[g][i] = an[g][i];
    }
}

// the whole K of a row of A, nothing requested ahead
template <int NCT, class BF>
__device__ __forceinline__ void f2_gemm16_k(f32x4 (&acc)[NCT], const float* arow, int K, bool vec, int kb0, int kbstep, int kq, BF bf) {
    float a[F2_G][4];
    f2_load_group(arow, K, vec, kb0, (K + 15) >> 4, kbstep, kq, a);
    f2_gemm16_pre<NCT>(acc, a, arow, K, vec, kb0, kbstep, kq, bf);
}

// rows [0, K) of a (rows, T, V) activation, frames t0 + tl*fstep (tl < bt), as an LDS tile [Kp][F2_PB]; everything else zero
// (a zero A element times an uninitialised LDS word could be NaN)
__device__ __forceinline__ void f2_stage(float* Bs, const float* src, long long rs, int K, int Kp, int bt, int fstep, int tid) {
    constexpr int U = 8;                                           // loads in flight per thread (one L2 round trip per batch)
    for (int e0 = tid; e0 < Kp * 20; e0 += U * F2_NT) {
        float4 t[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int e = e0 + i * F2_NT;
            const int k = e / 20, c4 = (e - k * 20) * 4;
            const int tl = c4 / F2_V, v = c4 - tl * F2_V;
            t[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < Kp * 20 && k < K && tl < bt) t[i] = *reinterpret_cast<const float4*>(src + k * rs + (long long)tl * fstep * F2_V + v);
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int e = e0 + i * F2_NT;
            const int k = e / 20, c4 = (e - k * 20) * 4;
            if (e < Kp * 20) *reinterpret_cast<float4*>(Bs + k * F2_PB + c4) = t[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// ---- E for 16 channels of one (sample, subset)
constexpr int F2_PD = 404;                 // D pitch (4*404 = 16 mod 64)

__device__ __forceinline__ void f2_e_body(const F2GcnArgs& a) {
    constexpr int V = F2_V, VV = F2_VV, NT = F2_NT, PX = F2_PX, PD = F2_PD, NTP = 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.Cin + 15) & ~15, R2 = 2 * a.R, R2p = R2 < 16 ? 16 : R2, Rp = (a.R + 15) & ~15;
    float* XB = smem;                    // [Kp][PX]   xbar, columns >= 20 zero
    float* PQ = XB + Kp * PX;            // [R2p][PX]  p rows 0..R-1, q rows R..2R-1
    float* Pp = PQ + R2p * PX;           // [64][PX]   partial pq tiles
    float* Ds = Pp + 64 * PX;            // [Rp][PD]   D; before that: [NTP][Kp][V] partial frame sums
    const int nct = a.Cout / 16;
    const int s = blockIdx.x / nct, c0 = (blockIdx.x - s * nct) * 16, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V;
    // Everything that does not depend on x is requested now and used after the xbar phase: the kernel is a chain of dependent
    // round trips on 12..48 workgroups, not a bandwidth problem
    // pq product: 1 x 4, 2 x 2, 3 x 1 or 4 x 1 (row tiles x K parts) over the waves.  The row tiles round UP (2R = 24: two tiles,
    // the second half empty); with three the fourth wave (ppart == nparts) multiplies zeros into a partial tile nobody sums
    const int nrt = (R2p + 15) / 16, nparts = 4 / nrt;
    const int prt = wave % nrt, ppart = wave / nrt;
    const float* a12 = ppart < nparts && prt * 16 + j < R2 ? a.w12 + ((long long)s * R2 + prt * 16 + j) * a.Cin : nullptr;
    float a12g[F2_G][4];
    f2_load_group(a12, a.Cin, a.vec12 != 0, ppart, Kp >> 4, nparts, kq, a12g);
    float b12r[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) b12r[i] = tid + i * NT < R2 * V ? a.b12[s * R2 + (tid + i * NT) / V] : 0.f;
    const float alpha = a.alpha[0];
    float aw[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, b4r[4], Avr[7];
    {
        const float* arow = a.w4 + ((long long)s * a.Cout + c0 + j) * a.R;
        f2_load_a(arow, a.R, 0, kq, a.vec4 != 0, aw[0]);
        if (a.R > 16) f2_load_a(arow, a.R, 16, kq, a.vec4 != 0, aw[1]);
#pragma unroll
        for (int r = 0; r < 4; ++r) b4r[r] = a.b4[s * a.Cout + c0 + kq * 4 + r];
#pragma unroll
        for (int i = 0; i < 7; ++i) Avr[i] = wave + 4 * i < VV / 16 ? a.A[s * VV + (wave + 4 * i) * 16 + j] : 0.f;
    }
    // 1. xbar.  From the producer's per-tile column sums when it left them (f2_tcn: [N][tiles][Cin][V]; reading all of x
    // again in each of these workgroups was 10-20 us of dependent round trips), else from x: four frame phases in parallel.
    // Either way summed in a fixed order.
    {
        float* XP = Ds;
        const float inv = 1.f / (float)a.T;
        if (a.xpart) {
            // (tile group g, channel, joint quad): NTP groups of tpg tiles each; eight such sums advance together, one tile (= one
            // load each, eight in flight) per step
            const int ntt = (a.T + F2_BT - 1) / F2_BT, tpg = (ntt + NTP - 1) / NTP;
            const float* xp = a.xpart + (long long)n * ntt * a.Cin * V;
            const int cnt = NTP * a.Cin * 5;
            for (int e0 = tid; e0 < cnt; e0 += 8 * NT) {
                float4 acc[8];
                int off[8], g8[8];
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int e = e0 + p * NT;
                    const int g = e / (a.Cin * 5), rem = e - g * a.Cin * 5;
                    const int ci = rem / 5, v4 = (rem - ci * 5) * 4;
                    acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                    off[p] = ci * V + v4;
                    g8[p] = e < cnt ? g : NTP;                      // NTP * tpg >= ntt: an out-of-range pair never loads
                }
                for (int i = 0; i < tpg; ++i) {
                    float4 q[8];
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        const int tile = g8[p] * tpg + i;
                        q[p] = tile < ntt ? *reinterpret_cast<const float4*>(xp + (long long)tile * a.Cin * V + off[p]) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int p = 0; p < 8; ++p) { acc[p].x += q[p].x; acc[p].y += q[p].y; acc[p].z += q[p].z; acc[p].w += q[p].w; }
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int e = e0 + p * NT;
                    if (e < cnt) *reinterpret_cast<float4*>(XP + (g8[p] * Kp) * V + off[p]) = acc[p];
                }
            }
        } else {
            const float* xb = a.x + (long long)n * a.Cin * TV;
            for (int e = tid; e < NTP * a.Cin * 5; e += NT) {
                const int tp = e / (a.Cin * 5), rem = e - tp * a.Cin * 5;
                const int ci = rem / 5, v4 = (rem - ci * 5) * 4;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                const float* p = xb + ci * TV + v4;
                for (int t = tp; t < a.T; t += 8 * NTP) {              // eight loads in flight, summed in frame order
                    float4 q[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        q[i] = t + i * NTP < a.T ? *reinterpret_cast<const float4*>(p + (long long)(t + i * NTP) * V) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { acc.x += q[i].x; acc.y += q[i].y; acc.z += q[i].z; acc.w += q[i].w; }
                }
                *reinterpret_cast<float4*>(XP + (tp * Kp + ci) * V + v4) = acc;
            }
        }
        __syncthreads();
        {
            for (int e = tid; e < Kp * (PX / 4); e += NT) {
                const int ci = e / (PX / 4), v4 = (e - ci * (PX / 4)) * 4;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ci < a.Cin && v4 < V) {
#pragma unroll
                    for (int tp = 0; tp < NTP; ++tp) {
                        const float4 q = *reinterpret_cast<const float4*>(XP + (tp * Kp + ci) * V + v4);
                        o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
                    }
                    o.x *= inv; o.y *= inv; o.z *= inv; o.w *= inv;
                }
                *reinterpret_cast<float4*>(XB + ci * PX + v4) = o;
            }
        }
        __syncthreads();
    }
    // 2. p, q = W12_s xbar + b12_s: (2R x Cin) x (Cin x 20)
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        f2_gemm16_pre<2>(acc, a12g, a12, a.Cin, a.vec12 != 0, ppart, nparts, kq, [&](int k, int ct) { return XB[k * PX + ct * 16 + j]; });
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Pp[((ppart * nrt + prt) * 16 + kq * 4 + r) * PX + ct * 16 + j] = acc[ct][r];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 5; ++i) {
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
    // 3. D[r][u*V + v] = tanh(p[r][u] - q[r][v]); rows R..Rp zero
    for (int e = tid; e < Rp * VV; e += NT) {
        const int r = e / VV, uv = e - r * VV;
        const int u = uv / V, v = uv - u * V;
        Ds[r * PD + uv] = r < a.R ? fast_tanh(PQ[r * PX + u] - PQ[(a.R + r) * PX + v]) : 0.f;
    }
    __syncthreads();
    // 4. E tile = alpha (W4 D + b4) + A: 16 channels x 400, 25 column tiles over the four waves, K = R <= 32
    {
        float* Eg = a.E + (((long long)n * a.S + s) * a.Cout + c0) * VV;
#pragma unroll
        for (int it = 0; it < 7; ++it) {
            const int ct = wave + 4 * it;
            if (ct < VV / 16) {
                const int col = ct * 16 + j;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) acc = mfma16(aw[0][i], Ds[(4 * kq + i) * PD + col], acc);
                if (a.R > 16) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = mfma16(aw[1][i], Ds[(16 + 4 * kq + i) * PD + col], acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) Eg[(long long)(kq * 4 + r) * VV + col] = alpha * (acc[r] + b4r[r]) + Avr[it];
            }
        }
    }
}

__global__ __launch_bounds__(F2_NT) void f2_e_kernel(const F2GcnArgs a) { f2_e_body(a); }
__global__ __launch_bounds__(F2_NT) void f2_e_grouped_kernel(const F2GcnArgs a, int npg) { f2_e_body(f2_group(a, blockIdx.y / npg, F2_VV)); }

// ---- x3 GEMM + aggregation + BatchNorm + residual for 8 channels x 4 frames
constexpr int F2_ES = 3328;                // E run of one subset: 8 * 400 floats = 12.5 DMA pieces of 1 KB, padded to 13

__device__ __forceinline__ void f2_gcn_body(const F2GcnArgs& a) {
    constexpr int V = F2_V, VV = F2_VV, NT = F2_NT, PB = F2_PB, CT = F2_CT, ES = F2_ES;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.Cin + 15) & ~15;
    float* Xs = smem;                    // [Kp][PB]      x tile
    float* X3 = Xs + Kp * PB;            // [2][32][PB]   partial products: rows s*8 + c (s < 3), 24 + c = down(x)
    float* Es = X3 + 2 * 32 * PB;        // [3][ES]       E_s[c][u][v]
    const int nct = a.Cout / CT;
    const int ctile = blockIdx.x % nct, tt = blockIdx.x / nct, n = blockIdx.y;
    const int c0 = ctile * CT, t0 = tt * F2_BT, bt = min(F2_BT, a.T - t0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V;
    // E tiles travel by LDS-DMA under the x tile's staging and the GEMM (the barrier below drains them)
    for (int p = wave; p < 3 * 13; p += 4) {
        const int s = p / 13, q = p - s * 13;
        int f = q * 256 + lane * 4;
        if (f > CT * VV - 4) f = CT * VV - 4;                     // lanes past the run re-read its last slot into the padding
        const float* g = a.E + (((long long)n * a.S + s) * a.Cout + c0) * VV + f;
        __builtin_amdgcn_global_load_lds((tg_gptr)g, (tg_lptr)(Es + s * ES + q * 256), 16, 0, 0);
    }
    const int rt = wave & 1, kh = wave >> 1;
    const float* arow;
    bool vec;
    {
        const int row = rt * 16 + j, sidx = row >> 3, c = row & 7;
        arow = sidx < 3 ? a.w3 + ((long long)sidx * a.Cout + c0 + c) * a.Cin
                        : (a.res_mode == 2 ? a.wd + (long long)(c0 + c) * a.Cin : nullptr);
        vec = sidx < 3 ? a.vec3 != 0 : a.vecd != 0;               // (uniform per 8 lanes, both paths are branch-safe)
    }
    float ag[F2_G][4];
    f2_load_group(arow, a.Cin, vec, kh, Kp >> 4, 2, kq, ag);                // weights travel under the staging of the tile
    f2_stage(Xs, a.x + (long long)n * a.Cin * TV + (long long)t0 * V, TV, a.Cin, Kp, bt, 1, tid);
    __syncthreads();
    {
        f32x4 acc[F2_NCT];
#pragma unroll
        for (int ct = 0; ct < F2_NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f2_gemm16_pre<F2_NCT>(acc, ag, arow, a.Cin, vec, kh, 2, kq, [&](int k, int ct) { return Xs[k * PB + ct * 16 + j]; });
#pragma unroll
        for (int ct = 0; ct < F2_NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) X3[((kh * 32) + rt * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
    }
    __syncthreads();
    // aggregation: thread = (channel c, frame t, joint group ug): u = ug, ug + 8, ug + 16
    {
        const int c = tid >> 5, t = (tid >> 3) & 3, ug = tid & 7;
        float x3v[3 * V];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const float b = a.b3[s * a.Cout + c0 + c];
#pragma unroll
            for (int v4 = 0; v4 < V; v4 += 4) {
                const f32x4 p0 = *reinterpret_cast<const f32x4*>(X3 + (s * 8 + c) * PB + t * V + v4);
                const f32x4 p1 = *reinterpret_cast<const f32x4*>(X3 + (32 + s * 8 + c) * PB + t * V + v4);
#pragma unroll
                for (int i = 0; i < 4; ++i) x3v[s * V + v4 + i] = p0[i] + p1[i] + b;
            }
        }
        const float sy = a.sy[c0 + c], ty = a.ty[c0 + c];
        const float bd = a.res_mode == 2 ? a.bd[c0 + c] : 0.f;
        if (t < bt) {
            for (int u = ug; u < V; u += 8) {
                float z = 0.f;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const float* er = Es + s * ES + (c * V + u) * V;
#pragma unroll
                    for (int v4 = 0; v4 < V; v4 += 4) {
                        const f32x4 e = *reinterpret_cast<const f32x4*>(er + v4);
#pragma unroll
                        for (int i = 0; i < 4; ++i) z = fmaf(e[i], x3v[s * V + v4 + i], z);
                    }
                }
                const float y = fmaf(sy, z, ty);
                float res = 0.f;
                const int col = t * V + u;
                if (a.res_mode == 1) res = Xs[(c0 + c) * PB + col];
                else if (a.res_mode == 2) res = X3[(24 + c) * PB + col] + X3[(32 + 24 + c) * PB + col] + bd;
                const long long o = ((long long)n * a.Cout + c0 + c) * TV + (long long)(t0 + t) * V + u;
                a.sum[o] = y + res;
                a.diff[o] = res - y;
            }
        }
    }
}

__global__ __launch_bounds__(F2_NT) void f2_gcn_kernel(const F2GcnArgs a) { f2_gcn_body(a); }
__global__ __launch_bounds__(F2_NT) void f2_gcn_grouped_kernel(const F2GcnArgs a, int npg) { f2_gcn_body(f2_group(a, blockIdx.y / npg, F2_VV)); }

// ---------------------------------------------------------------------------------------------------------------------
// 16 rows x 4 frames of a pointwise product with the block's epilogues
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void f2_gemm_body(const F2GemmArgs& a) {
    constexpr int V = F2_V, NT = F2_NT, PB = F2_PB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.K + 15) & ~15;
    float* Bs = smem;                    // [Kp][PB]
    float* Pp = Bs + Kp * PB;            // [4][16][PB]
    const int nmt = a.M / 16;
    const int mtile = blockIdx.x % nmt, tt = blockIdx.x / nmt, n = blockIdx.y;
    const int m0 = mtile * 16, t0 = tt * F2_BT, bt = min(F2_BT, a.T - t0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V;
    const float* arow = a.w + (long long)(m0 + j) * a.K;
    float ag[F2_G][4];
    f2_load_group(arow, a.K, a.vec != 0, wave, Kp >> 4, 4, kq, ag);         // weights travel under the staging of the tile
    f2_stage(Bs, a.x + (long long)n * a.K * TV + (long long)t0 * V, TV, a.K, Kp, bt, 1, tid);
    __syncthreads();
    {
        f32x4 acc[F2_NCT];
#pragma unroll
        for (int ct = 0; ct < F2_NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f2_gemm16_pre<F2_NCT>(acc, ag, arow, a.K, a.vec != 0, wave, 4, kq, [&](int k, int ct) { return Bs[k * PB + ct * 16 + j]; });
#pragma unroll
        for (int ct = 0; ct < F2_NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Pp[(wave * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
    }
    __syncthreads();
    for (int e = tid; e < 16 * 20; e += NT) {
        const int row = e / 20, c4 = (e - row * 20) * 4;
        if (c4 >= bt * V) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(Pp + row * PB + c4);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(Pp + (w * 16 + row) * PB + c4);
            v += p;
        }
        const float b = a.b[m0 + row];
        const long long o = ((long long)n * a.M + m0 + row) * TV + (long long)t0 * V + c4;
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

__global__ __launch_bounds__(F2_NT) void f2_gemm_kernel(const F2GemmArgs a) { f2_gemm_body(a); }
__global__ __launch_bounds__(F2_NT) void f2_gemm_grouped_kernel(const F2GemmArgs a, int npg) { f2_gemm_body(f2_group(a, blockIdx.y / npg)); }

// ---------------------------------------------------------------------------------------------------------------------
// MS-TCN after its entry convs + the block's residual and ReLU: 16 output channels x 4 output frames
// ---------------------------------------------------------------------------------------------------------------------
constexpr int F2_PH = F2_HF * F2_V + 4;      // halo tile pitch

__device__ __forceinline__ void f2_tcn_body(const F2TcnArgs& a, const int g) {
    constexpr int V = F2_V, NT = F2_NT, PB = F2_PB, PH = F2_PH;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = a.res_mode == 2 ? (a.Cin + 15) & ~15 : 0;
    float* Pp = smem;                    // [4][16][PB]
    float* Ot = Pp + 4 * 16 * PB;        // [16][PB]      finished tile (for the column sums)
    float* Xs = Ot + 16 * PB;            // [Kp][PB]      strided frames of the block input (convolutional residual)
    float* Hs = Xs + Kp * PB;            // [Cb][PH]      this branch's entry output with the temporal halo
    const int nmt = a.Cout / 16;
    const int mtile = blockIdx.x % nmt, tt = blockIdx.x / nmt, n = blockIdx.y;
    const int c0 = mtile * 16, t0 = tt * F2_BT, bt = min(F2_BT, a.T2 - t0);
    const int branch = c0 / a.Cb, cb0 = c0 - branch * a.Cb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V, TV2 = (long long)a.T2 * V;
    const bool temporal = branch < a.nb;
    int d = 1, pad = 0, tlo = 0;
    if (temporal) {
        d = a.dil[branch];
        pad = ((a.ks - 1) * d) / 2;
        tlo = t0 * a.stride - pad;
        const int nfr = (F2_BT - 1) * a.stride + (a.ks - 1) * d + 1;
        const float* hb = a.h + ((long long)n * a.Cout + branch * a.Cb) * TV;
        const int cnt = a.Cb * nfr * 5;
        for (int e0 = tid; e0 < cnt; e0 += 8 * NT) {
            float4 q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = e0 + i * NT;
                const int ci = e / (nfr * 5), rem = e - ci * nfr * 5;
                const int f = rem / 5, v4 = (rem - f * 5) * 4;
                const int t = tlo + f;
                q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < cnt && t >= 0 && t < a.T) q[i] = *reinterpret_cast<const float4*>(hb + ci * TV + (long long)t * V + v4);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = e0 + i * NT;
                const int ci = e / (nfr * 5), rem = e - ci * nfr * 5;
                const int f = rem / 5, v4 = (rem - f * 5) * 4;
                if (e < cnt) *reinterpret_cast<float4*>(Hs + ci * PH + f * V + v4) = q[i];
            }
        }
    }
    if (a.res_mode == 2)
        f2_stage(Xs, a.x + (long long)n * a.Cin * TV + (long long)t0 * a.stride * V, TV, a.Cin, Kp, bt, a.stride, tid);
    __syncthreads();
    {
        f32x4 acc[F2_NCT];
#pragma unroll
        for (int ct = 0; ct < F2_NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (temporal) {
            // this lane's columns: (frame tl, joint v) of tile ct -> offset of tap 0 inside a halo row
            int boff[F2_NCT];
#pragma unroll
            for (int ct = 0; ct < F2_NCT; ++ct) {
                const int col = ct * 16 + j, tl = col / V, v = col - tl * V;
                boff[ct] = tl * a.stride * V + v;
            }
            const int K = a.Cb * a.ks;
            f2_gemm16_k<F2_NCT>(acc, a.wt[branch] + (long long)g * a.Cb * K + (long long)(cb0 + j) * K, K, a.vect != 0, wave, 4, kq, [&](int k, int ct) {
                const int ci = k / a.ks, tap = k - ci * a.ks;
                return Hs[ci * PH + tap * d * V + boff[ct]];
            });
        }
        if (a.res_mode == 2)
            f2_gemm16_k<F2_NCT>(acc, a.wr + (long long)g * a.Cout * a.Cin + (long long)(c0 + j) * a.Cin, a.Cin, a.vecr != 0, wave, 4, kq,
                                [&](int k, int ct) { return Xs[k * PB + ct * 16 + j]; });
#pragma unroll
        for (int ct = 0; ct < F2_NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Pp[(wave * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
    }
    __syncthreads();
    const int Ch = (a.nb + 1) * a.Cb;
    for (int e = tid; e < 16 * 20; e += NT) {
        const int row = e / 20, c4 = (e - row * 20) * 4;
        const int tl = c4 / V, v = c4 - tl * V;
        if (tl >= bt) continue;
        f32x4 acc = *reinterpret_cast<const f32x4*>(Pp + row * PB + c4);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(Pp + (w * 16 + row) * PB + c4);
            acc += p;
        }
        const int c = c0 + row, cb = cb0 + row, tq = t0 + tl, ts = tq * a.stride;
        f32x4 val;
        if (temporal) {
            const float b = a.bt[branch][g * a.Cb + cb];
            val = (f32x4){b, b, b, b};
        } else if (branch == a.nb) {                               // MaxPool2d((3,1), stride, pad 1) of the ReLU'd entry output, then its BatchNorm
            const float* hp = a.h + ((long long)n * a.Cout + c) * TV + v;
            f32x4 m = *reinterpret_cast<const f32x4*>(hp + (long long)ts * V);
            if (ts - 1 >= 0) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(hp + (long long)(ts - 1) * V);
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = fmaxf(m[i], q[i]);
            }
            if (ts + 1 < a.T) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(hp + (long long)(ts + 1) * V);
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = fmaxf(m[i], q[i]);
            }
            const float sp = a.sp[g * a.Cb + cb], tp = a.tp[g * a.Cb + cb];
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] = fmaf(sp, m[i], tp);
        } else {                                                   // plain branch: computed with the entry convs (rows >= Ch of h)
            val = *reinterpret_cast<const f32x4*>(a.h + ((long long)n * a.Cout + Ch + cb) * TV + (long long)ts * V + v);
        }
        val += acc;
        if (a.res_mode == 1) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(a.x + ((long long)n * a.Cin + c) * TV + (long long)tq * V + v);
            val += q;
        } else if (a.res_mode == 2) {
            const float b = a.br[g * a.Cout + c];
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] += b;
        }
        float4 r = make_float4(fmaxf(val[0], 0.f), fmaxf(val[1], 0.f), fmaxf(val[2], 0.f), fmaxf(val[3], 0.f));
        *reinterpret_cast<float4*>(a.out + ((long long)n * a.Cout + c) * TV2 + (long long)tq * V + v) = r;
        *reinterpret_cast<float4*>(Ot + row * PB + c4) = r;
    }
    if (a.xpart) {
        __syncthreads();
        if (tid < 16 * 5) {
            const int row = tid / 5, v4 = (tid - row * 5) * 4;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int tl = 0; tl < bt; ++tl) {
                const float4 q = *reinterpret_cast<const float4*>(Ot + row * PB + tl * V + v4);
                o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
            }
            const int ntt = (a.T2 + F2_BT - 1) / F2_BT;
            *reinterpret_cast<float4*>(a.xpart + (((long long)n * ntt + tt) * a.Cout + c0 + row) * V + v4) = o;
        }
    }
}

__global__ __launch_bounds__(F2_NT) void f2_tcn_kernel(const F2TcnArgs a) { f2_tcn_body(a, 0); }
__global__ __launch_bounds__(F2_NT) void f2_tcn_grouped_kernel(const F2TcnArgs a, int npg) { f2_tcn_body(a, blockIdx.y / npg); }

constexpr size_t f2_e_lds(int Cin, int R) { return f2_e_lds(Cin, R, 4, F2_V, F2_PD); }
constexpr size_t f2_gcn_lds(int Cin) { return f2_gcn_lds(Cin, 256, F2_PB, F2_ES); }                // the whole K in one chunk
constexpr size_t f2_gemm_lds(int K) { return f2_gemm_lds(K, F2_PB); }
size_t f2_tcn_lds(int Cin, int Cb, int res_mode) {                                                 // two regions, side by side
    return sizeof(float) * ((size_t)5 * 16 * F2_PB + (size_t)(res_mode == 2 ? (Cin + 15) & ~15 : 0) * F2_PB + (size_t)Cb * F2_PH);
}

bool f2_served(int V) { return V == F2_V; }
// (the gcn descriptors and the pointwise ones have always been told apart in the text of a refused V)
const F2Family F2_GCN_FAMILY = {f2_served, "this family is built for V = 20, S = 3", "null pointer", 16, "x, E and xpart must be 16-byte aligned", nullptr, true};
const F2Family F2_FAMILY = {f2_served, "built for V = 20", "null pointer", 16, nullptr, "activations must be 16-byte aligned", false};

// groups == 0: the plain entry point; otherwise the grouped one.
int f2_e_launch(const tamgcn_f2_gcn_desc* d, int groups, void* stream, const char* who) {
    F2GcnArgs a;
    if (f2_gcn_args(d, &a, F2_GCN_FAMILY, false, who) || f2_gcn_groups_ok(a, groups, who)) return -1;
    const dim3 grid(d->S * (d->Cout / 16), d->N);
    if (groups) {
        tg_launch_lds<f2_e_grouped_kernel>(f2_e_lds(256, 32), grid, dim3(F2_NT), f2_e_lds(d->Cin, d->R), (hipStream_t)stream, a, d->N / groups);
        tamgcn_note_kernel("f2_e_grouped_kernel");
    } else {
        tg_launch_lds<f2_e_kernel>(f2_e_lds(256, 32), grid, dim3(F2_NT), f2_e_lds(d->Cin, d->R), (hipStream_t)stream, a);
        tamgcn_note_kernel("f2_e_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

int f2_gcn_launch(const tamgcn_f2_gcn_desc* d, int groups, void* stream, const char* who) {
    F2GcnArgs a;
    if (f2_gcn_args(d, &a, F2_GCN_FAMILY, true, who) || f2_gcn_groups_ok(a, groups, who)) return -1;
    const dim3 grid(ceil_div(d->T, F2_BT) * (d->Cout / F2_CT), d->N);
    if (groups) {
        tg_launch_lds<f2_gcn_grouped_kernel>(f2_gcn_lds(256), grid, dim3(F2_NT), f2_gcn_lds(d->Cin), (hipStream_t)stream, a, d->N / groups);
        tamgcn_note_kernel("f2_gcn_grouped_kernel");
    } else {
        tg_launch_lds<f2_gcn_kernel>(f2_gcn_lds(256), grid, dim3(F2_NT), f2_gcn_lds(d->Cin), (hipStream_t)stream, a);
        tamgcn_note_kernel("f2_gcn_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

int f2_gemm_launch(const tamgcn_f2_gemm_desc* d, int groups, void* stream, const char* who) {
    F2GemmArgs a;
    if (f2_gemm_args(d, &a, F2_FAMILY, who) || f2_gemm_groups_ok(a, groups, who)) return -1;
    const dim3 grid(ceil_div(d->T, F2_BT) * (d->M / 16), d->N);
    if (groups) {
        tg_launch_lds<f2_gemm_grouped_kernel>(f2_gemm_lds(256), grid, dim3(F2_NT), f2_gemm_lds(d->K), (hipStream_t)stream, a, d->N / groups);
        tamgcn_note_kernel("f2_gemm_grouped_kernel");
    } else {
        tg_launch_lds<f2_gemm_kernel>(f2_gemm_lds(256), grid, dim3(F2_NT), f2_gemm_lds(d->K), (hipStream_t)stream, a);
        tamgcn_note_kernel("f2_gemm_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

int f2_tcn_launch(const tamgcn_f2_tcn_desc* d, int groups, void* stream, const char* who) {
    F2TcnArgs a;
    if (f2_tcn_args(d, &a, F2_FAMILY, who)) return -1;
    const size_t lds = f2_tcn_lds(d->Cin, d->Cb, d->res_mode);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    if (f2_tcn_groups_ok(a, groups, who)) return -1;
    const dim3 grid(ceil_div(a.T2, F2_BT) * (d->Cout / 16), d->N);
    if (groups) {
        tg_launch_lds<f2_tcn_grouped_kernel>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a, d->N / groups);
        tamgcn_note_kernel("f2_tcn_grouped_kernel");
    } else {
        tg_launch_lds<f2_tcn_kernel>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a);
        tamgcn_note_kernel("f2_tcn_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" int tamgcn_f2_e(const tamgcn_f2_gcn_desc* d, void* stream) { return f2_e_launch(d, 0, stream, "tamgcn_f2_e"); }
extern "C" int tamgcn_f2_gcn(const tamgcn_f2_gcn_desc* d, void* stream) { return f2_gcn_launch(d, 0, stream, "tamgcn_f2_gcn"); }
extern "C" int tamgcn_f2_gemm(const tamgcn_f2_gemm_desc* d, void* stream) { return f2_gemm_launch(d, 0, stream, "tamgcn_f2_gemm"); }
extern "C" int tamgcn_f2_tcn(const tamgcn_f2_tcn_desc* d, void* stream) { return f2_tcn_launch(d, 0, stream, "tamgcn_f2_tcn"); }

extern "C" int tamgcn_f2_e_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2_e_grouped") ? -1 : f2_e_launch(d, groups, stream, "tamgcn_f2_e_grouped");
}
extern "C" int tamgcn_f2_gcn_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2_gcn_grouped") ? -1 : f2_gcn_launch(d, groups, stream, "tamgcn_f2_gcn_grouped");
}
extern "C" int tamgcn_f2_gemm_grouped(const tamgcn_f2_gemm_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2_gemm_grouped") ? -1 : f2_gemm_launch(d, groups, stream, "tamgcn_f2_gemm_grouped");
}
extern "C" int tamgcn_f2_tcn_grouped(const tamgcn_f2_tcn_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2_tcn_grouped") ? -1 : f2_tcn_launch(d, groups, stream, "tamgcn_f2_tcn_grouped");
}
