// f2g: the small-batch eval-mode TCN_GCN_unit (f2.hip's family: same four stages, same algebra, include/tamgcn.h) for ANY
// joint count 8 <= V <= 28, with V a KERNEL ARGUMENT.  f2v.hip instantiates its kernels per joint count (17, 18, 25) and f2.hip
// is written for 20; every other skeleton used to take the general eval path at batch 1.  This file is to f2v.hip what vgen.hip
// is to ctrgc_tiled.hip: the same layout and tiling, templated only on what sizes a register array or fixes an LDS pitch --
// the frame pitch VP = (V + 3) & ~3 in {8, 12, 16, 20, 24, 28}: six instantiations per stage serve 21 joint counts.
//
//   layout      f2v's (include/tamgcn.h).  The block's input and output are contiguous (N, C, T, V); E, sum, diff, g, h and
//               xpart have frames of VP floats, pad columns V..VP-1 of E, sum, diff, xpart exactly zero.  The contiguous input
//               is read in 16-byte pieces from dword-aligned addresses; the last piece of a frame keeps its first
//               V - (VP - 4) lanes (1..4, a run-time count), the others are REPLACED by zeros.  At V % 4 == 0 nothing is padded.
//   run time    everything f2v derives from V * VP: the E run of a channel (EC = V * VP floats), its column tiles, the D pitch
//               (ECT * 16 + 4: conflict-free for every ECT), the 1 KB DMA pieces of a subset's E run, and every `joint < V`
//               predicate.  Register arrays are sized for V = VP and guarded by wave-uniform run-time counts.
//   LDS         f2v's constants do not fit at the wide end: the gcn stage at V = 28 holds three E runs of 25.6 KB and two
//               partial x3 tiles of 29.7 KB, which leaves 52 KB for the K chunk, not the 59 KB of 128 rows.  The host picks the
//               K chunk per geometry (fg_gcn_kc: the largest multiple of 16 up to 128 that fits 160 KB; 112 rows at V = 28, 128
//               everywhere else), and the E builder takes two frame phases instead of four where four partial tiles do not
//               fit (f2v's rule).  tamgcn_f2g_lds_bytes reports every stage's request; nothing above 160 KB is launched.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 (exact fp32), the K blocks of a product dealt round-robin to the waves, the partial tiles
// summed through LDS in a fixed order, no atomics: two runs are bit-equal.  S = 3.  No grouped entry points.
#include "common.h"

namespace {

constexpr int FG_NT = 256, FG_BT = 4, FG_G = 4, FG_KC = 128, FG_HF = 15, FG_PX = 36, FG_CT = 8;
constexpr int FG_VMIN = 8, FG_VMAX = 28;
constexpr size_t FG_LDS_MAX = 160 * 1024;

// What the frame pitch fixes.  The run-time half (EC, ECT, PD, EPC, ES) is FgRt.
template <int VP> struct FgGeo {
    static constexpr int QF = VP / 4;                  // 16-byte pieces per frame
    static constexpr int NC = FG_BT * VP;              // columns of a tile
    static constexpr int NCT = NC / 16;                // MFMA column tiles
    static constexpr int PB = NC + 4;                  // tile pitch: the four k rows of a fragment read sit 16 banks apart
    static constexpr int PH = FG_HF * VP + 4;          // halo tile pitch
    static constexpr int NIT = ((VP * VP + 15) / 16 + 3) / 4;   // E column tiles per wave at V = VP
    static constexpr int NB = VP / 4;                  // 64 * VP / 256: pq elements per thread at R = 32, V = VP
    static_assert(VP % 4 == 0 && VP >= 8 && VP <= 28 && NC % 16 == 0, "geometry: whole MFMA tiles, xbar in two tiles");
    static_assert((4 * PB) % 64 == 16, "conflict-free pitch");
};

struct FgRt {
    int EC, ECT, PD, EPC, ES;
    __host__ __device__ FgRt(int V, int VP) {
        EC = V * VP;                                   // floats of one channel of E: rows u of VP
        ECT = (EC + 15) >> 4;                          // column tiles of the E product
        PD = ECT * 16 + 4;                             // D pitch (4 PD % 64 == 16 for every ECT)
        EPC = (FG_CT * EC + 255) >> 8;                 // 1 KB DMA pieces of one subset's E run (FG_CT * EC >= 512)
        ES = EPC * 256;
    }
};

__device__ __forceinline__ void fg_load_a(const float* arow, int K, int k0, int kq, bool vec, float (&a)[4]) {
    const int k = k0 + 4 * kq;
    if (vec) {
        const float4 t = arow ? *reinterpret_cast<const float4*>(arow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = (arow && k + i < K) ? arow[k + i] : 0.f;
    }
}

// blocks kb, kb + kbstep, ... (< kbend) of a row of A
__device__ __forceinline__ void fg_load_group(const float* arow, int K, bool vec, int kb, int kbend, int kbstep, int kq, float (&dst)[FG_G][4]) {
#pragma unroll
    for (int g = 0; g < FG_G; ++g) {
        const int b = kb + g * kbstep;
        if (b < kbend) fg_load_a(arow, K, b * 16, kq, vec, dst[g]);
        else { dst[g][0] = dst[g][1] = dst[g][2] = dst[g][3] = 0.f; }
    }
}

// acc[ct] += A[16 rows][16-k blocks kb, kb + kbstep, ... < kbend] * B; this lane's B value for tile ct at row k is bf(k, ct).
// A fragments travel four blocks at a time, one group ahead (f2.hip).
template <int NCT, class BF>
__device__ __forceinline__ void fg_gemm16(f32x4 (&acc)[NCT], const float* arow, int K, bool vec, int kb, int kbend, int kbstep, int kq, BF bf) {
    constexpr int G = FG_G;
    float a[G][4], an[G][4];
    fg_load_group(arow, K, vec, kb, kbend, kbstep, kq, a);
    for (; kb < kbend; kb += G * kbstep) {
        fg_load_group(arow, K, vec, kb + G * kbstep, kbend, kbstep, kq, an);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int b = kb + g * kbstep;
            if (b < kbend) {                                       // wave-uniform
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

// Rows [0, rows) of an LDS tile [rows][PB] <- rows [0, K) of an activation, frames tl*fstep (tl < bt); everything else zero.
// PADDED: the source has frames of VP floats (the family's own buffers: aligned pieces, pad columns copied as they are).
// Otherwise frames of V floats from a dword-aligned address: the last piece of a frame keeps its first V - (VP - 4) lanes.
template <int VP, bool PADDED>
__device__ __forceinline__ void fg_stage(float* Bs, const float* src, long long rs, int K, int rows, int bt, int fstep, int V, int tid) {
    using G = FgGeo<VP>;
    constexpr int U = 8, QT = FG_BT * G::QF;
    const int FP = PADDED ? VP : V, last = V - (VP - 4);
    for (int e0 = tid; e0 < rows * QT; e0 += U * FG_NT) {
        float4 t[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int e = e0 + i * FG_NT;
            const int k = e / QT, r = e - k * QT;
            const int tl = r / G::QF, q = r - tl * G::QF;
            t[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < rows * QT && k < K && tl < bt) {
                t[i] = *reinterpret_cast<const float4*>(src + k * rs + (long long)tl * fstep * FP + 4 * q);
                if (!PADDED && q == G::QF - 1) {                   // lanes past the frame: the next frame or the slack behind the tensor
                    if (last < 2) t[i].y = 0.f;
                    if (last < 3) t[i].z = 0.f;
                    if (last < 4) t[i].w = 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int e = e0 + i * FG_NT;
            const int k = e / QT, r = e - k * QT;
            if (e < rows * QT) *reinterpret_cast<float4*>(Bs + k * G::PB + 4 * r) = t[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct FgGcnArgs {
    int N, Cin, Cout, T, V, S, R, res_mode;
    const float *x, *w12, *b12, *w4, *b4, *A, *alpha, *w3, *b3, *sy, *ty, *wd, *bd, *xpart;
    float *E, *sum, *diff;
    int vec12, vec4, vec3, vecd;
    int ntp;                             // f2g_e: frame phases of the xbar sum (4, or 2 where 4 partial tiles do not fit LDS)
    int kc;                              // f2g_gcn: K rows of a staged chunk (a multiple of 16, <= FG_KC)
};

// ---- E for 16 channels of one (sample, subset): E[c][u][v] at [c][u * VP + v], pad columns zero
template <int VP>
__global__ __launch_bounds__(FG_NT) void f2g_e_kernel(const FgGcnArgs a) {
    using G = FgGeo<VP>;
    constexpr int NT = FG_NT, PX = FG_PX, QF = G::QF, NB = G::NB, NIT = G::NIT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int V = a.V;
    const FgRt rt(V, VP);
    const int EC = rt.EC, ECT = rt.ECT, PD = rt.PD;
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
        fg_load_a(arow, a.R, 0, kq, a.vec4 != 0, aw[0]);
        if (a.R > 16) fg_load_a(arow, a.R, 16, kq, a.vec4 != 0, aw[1]);
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
            const int ntt = (a.T + FG_BT - 1) / FG_BT, tpg = (ntt + NTP - 1) / NTP;
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
        fg_gemm16<2>(acc, a12, a.Cin, a.vec12 != 0, ppart, Kp >> 4, nparts, kq, [&](int k, int ct) { return XB[k * PX + ct * 16 + j]; });
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
    {
        const int dw = ECT * 16;
        for (int e = tid; e < Rp * dw; e += NT) {
            const int r = e / dw, uv = e - r * dw;
            const int u = uv / VP, v = uv - u * VP;
            Ds[r * PD + uv] = (r < a.R && u < V && v < V) ? fast_tanh(PQ[r * PX + u] - PQ[(a.R + r) * PX + v]) : 0.f;
        }
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

// ---- x3 GEMM + aggregation + BatchNorm + residual for 8 channels x 4 frames; K staged in chunks of a.kc rows
template <int VP>
__global__ __launch_bounds__(FG_NT) void f2g_gcn_kernel(const FgGcnArgs a) {
    using G = FgGeo<VP>;
    constexpr int PB = G::PB, CT = FG_CT, NCT = G::NCT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int V = a.V;
    const FgRt rt(V, VP);
    const int EC = rt.EC, ES = rt.ES, EPC = rt.EPC;
    const int Kp = (a.Cin + 15) & ~15, Kc = Kp < a.kc ? Kp : a.kc;
    float* Xs = smem;                    // [Kc][PB]      one K chunk of the x tile
    float* X3 = Xs + Kc * PB;            // [2][32][PB]   partial products: rows s*8 + c (s < 3), 24 + c = down(x)
    float* Es = X3 + 2 * 32 * PB;        // [3][ES]       E_s[c][u][VP]
    const int nct = a.Cout / CT;
    const int ctile = blockIdx.x % nct, tt = blockIdx.x / nct, n = blockIdx.y;
    const int c0 = ctile * CT, t0 = tt * FG_BT, bt = min(FG_BT, a.T - t0);
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
    const int rtile = wave & 1, kh = wave >> 1;
    const float* arow;
    bool vec;
    {
        const int row = rtile * 16 + j, sidx = row >> 3, c = row & 7;
        arow = sidx < 3 ? a.w3 + ((long long)sidx * a.Cout + c0 + c) * a.Cin
                        : (a.res_mode == 2 ? a.wd + (long long)(c0 + c) * a.Cin : nullptr);
        vec = sidx < 3 ? a.vec3 != 0 : a.vecd != 0;
    }
    {
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Kp; k0 += Kc) {
            const int rows = min(Kc, Kp - k0);
            if (k0) __syncthreads();                               // the previous chunk has been consumed
            fg_stage<VP, false>(Xs, a.x + ((long long)n * a.Cin + k0) * TV + (long long)t0 * V, TV, a.Cin - k0, rows, bt, 1, V, tid);
            __syncthreads();
            fg_gemm16<NCT>(acc, arow, a.Cin, vec, (k0 >> 4) + kh, (k0 + rows) >> 4, 2, kq,
                           [&](int k, int ct) { return Xs[(k - k0) * PB + ct * 16 + j]; });
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) X3[((kh * 32) + rtile * 16 + kq * 4 + r) * PB + ct * 16 + j] = acc[ct][r];
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
                        if (v4 == VP - 4) {                        // the pad joints take no part: a select, E's pad columns are not trusted
                            if (VP - 3 >= V) e[1] = 0.f;
                            if (VP - 2 >= V) e[2] = 0.f;
                            if (VP - 1 >= V) e[3] = 0.f;
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i) z = fmaf(e[i], x3v[s * VP + v4 + i], z);
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
struct FgGemmArgs {
    int N, K, M, T, V, mode, relu_rows, vec;
    const float *x, *w, *b, *add;
    float* out;
};

template <int VP>
__global__ __launch_bounds__(FG_NT) void f2g_gemm_kernel(const FgGemmArgs a) {
    using G = FgGeo<VP>;
    constexpr int NT = FG_NT, PB = G::PB, NCT = G::NCT, QT = FG_BT * G::QF;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (a.K + 15) & ~15;
    float* Bs = smem;                    // [Kp][PB]
    float* Pp = Bs + Kp * PB;            // [4][16][PB]
    const int nmt = a.M / 16;
    const int mtile = blockIdx.x % nmt, tt = blockIdx.x / nmt, n = blockIdx.y;
    const int m0 = mtile * 16, t0 = tt * FG_BT, bt = min(FG_BT, a.T - t0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TVP = (long long)a.T * VP;
    const float* arow = a.w + (long long)(m0 + j) * a.K;
    fg_stage<VP, true>(Bs, a.x + (long long)n * a.K * TVP + (long long)t0 * VP, TVP, a.K, Kp, bt, 1, a.V, tid);
    __syncthreads();
    {
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
        fg_gemm16<NCT>(acc, arow, a.K, a.vec != 0, wave, Kp >> 4, 4, kq, [&](int k, int ct) { return Bs[k * PB + ct * 16 + j]; });
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
// floats; the block input x and the output are contiguous (N, C, T, V).
// ---------------------------------------------------------------------------------------------------------------------
struct FgTcnArgs {
    int N, Cin, Cout, T, T2, V, stride, Cb, nb, ks, res_mode, vect, vecr;
    int dil[4];
    const float* h;
    const float* wt[4]; const float* bt[4];
    const float *sp, *tp;
    const float *x, *wr, *br;
    float* out;
    float* xpart;                        // NULL | (N, ceil(T2 / 4), Cout, VP): sum over each tile's frames of out, pad joints zero
};

template <int VP>
__global__ __launch_bounds__(FG_NT) void f2g_tcn_kernel(const FgTcnArgs a) {
    using G = FgGeo<VP>;
    constexpr int NT = FG_NT, PB = G::PB, PH = G::PH, NCT = G::NCT, QF = G::QF, QT = FG_BT * G::QF;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int V = a.V;
    const int Kp = a.res_mode == 2 ? (a.Cin + 15) & ~15 : 0;
    float* Pp = smem;                    // [4][16][PB]
    float* Ot = Pp + 4 * 16 * PB;        // [16][PB]      finished tile
    float* Us = Ot + 16 * PB;            // first [Kp][PB]: strided frames of the block input (convolutional residual), then
                                         // [Cb][PH]: this branch's entry output with the temporal halo
    const int nmt = a.Cout / 16;
    const int mtile = blockIdx.x % nmt, tt = blockIdx.x / nmt, n = blockIdx.y;
    const int c0 = mtile * 16, t0 = tt * FG_BT, bt = min(FG_BT, a.T2 - t0);
    const int branch = c0 / a.Cb, cb0 = c0 - branch * a.Cb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long TV = (long long)a.T * V, TVP = (long long)a.T * VP, TV2 = (long long)a.T2 * V;
    const bool temporal = branch < a.nb;
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.res_mode == 2) {
        fg_stage<VP, false>(Us, a.x + (long long)n * a.Cin * TV + (long long)t0 * a.stride * V, TV, a.Cin, Kp, bt, a.stride, V, tid);
        __syncthreads();
        fg_gemm16<NCT>(acc, a.wr + (long long)(c0 + j) * a.Cin, a.Cin, a.vecr != 0, wave, Kp >> 4, 4, kq,
                       [&](int k, int ct) { return Us[k * PB + ct * 16 + j]; });
        if (temporal) __syncthreads();                             // (block-uniform) the region is staged again below
    }
    if (temporal) {
        const int d = a.dil[branch];
        const int pad = ((a.ks - 1) * d) / 2, tlo = t0 * a.stride - pad;
        const int nfr = (FG_BT - 1) * a.stride + (a.ks - 1) * d + 1;
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
        fg_gemm16<NCT>(acc, a.wt[branch] + (long long)(cb0 + j) * K, K, a.vect != 0, wave, (K + 15) >> 4, 4, kq, [&](int k, int ct) {
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
            const float b = a.bt[branch][cb];
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
            const float sp = a.sp[cb], tp = a.tp[cb];
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
            const float b = a.br[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] += b;
        }
        float4 r = make_float4(fmaxf(val[0], 0.f), v + 1 < V ? fmaxf(val[1], 0.f) : 0.f, v + 2 < V ? fmaxf(val[2], 0.f) : 0.f,
                               v + 3 < V ? fmaxf(val[3], 0.f) : 0.f);
        *reinterpret_cast<float4*>(Ot + row * PB + c4) = r;
    }
    __syncthreads();
    const int btv = bt * V;
    for (int e = tid; e < 16 * btv; e += NT) {                     // the block output: contiguous rows, element stores
        const int row = e / btv, rem = e - row * btv;
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
        const int ntt = (a.T2 + FG_BT - 1) / FG_BT;
        *reinterpret_cast<float4*>(a.xpart + (((long long)n * ntt + tt) * a.Cout + c0 + row) * VP + v4) = o;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
#define FG_PITCHES(X) X(8) X(12) X(16) X(20) X(24) X(28)
#define FG_SERVES "this family serves 8 <= V <= 28, S = 3"

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool fg_served(int V) { return V >= FG_VMIN && V <= FG_VMAX; }
inline int fg_vp(int V) { return (V + 3) & ~3; }

// The LDS requests, from the joint count: what the kernels above lay out.
size_t fg_e_lds(int V, int Cin, int R, int ntp) {
    const int VP = fg_vp(V), Kp = (Cin + 15) & ~15, R2p = 2 * R < 16 ? 16 : 2 * R, Rp = (R + 15) & ~15;
    const FgRt rt(V, VP);
    const size_t d = (size_t)Rp * rt.PD, xp = (size_t)ntp * Kp * VP;
    return sizeof(float) * ((size_t)Kp * FG_PX + (size_t)R2p * FG_PX + 64 * FG_PX + (d > xp ? d : xp));
}
int fg_e_ntp(int V, int Cin, int R) { return fg_e_lds(V, Cin, R, 4) <= FG_LDS_MAX ? 4 : 2; }
size_t fg_gcn_lds(int V, int Cin, int kc) {
    const int VP = fg_vp(V), PB = FG_BT * VP + 4, Kp = (Cin + 15) & ~15;
    const FgRt rt(V, VP);
    return sizeof(float) * ((size_t)(Kp < kc ? Kp : kc) * PB + 2 * 32 * PB + 3 * (size_t)rt.ES);
}
// the K chunk: the largest multiple of 16 up to FG_KC with which the stage fits (112 rows at V = 28, FG_KC below)
int fg_gcn_kc(int V, int Cin) {
    int kc = FG_KC;
    while (kc > 16 && fg_gcn_lds(V, Cin, kc) > FG_LDS_MAX) kc -= 16;
    return kc;
}
size_t fg_gemm_lds(int V, int K) { return sizeof(float) * ((size_t)(((K + 15) & ~15) + 4 * 16) * (FG_BT * fg_vp(V) + 4)); }
size_t fg_tcn_lds(int V, int Cin, int Cb, int res_mode) {
    const int VP = fg_vp(V), PB = FG_BT * VP + 4, PH = FG_HF * VP + 4;
    const size_t xs = (size_t)(res_mode == 2 ? (Cin + 15) & ~15 : 0) * PB, hs = (size_t)Cb * PH;
    return sizeof(float) * ((size_t)5 * 16 * PB + (xs > hs ? xs : hs));
}

// V first, on the host, before a pointer of the descriptor is looked at
template <class D> int fg_pick(const D* d, const char* who) {
    TG_CHECK(d, "%s: null descriptor (V=n/a; " FG_SERVES ")", who);
    TG_CHECK(fg_served(d->V), "%s: V=%d (" FG_SERVES ")", who, d->V);
    return 0;
}

int fg_fill(const tamgcn_f2_gcn_desc* d, FgGcnArgs* a, const char* who) {
    if (fg_pick(d, who)) return -1;
    TG_CHECK(d->S == 3, "%s: V=%d S=%d (" FG_SERVES ")", who, d->V, d->S);
    TG_CHECK(d->x && d->w12 && d->b12 && d->w4 && d->b4 && d->A && d->alpha && d->w3 && d->b3 && d->sy && d->ty && d->E,
             "%s: null pointer", who);
    TG_CHECK(d->N > 0 && d->T > 0 && d->Cin > 0 && d->Cin <= 256 && d->Cout > 0 && d->Cout % 16 == 0,
             "%s: bad shape N=%d T=%d Cin=%d Cout=%d (Cin <= 256, Cout %% 16 == 0)", who, d->N, d->T, d->Cin, d->Cout);
    TG_CHECK(d->R >= 1 && d->R <= 32, "%s: R=%d outside 1..32", who, d->R);
    TG_CHECK(d->res_mode >= 0 && d->res_mode <= 2, "%s: res_mode=%d", who, d->res_mode);
    TG_CHECK(d->res_mode != 1 || d->Cin == d->Cout, "%s: identity residual needs Cin == Cout", who);
    TG_CHECK(d->res_mode != 2 || (d->wd && d->bd), "%s: convolutional residual without weights", who);
    TG_CHECK(al4(d->x) && al16(d->E) && (!d->xpart || al16(d->xpart)), "%s: x must be 4-byte, E and xpart 16-byte aligned", who);
    a->N = d->N; a->Cin = d->Cin; a->Cout = d->Cout; a->T = d->T; a->V = d->V; a->S = d->S; a->R = d->R; a->res_mode = d->res_mode;
    a->x = d->x; a->w12 = d->w12; a->b12 = d->b12; a->w4 = d->w4; a->b4 = d->b4; a->A = d->A; a->alpha = d->alpha;
    a->w3 = d->w3; a->b3 = d->b3; a->sy = d->sy; a->ty = d->ty; a->wd = d->wd; a->bd = d->bd;
    a->E = d->E; a->sum = d->sum; a->diff = d->diff; a->xpart = d->xpart;
    a->vec12 = d->Cin % 16 == 0 && al16(d->w12);
    a->vec3 = d->Cin % 16 == 0 && al16(d->w3);
    a->vecd = d->res_mode == 2 && d->Cin % 16 == 0 && al16(d->wd);
    a->vec4 = d->R % 16 == 0 && al16(d->w4);
    a->ntp = 4;
    a->kc = FG_KC;
    return 0;
}

#define FG_LAUNCH_CASE(p) case p: tg_launch_lds<FG_KERNEL<p>>(FG_LDS_MAX, grid, dim3(FG_NT), lds, (hipStream_t)stream, a); break;

int fg_e_launch(const tamgcn_f2_gcn_desc* d, void* stream, const char* who) {
    FgGcnArgs a;
    if (fg_fill(d, &a, who)) return -1;
    a.ntp = fg_e_ntp(d->V, d->Cin, d->R);
    const size_t lds = fg_e_lds(d->V, d->Cin, d->R, a.ntp);
    TG_CHECK(lds <= FG_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(d->S * (d->Cout / 16), d->N);
#define FG_KERNEL f2g_e_kernel
    switch (fg_vp(d->V)) { FG_PITCHES(FG_LAUNCH_CASE) }
#undef FG_KERNEL
    tamgcn_note_kernel("f2g_e_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int fg_gcn_launch(const tamgcn_f2_gcn_desc* d, void* stream, const char* who) {
    FgGcnArgs a;
    if (fg_fill(d, &a, who)) return -1;
    TG_CHECK(d->sum && d->diff && al16(d->sum) && al16(d->diff), "%s: null or misaligned output", who);
    a.kc = fg_gcn_kc(d->V, d->Cin);
    const size_t lds = fg_gcn_lds(d->V, d->Cin, a.kc);
    TG_CHECK(lds <= FG_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(ceil_div(d->T, FG_BT) * (d->Cout / FG_CT), d->N);
#define FG_KERNEL f2g_gcn_kernel
    switch (fg_vp(d->V)) { FG_PITCHES(FG_LAUNCH_CASE) }
#undef FG_KERNEL
    tamgcn_note_kernel("f2g_gcn_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int fg_gemm_launch(const tamgcn_f2_gemm_desc* d, void* stream, const char* who) {
    if (fg_pick(d, who)) return -1;
    TG_CHECK(d->x && d->w && d->b && d->out, "%s: null pointer", who);
    TG_CHECK(d->N > 0 && d->T > 0 && d->K > 0 && d->K <= 256 && d->M > 0 && d->M % 16 == 0,
             "%s: bad shape N=%d T=%d K=%d M=%d (K <= 256, M %% 16 == 0)", who, d->N, d->T, d->K, d->M);
    TG_CHECK(d->mode == 0 || d->mode == 1, "%s: mode=%d", who, d->mode);
    TG_CHECK(d->mode != 0 || d->add, "%s: mode 0 needs the addend", who);
    TG_CHECK(al16(d->x) && al16(d->out) && (!d->add || al16(d->add)), "%s: activations must be 16-byte aligned", who);
    FgGemmArgs a;
    a.N = d->N; a.K = d->K; a.M = d->M; a.T = d->T; a.V = d->V; a.mode = d->mode; a.relu_rows = d->relu_rows;
    a.vec = d->K % 16 == 0 && al16(d->w);
    a.x = d->x; a.w = d->w; a.b = d->b; a.add = d->add; a.out = d->out;
    const size_t lds = fg_gemm_lds(d->V, d->K);
    TG_CHECK(lds <= FG_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(ceil_div(d->T, FG_BT) * (d->M / 16), d->N);
#define FG_KERNEL f2g_gemm_kernel
    switch (fg_vp(d->V)) { FG_PITCHES(FG_LAUNCH_CASE) }
#undef FG_KERNEL
    tamgcn_note_kernel("f2g_gemm_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int fg_tcn_launch(const tamgcn_f2_tcn_desc* d, void* stream, const char* who) {
    if (fg_pick(d, who)) return -1;
    TG_CHECK(d->h && d->out && d->sp && d->tp, "%s: null pointer", who);
    TG_CHECK(d->N > 0 && d->T > 0 && d->Cout > 0 && d->Cout % 16 == 0 && d->stride >= 1 && d->stride <= 2,
             "%s: bad shape N=%d T=%d Cout=%d stride=%d", who, d->N, d->T, d->Cout, d->stride);
    TG_CHECK(d->nb >= 1 && d->nb <= 4 && d->Cb > 0 && d->Cb % 16 == 0 && d->Cb <= 64 && (d->nb + 2) * d->Cb == d->Cout,
             "%s: nb=%d Cb=%d Cout=%d (Cb %% 16 == 0, Cb <= 64, (nb + 2) Cb == Cout)", who, d->nb, d->Cb, d->Cout);
    TG_CHECK(d->ks >= 1 && d->ks % 2 == 1, "%s: kernel size %d", who, d->ks);
    for (int b = 0; b < d->nb; ++b) {
        TG_CHECK(d->wt[b] && d->bt[b] && d->dil[b] >= 1, "%s: branch %d: null weights or dilation %d", who, b, d->dil[b]);
        TG_CHECK((FG_BT - 1) * d->stride + (d->ks - 1) * d->dil[b] + 1 <= FG_HF, "%s: branch %d: halo of k=%d dilation %d stride %d exceeds %d frames",
                 who, b, d->ks, d->dil[b], d->stride, FG_HF);
    }
    TG_CHECK(d->res_mode >= 0 && d->res_mode <= 2, "%s: res_mode=%d", who, d->res_mode);
    TG_CHECK(d->res_mode == 0 || d->x, "%s: residual without the block input", who);
    TG_CHECK(d->res_mode != 1 || (d->Cin == d->Cout && d->stride == 1), "%s: identity residual needs Cin == Cout, stride 1", who);
    TG_CHECK(d->res_mode != 2 || (d->wr && d->br && d->Cin > 0 && d->Cin <= 256), "%s: convolutional residual: weights / Cin=%d", who, d->Cin);
    TG_CHECK(al16(d->h) && al4(d->out) && (!d->x || al4(d->x)) && (!d->xpart || al16(d->xpart)),
             "%s: h and xpart must be 16-byte, x and out 4-byte aligned", who);
    FgTcnArgs a;
    a.N = d->N; a.Cin = d->Cin; a.Cout = d->Cout; a.T = d->T; a.V = d->V; a.stride = d->stride; a.T2 = (d->T - 1) / d->stride + 1;
    a.Cb = d->Cb; a.nb = d->nb; a.ks = d->ks; a.res_mode = d->res_mode;
    bool vt = (d->Cb * d->ks) % 16 == 0;
    for (int b = 0; b < 4; ++b) {
        a.dil[b] = b < d->nb ? d->dil[b] : 1;
        a.wt[b] = b < d->nb ? d->wt[b] : nullptr;
        a.bt[b] = b < d->nb ? d->bt[b] : nullptr;
        if (b < d->nb) vt = vt && al16(d->wt[b]);
    }
    a.vect = vt;
    a.vecr = d->res_mode == 2 && d->Cin % 16 == 0 && al16(d->wr);
    a.h = d->h; a.sp = d->sp; a.tp = d->tp; a.x = d->x; a.wr = d->wr; a.br = d->br; a.out = d->out; a.xpart = d->xpart;
    const size_t lds = fg_tcn_lds(d->V, d->Cin, d->Cb, d->res_mode);
    TG_CHECK(lds <= FG_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(ceil_div(a.T2, FG_BT) * (d->Cout / 16), d->N);
#define FG_KERNEL f2g_tcn_kernel
    switch (fg_vp(d->V)) { FG_PITCHES(FG_LAUNCH_CASE) }
#undef FG_KERNEL
    tamgcn_note_kernel("f2g_tcn_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" int tamgcn_f2g_supported(int V) { return fg_served(V) ? 1 : 0; }

// The largest dynamic-LDS request of a stage (0 e | 1 gcn | 2 gemm | 3 tcn) at joint count V in bytes, -1 for a geometry the
// entry points refuse.  c: Cin (e, gcn; tcn: the residual conv's, the largest request being res_mode 2's) | K (gemm);
// r: R (e) | Cb (tcn) | ignored (gcn, gemm).
extern "C" int tamgcn_f2g_lds_bytes(int stage, int V, int c, int r) {
    if (!fg_served(V) || c < 1 || c > 256) return -1;
    size_t lds;
    switch (stage) {
        case 0:
            if (r < 1 || r > 32) return -1;
            lds = fg_e_lds(V, c, r, fg_e_ntp(V, c, r));
            break;
        case 1: lds = fg_gcn_lds(V, c, fg_gcn_kc(V, c)); break;
        case 2: lds = fg_gemm_lds(V, c); break;
        case 3: {
            if (r < 16 || r > 64 || r % 16) return -1;
            const size_t l2 = fg_tcn_lds(V, c, r, 2), l0 = fg_tcn_lds(V, c, r, 0);
            lds = l2 > l0 ? l2 : l0;
            break;
        }
        default: return -1;
    }
    return lds <= FG_LDS_MAX ? (int)lds : -1;
}

extern "C" int tamgcn_f2g_e(const tamgcn_f2_gcn_desc* d, void* stream) { return fg_e_launch(d, stream, "tamgcn_f2g_e"); }
extern "C" int tamgcn_f2g_gcn(const tamgcn_f2_gcn_desc* d, void* stream) { return fg_gcn_launch(d, stream, "tamgcn_f2g_gcn"); }
extern "C" int tamgcn_f2g_gemm(const tamgcn_f2_gemm_desc* d, void* stream) { return fg_gemm_launch(d, stream, "tamgcn_f2g_gemm"); }
extern "C" int tamgcn_f2g_tcn(const tamgcn_f2_tcn_desc* d, void* stream) { return fg_tcn_launch(d, stream, "tamgcn_f2g_tcn"); }
