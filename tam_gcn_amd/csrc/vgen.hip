// CTRGC for ANY skeleton of 2 <= V <= 32 joints: the kernels of the V = 25 route (ctrgc.hip's E builder, the three streaming
// kernels, ctrgc_de.hip's register-staged tail) with V as a kernel ARGUMENT.  Same arithmetic, same output tensors, same
// partial-sum layouts, so the ops layer's fixed-order reductions serve both.  The streaming kernels are not a copy:
// ctrgc_stream_body.h holds their bodies once, ctrgc_tiled.hip instantiates them with the compile-time policy TlGeo<V> and this
// file with the run-time policy VgGeo<VP>, and at V = 20, 25, 32 the two give the same words (tests/test_gpu_vgen_routes.py).
//
//   vgen_E_kernel               E[n,s,c,u,v] = alpha (W4_s tanh(p_u - q_v) + b4_s)[c] + A_s[u,v]   workgroup = (n, s), D in LDS
//   vgen_agg_fwd_kernel<VP,ST>  y[n,c,t,u]     = sum_s sum_v x3_s[n,c,t,v] E_s[n,c,u,v]  + moment partials   workgroup = (n, c)
//   vgen_agg_bwd_kernel<VP,ST>  dx3_s[n,c,t,v] = sum_u dy[n,c,t,u] E_s[n,c,u,v]          + db3 partials
//   vgen_de_acc_kernel<VP,ST>   dE_s[n,c,u,v]  = sum_t dy[n,c,t,u] x3_s[n,c,t,v]
//   vgen_de_tail_kernel<RT>     dE -> dA, dW4, db4, dalpha, dp, dq                                  workgroup = (n, s, channel group)
//
// What is a template argument is only what sizes a register array: VP, the joints of the LDS images (V rounded up to 16: 16 or
// 32), the subset count ST and the tail's R tiling.  The joint pads of every LDS image are zero, the contraction over joints runs
// (V + 3) / 4 MFMA steps, and nothing of a pad ever reaches global memory.
//
// Rows of V floats are only dword-aligned once T * V % 4 != 0; the streaming kernels read them in 16-byte pieces all the same
// (full rate on gfx950) and the last piece of a chunk may reach <= 12 bytes past it: the ops' allocator keeps that slack behind
// every tensor, and every float past the chunk's valid run is replaced by zero before it reaches LDS.
//
// VP = 16 has ONE joint tile: a 32-frame chunk is two output tiles, so waves 0 and 1 carry the aggregation's MFMAs (all four
// still stream the operands, and these kernels are HBM-bound); in the dE accumulation wave s owns subset s.
//
// The tail keeps D = tanh(p_u - q_v) of every (u, v) in LDS (R * V * V floats: 131 KB at V = 32, R = 32), which leaves no room
// for a 16-channel dE chunk of all V * V columns at the large end.  So the chunk is staged in column windows of W columns (W a
// multiple of 16 chosen by the host from what D leaves free; one window wherever it fits, which is every V <= 25).
#include "ctrgc_stream_body.h"

namespace {

constexpr int VG_LDS_MAX = 160 * 1024 - 256;   // dynamic LDS a workgroup may ask for (static arrays of the kernels on top)

__host__ __device__ constexpr int vg_pitch16(int n) { return ((n + 13) & ~15) + 2; }   // smallest p >= n with p % 16 == 2

// ---------------------------------------------------------------------------------------------------------------
// E for every channel of one (sample, subset)
// ---------------------------------------------------------------------------------------------------------------
struct VgEArgs {
    int N, Cout, S, R, V;
    const float* pq; const float* w4; const float* b4; const float* A; const float* alpha;
    float* E;
};

__global__ __launch_bounds__(512) void vgen_E_kernel(const VgEArgs a) {
    constexpr int NT = 512, NW = 8, NIT = 8;          // <= 64 column tiles of 16 (V * V <= 1024) over 8 waves
    const int V = a.V, VV = V * V, NTILE = (VV + 15) / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ds = smem;                         // [R][VV]
    float* PQ = Ds + a.R * VV;                // [p|q][R][V]
    const int n = blockIdx.x / a.S, s = blockIdx.x - n * a.S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const long long NV = (long long)a.N * V;
    const float alpha = a.alpha[0];
    const float rcpV = 1.f / (float)V;
    {
        const int cnt = 2 * a.R * V;
        for (int e = tid; e < cnt; e += NT) {
            const int row = tg_rcp_div(e, rcpV), v = e - row * V;
            PQ[e] = a.pq[((long long)s * 2 * a.R + row) * NV + (long long)n * V + v];
        }
    }
    float Ar[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int col = (wave + it * NW) * 16 + j;
        Ar[it] = col < VV ? a.A[s * VV + col] : 0.f;
    }
    __syncthreads();
    for (int uv = tid; uv < VV; uv += NT) {
        const int u = tg_rcp_div(uv, rcpV), v = uv - u * V;
        for (int r = 0; r < a.R; ++r) Ds[r * VV + uv] = fast_tanh(PQ[r * V + u] - PQ[(a.R + r) * V + v]);
    }
    __syncthreads();
    float* Eg = a.E + ((long long)n * a.S + s) * a.Cout * VV;
    for (int c0 = 0; c0 < a.Cout; c0 += 16) {
        float aw[8], b4r[4];
#pragma unroll
        for (int k = 0; k < 8; ++k) aw[k] = (k * 4 + kq < a.R) ? a.w4[((long long)s * a.Cout + c0 + j) * a.R + k * 4 + kq] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) b4r[r] = a.b4[s * a.Cout + c0 + kq * 4 + r];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int ct = wave + it * NW;
            if (ct < NTILE) {                          // wave-uniform
                const int col = ct * 16 + j;
                const int colc = col < VV ? col : 0;
                f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k * 4 < a.R) acc = mfma16(aw[k], Ds[(k * 4 + kq) * VV + colc], acc);
                if (col < VV) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Eg[(long long)(c0 + kq * 4 + r) * VV + col] = alpha * (acc[r] + b4r[r]) + Ar[it];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// streaming kernels: the body fragments of ctrgc_stream_body.h under the run-time policy VgGeo<VP>, pasted into the kernels
// ---------------------------------------------------------------------------------------------------------------
template <int VP, int ST>
__global__ __launch_bounds__(256, 2) void vgen_agg_fwd_kernel(int N, int Cout, int T, int V, const float* __restrict__ x3, const float* __restrict__ E,
                                                              float* __restrict__ y, float* __restrict__ stats_part) {
    using G = VgGeo<VP>;
    const G g(V);
#include "ctrgc_stream_agg_fwd.h"
}

template <int VP, int ST>
__global__ __launch_bounds__(256, 2) void vgen_agg_bwd_kernel(int N, int Cout, int T, int V, const SrcDev dy, const float* __restrict__ E,
                                                              float* __restrict__ dx3, float* __restrict__ db3_part) {
    using G = VgGeo<VP>;
    const G g(V);
#include "ctrgc_stream_agg_bwd.h"
}

template <int VP, int ST>
__global__ __launch_bounds__(256) void vgen_de_acc_kernel(int N, int Cout, int T, int V, const float* __restrict__ x3, const SrcDev dy,
                                                          float* __restrict__ dE) {
    using G = VgGeo<VP>;
    const G g(V);
#include "ctrgc_stream_de_acc.h"
}

// ---------------------------------------------------------------------------------------------------------------
// dE -> dA, db4, dW4, dalpha, dp, dq     (one workgroup per (n, s, channel group))
// ---------------------------------------------------------------------------------------------------------------
struct VgTailArgs {
    int N, Cout, S, R, G, V, W;  // G channel groups; W columns of (u, v) per dE window, a multiple of 16
    const float* dE; const float* pq; const float* w4; const float* b4; const float* alpha;
    float* dA_part; float* dw4_part; float* db4_part; float* dalpha_part; float* dpq;
};

template <int RT>
__global__ __launch_bounds__(512) void vgen_de_tail_kernel(const VgTailArgs a) {
    constexpr int NT = 512, NW = 8, TPW = 8, NA = 2;  // <= 64 column tiles over 8 waves; <= 1024 columns over 512 threads
    const int V = a.V, VV = V * V, PD = vg_pitch16(VV), W = a.W, WP = W + 2, NCT = (VV + 15) / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red_alpha[NW];
    float* Ds = smem;                        // [R][PD]    D, later dS in place
    float* red = Ds + a.R * PD;              // [NW][16][RT*16]
    float* DEs = red + NW * 16 * RT * 16;    // [16][WP]   one window of a dE chunk; before the first chunk: p, q
    float* PQ = DEs;                         // [p | q][R][V]
    const int grp = blockIdx.x % a.G, ns = blockIdx.x / a.G;
    const int n = ns / a.S, s = ns - n * a.S;
    const int cg = a.Cout / a.G, cbeg = grp * cg, cend = cbeg + cg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mj = lane & 15, mkq = lane >> 4;
    const long long NV = (long long)a.N * V;
    const float alpha = a.alpha[0];
    const float rcpV = 1.f / (float)V;
    {   // p, q of this (n, subset) -> LDS, then D[r][uv] = tanh(p[r][u] - q[r][v]) from LDS
        const int cnt = 2 * a.R * V;
        for (int e = tid; e < cnt; e += NT) {
            const int row = tg_rcp_div(e, rcpV), v = e - row * V;
            PQ[e] = a.pq[((long long)s * 2 * a.R + row) * NV + (long long)n * V + v];
        }
        __syncthreads();
        for (int uv = tid; uv < VV; uv += NT) {
            const int u = tg_rcp_div(uv, rcpV), v = uv - u * V;
            for (int r = 0; r < a.R; ++r) Ds[r * PD + uv] = fast_tanh(PQ[r * V + u] - PQ[(a.R + r) * V + v]);
        }
    }
    f32x4 accG[TPW][RT];
#pragma unroll
    for (int q = 0; q < TPW; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) accG[q][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float accA[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) accA[i] = 0.f;
    float dalpha_acc = 0.f;
    const int sc = tid >> 5, sl = tid & 31;          // staging: channel, lane of 32 along the columns
    const int dbc = (tid >> 4) & 15, l16 = tid & 15; // db4 pass: channel, lane of 16 (threads 256.. shadow 0..255, no second write)

    for (int c0 = cbeg; c0 < cend; c0 += 16) {
        float aw[RT][4];                     // W4^T fragment of this chunk: A[i = r][k = c]
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4)
                aw[rt][k4] = (rt * 16 + mj < a.R) ? a.w4[((long long)s * a.Cout + c0 + k4 * 4 + mkq) * a.R + rt * 16 + mj] : 0.f;
        const float* dEg = a.dE + (((long long)n * a.S + s) * a.Cout + c0) * VV;
        float db = 0.f;
        f32x4 accW[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) accW[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int w0 = 0; w0 < VV; w0 += W) {
            __syncthreads();                 // previous window (and the D fill, and the previous chunk's flush) done
            for (int col = sl; col < W; col += 32)           // columns past V * V are zero in the image
                DEs[sc * WP + col] = w0 + col < VV ? dEg[(long long)sc * VV + w0 + col] : 0.f;
            __syncthreads();
            // dG[r][uv] += sum_c W4[c][r] dE[c][uv]
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                const int ct = wave + q * NW, lc0 = ct * 16 - w0;
                if (ct < NCT && lc0 >= 0 && lc0 < W) {       // wave-uniform
#pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4) {
                        const float b = DEs[(k4 * 4 + mkq) * WP + lc0 + mj];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) accG[q][rt] = mfma16(aw[rt][k4], b, accG[q][rt]);
                    }
                }
            }
            // dA partial: sum over channels
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int lc = tid + i * NT - w0;
                if (lc >= 0 && lc < W && lc + w0 < VV) {
                    float t = 0.f;
#pragma unroll
                    for (int cl = 0; cl < 16; ++cl) t += DEs[cl * WP + lc];
                    accA[i] += t;
                }
            }
            // db4raw[c] = sum_uv dE[c][uv]
            for (int col = l16; col < W; col += 16) db += DEs[dbc * WP + col];
            // dW4raw[c][r] = sum_uv dE[c][uv] D[r][uv]: the window's columns split over the waves
            for (int st = wave; st < W / 4; st += NW) {
                const int k = st * 4 + mkq;
                const bool kok = w0 + k < VV;
                const float av = DEs[mj * WP + k];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int r = rt * 16 + mj;
                    const float bv = (kok && r < a.R) ? Ds[r * PD + w0 + k] : 0.f;
                    accW[rt] = mfma16(av, bv, accW[rt]);
                }
            }
        }
        db = wave_sum16(db);
        if (l16 == 0 && tid < 256) {
            a.db4_part[((long long)n * a.S + s) * a.Cout + c0 + dbc] = alpha * db;
            dalpha_acc = fmaf(a.b4[s * a.Cout + c0 + dbc], db, dalpha_acc);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) red[(wave * 16 + mkq * 4 + rr) * (RT * 16) + rt * 16 + mj] = accW[rt][rr];
        __syncthreads();
        for (int e = tid; e < 16 * RT * 16; e += NT) {
            const int cl = e / (RT * 16), r = e - cl * (RT * 16);
            if (r < a.R) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) t += red[(w * 16 + cl) * (RT * 16) + r];
                const long long wi = ((long long)s * a.Cout + c0 + cl) * a.R + r;
                a.dw4_part[(long long)n * a.S * a.Cout * a.R + wi] = alpha * t;
                dalpha_acc = fmaf(a.w4[wi], t, dalpha_acc);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int uv = tid + i * NT;
        if (uv < VV) a.dA_part[(((long long)n * a.G + grp) * a.S + s) * VV + uv] = accA[i];
    }
    __syncthreads();                         // every wave is done reading D
    // dS[r][uv] = alpha * dG * (1 - D^2), in place over D
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
        const int ct = wave + q * NW;
        const int col = ct * 16 + mj;
        if (ct < NCT && col < VV) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int r = rt * 16 + mkq * 4 + rr;
                    if (r < a.R) {
                        const float d = Ds[r * PD + col];
                        Ds[r * PD + col] = alpha * accG[q][rt][rr] * (1.f - d * d);
                    }
                }
        }
    }
    __syncthreads();
    // dp[r][u] = sum_v dS[r][u][v];  dq[r][v] = -sum_u dS[r][u][v]
    for (int e = tid; e < a.R * V * 2; e += NT) {
        const int which = e >= a.R * V;
        const int rem = e - which * a.R * V;
        const int r = tg_rcp_div(rem, rcpV), k = rem - r * V;
        float t = 0.f;
        if (which == 0) {
            for (int v = 0; v < V; ++v) t += Ds[r * PD + k * V + v];
        } else {
            for (int u = 0; u < V; ++u) t -= Ds[r * PD + u * V + k];
        }
        a.dpq[(((long long)grp * a.S * 2 + s * 2 + which) * a.R + r) * NV + (long long)n * V + k] = t;
    }
    dalpha_acc = wave_sum64(dalpha_acc);
    if (lane == 0) red_alpha[wave] = dalpha_acc;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < NW; ++w) t += red_alpha[w];
        a.dalpha_part[(n * a.S + s) * a.G + grp] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LDS requests
// ---------------------------------------------------------------------------------------------------------------
int vg_vp(int V) { return V <= 16 ? 16 : 32; }
size_t vg_e_lds(int V, int R) { return sizeof(float) * ((size_t)R * V * V + 2 * (size_t)R * V); }
// the tail's window: as many columns as D and the partial tiles leave room for, at most all of them; 0: does not fit
int vg_tail_window(int V, int R) {
    const int VV = V * V, RT = R <= 16 ? 1 : 2;
    const long long avail = VG_LDS_MAX / (long long)sizeof(float) - (long long)R * vg_pitch16(VV) - 8 * 16 * RT * 16;
    if (avail < 2LL * R * V || avail < 16 * 18) return 0;
    const int wmax = (int)((avail / 16 - 2) / 16) * 16, wfull = (VV + 15) & ~15;
    return wmax < wfull ? wmax : wfull;
}
size_t vg_tail_lds(int V, int R) {
    const int VV = V * V, RT = R <= 16 ? 1 : 2, W = vg_tail_window(V, R);
    const size_t x = (size_t)16 * (W + 2), pq = 2 * (size_t)R * V;
    return sizeof(float) * ((size_t)R * vg_pitch16(VV) + 8 * 16 * RT * 16 + (x > pq ? x : pq));
}

bool vg_v_ok(int V) { return V >= 2 && V <= 32; }
bool vg_r_ok(int R) { return R >= 4 && R <= 32 && R % 4 == 0; }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
extern "C" int tamgcn_vgen_supported(int V) { return vg_v_ok(V) ? 1 : 0; }

// largest dynamic-LDS request of the family for (S, V, R); -1 outside its range
extern "C" int tamgcn_vgen_lds_bytes(int S, int V, int R) {
    if (!vg_v_ok(V) || !(S == 1 || S == 3) || !vg_r_ok(R) || !vg_tail_window(V, R)) return -1;
    size_t m = vg_e_lds(V, R);
    const size_t o[4] = {stream_agg_lds(vg_vp(V), S, false), stream_agg_lds(vg_vp(V), S, true), stream_de_lds(vg_vp(V), S), vg_tail_lds(V, R)};
    for (size_t x : o) m = x > m ? x : m;
    return (int)m;
}

// checks shared by the per-(n, s) kernels (E builder, tail)
static int vgen_ns_check(const tamgcn_ctrgc_desc* d, const char* who) {
    if (!vg_v_ok(d->V)) { tamgcn_set_error("%s: V=%d (the run-time-V CTRGC kernels take 2 <= V <= 32)", who, d->V); return -1; }
    if (!(d->S == 1 || d->S == 3)) { tamgcn_set_error("%s: S=%d (1 or 3 subsets)", who, d->S); return -1; }
    if (!(d->N > 0 && d->Cout > 0 && d->Cout % 16 == 0)) { tamgcn_set_error("%s: bad shape N=%d Cout=%d (Cout a multiple of 16)", who, d->N, d->Cout); return -1; }
    if (!vg_r_ok(d->R)) { tamgcn_set_error("%s: R=%d outside 4..32 (multiples of 4)", who, d->R); return -1; }
    if ((long long)d->N * d->S * 64 >= (1LL << 31)) { tamgcn_set_error("%s: N*S too large for the grid", who); return -1; }
    if ((long long)d->S * d->Cout * d->V * d->V >= (1LL << 31) || (long long)d->S * d->Cout * d->R >= (1LL << 31) ||
        (long long)d->N * d->V >= (1LL << 31) / (2 * d->S * d->R)) {
        tamgcn_set_error("%s: a per-sample block of >= 2^31 elements", who); return -1;
    }
    return 0;
}

// checks shared by the per-(n, c) streaming kernels
static int vgen_stream_check(const tamgcn_ctrgc_desc* d, const char* who) {
    if (!vg_v_ok(d->V)) { tamgcn_set_error("%s: V=%d (the run-time-V CTRGC kernels take 2 <= V <= 32)", who, d->V); return -1; }
    if (!(d->S == 1 || d->S == 3)) { tamgcn_set_error("%s: S=%d (1 or 3 subsets)", who, d->S); return -1; }
    if (!(d->N > 0 && d->Cout > 0 && d->T > 0 && d->Cout % 16 == 0)) {
        tamgcn_set_error("%s: bad dims N=%d Cout=%d T=%d (Cout a multiple of 16)", who, d->N, d->Cout, d->T); return -1;
    }
    if ((long long)d->N * d->Cout >= (1LL << 31)) { tamgcn_set_error("%s: N*Cout too large for the grid", who); return -1; }
    if ((long long)d->T * d->V >= (1LL << 31) - 4 * STREAM_BT * 32) { tamgcn_set_error("%s: T*V=%lld >= 2^31", who, (long long)d->T * d->V); return -1; }
    return 0;
}

extern "C" int tamgcn_vgen_build_e(const tamgcn_ctrgc_desc* d, float* E, void* stream) {
    TG_CHECK(d && E && d->pq && d->w4 && d->b4 && d->A && d->alpha, "tamgcn_vgen_build_e: null pointer");
    if (vgen_ns_check(d, "tamgcn_vgen_build_e")) return -1;
    VgEArgs a;
    a.N = d->N; a.Cout = d->Cout; a.S = d->S; a.R = d->R; a.V = d->V;
    a.pq = d->pq; a.w4 = d->w4; a.b4 = d->b4; a.A = d->A; a.alpha = d->alpha; a.E = E;
    const size_t lds = vg_e_lds(d->V, d->R);
    TG_CHECK(lds <= (size_t)VG_LDS_MAX, "tamgcn_vgen_build_e: %zu bytes of LDS", lds);
    tg_launch_lds<vgen_E_kernel>(VG_LDS_MAX, dim3(d->N * d->S), dim3(512), lds, (hipStream_t)stream, a);
    tamgcn_note_kernel("vgen_E_kernel");
    TG_LAUNCH_CHECK("tamgcn_vgen_build_e");
    return 0;
}

#define VG_CASE(KERNEL, VP_, SS_, LDS_, ...)                                                                          \
    if (vg_vp(d->V) == VP_ && d->S == SS_) {                                                                          \
        const size_t lds_ = (LDS_);   /* fixed per instantiation */                                                   \
        tg_launch_lds<KERNEL<VP_, SS_>>(lds_, dim3((unsigned)(d->N * d->Cout)), dim3(256), lds_, (hipStream_t)stream, __VA_ARGS__); \
        tamgcn_note_kernel(#KERNEL "<%d, %d>", VP_, SS_);                                                             \
        launched = true;                                                                                              \
    }

extern "C" int tamgcn_vgen_agg_fwd(const tamgcn_ctrgc_desc* d, const float* x3, const float* E, float* y, float* stats_part, void* stream) {
    TG_CHECK(d && x3 && E && y, "tamgcn_vgen_agg_fwd: null pointer");
    if (vgen_stream_check(d, "tamgcn_vgen_agg_fwd")) return -1;
    bool launched = false;
    VG_CASE(vgen_agg_fwd_kernel, 32, 3, stream_agg_lds(32, 3, false), d->N, d->Cout, d->T, d->V, x3, E, y, stats_part)
    else VG_CASE(vgen_agg_fwd_kernel, 32, 1, stream_agg_lds(32, 1, false), d->N, d->Cout, d->T, d->V, x3, E, y, stats_part)
    else VG_CASE(vgen_agg_fwd_kernel, 16, 3, stream_agg_lds(16, 3, false), d->N, d->Cout, d->T, d->V, x3, E, y, stats_part)
    else VG_CASE(vgen_agg_fwd_kernel, 16, 1, stream_agg_lds(16, 1, false), d->N, d->Cout, d->T, d->V, x3, E, y, stats_part)
    TG_CHECK(launched, "tamgcn_vgen_agg_fwd: no instantiation for S=%d V=%d", d->S, d->V);
    TG_LAUNCH_CHECK("tamgcn_vgen_agg_fwd");
    return 0;
}

extern "C" int tamgcn_vgen_agg_bwd(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* E, float* dx3, float* db3_part, void* stream) {
    TG_CHECK(d && dy && dy->x1 && E && dx3, "tamgcn_vgen_agg_bwd: null pointer");
    if (vgen_stream_check(d, "tamgcn_vgen_agg_bwd")) return -1;
    TG_CHECK(dy->coff >= 0 && dy->ctot >= dy->coff + d->Cout, "tamgcn_vgen_agg_bwd: dy has %d channels from %d, need %d", dy->ctot, dy->coff, d->Cout);
    const SrcDev dys = make_src(*dy);
    bool launched = false;
    VG_CASE(vgen_agg_bwd_kernel, 32, 3, stream_agg_lds(32, 3, true), d->N, d->Cout, d->T, d->V, dys, E, dx3, db3_part)
    else VG_CASE(vgen_agg_bwd_kernel, 32, 1, stream_agg_lds(32, 1, true), d->N, d->Cout, d->T, d->V, dys, E, dx3, db3_part)
    else VG_CASE(vgen_agg_bwd_kernel, 16, 3, stream_agg_lds(16, 3, true), d->N, d->Cout, d->T, d->V, dys, E, dx3, db3_part)
    else VG_CASE(vgen_agg_bwd_kernel, 16, 1, stream_agg_lds(16, 1, true), d->N, d->Cout, d->T, d->V, dys, E, dx3, db3_part)
    TG_CHECK(launched, "tamgcn_vgen_agg_bwd: no instantiation for S=%d V=%d", d->S, d->V);
    TG_LAUNCH_CHECK("tamgcn_vgen_agg_bwd");
    return 0;
}

extern "C" int tamgcn_vgen_de_acc(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* x3, float* dE, void* stream) {
    TG_CHECK(d && dy && dy->x1 && x3 && dE, "tamgcn_vgen_de_acc: null pointer");
    if (vgen_stream_check(d, "tamgcn_vgen_de_acc")) return -1;
    TG_CHECK(dy->coff >= 0 && dy->ctot >= dy->coff + d->Cout, "tamgcn_vgen_de_acc: dy has %d channels from %d, need %d", dy->ctot, dy->coff, d->Cout);
    const SrcDev dys = make_src(*dy);
    bool launched = false;
    VG_CASE(vgen_de_acc_kernel, 32, 3, stream_de_lds(32, 3), d->N, d->Cout, d->T, d->V, x3, dys, dE)
    else VG_CASE(vgen_de_acc_kernel, 32, 1, stream_de_lds(32, 1), d->N, d->Cout, d->T, d->V, x3, dys, dE)
    else VG_CASE(vgen_de_acc_kernel, 16, 3, stream_de_lds(16, 3), d->N, d->Cout, d->T, d->V, x3, dys, dE)
    else VG_CASE(vgen_de_acc_kernel, 16, 1, stream_de_lds(16, 1), d->N, d->Cout, d->T, d->V, x3, dys, dE)
    TG_CHECK(launched, "tamgcn_vgen_de_acc: no instantiation for S=%d V=%d", d->S, d->V);
    TG_LAUNCH_CHECK("tamgcn_vgen_de_acc");
    return 0;
}

#define VG_TAIL_CASE(RT_)                                                                                             \
    if (rt == RT_) {                                                                                                  \
        tg_launch_lds<vgen_de_tail_kernel<RT_>>(VG_LDS_MAX, dim3(d->N * d->S * groups), dim3(512), lds, (hipStream_t)stream, a); \
        tamgcn_note_kernel("vgen_de_tail_kernel<%d>", RT_);                                                           \
        launched = true;                                                                                              \
    }

extern "C" int tamgcn_vgen_de_tail(const tamgcn_ctrgc_desc* d, const float* dE, float* dA_part, float* dw4_part, float* db4_part,
                                   float* dalpha_part, float* dpq, int groups, void* stream) {
    TG_CHECK(d && dE && dA_part && dw4_part && db4_part && dalpha_part && dpq, "tamgcn_vgen_de_tail: null pointer");
    TG_CHECK(d->pq && d->w4 && d->b4 && d->alpha, "tamgcn_vgen_de_tail: null parameter pointer");
    if (vgen_ns_check(d, "tamgcn_vgen_de_tail")) return -1;
    TG_CHECK(groups >= 1 && d->Cout % (16 * groups) == 0, "tamgcn_vgen_de_tail: groups=%d must divide Cout/16=%d", groups, d->Cout / 16);
    TG_CHECK((long long)d->N * d->S * groups < (1LL << 31), "tamgcn_vgen_de_tail: N*S*groups too large for the grid");
    VgTailArgs a;
    a.N = d->N; a.Cout = d->Cout; a.S = d->S; a.R = d->R; a.G = groups; a.V = d->V; a.W = vg_tail_window(d->V, d->R);
    TG_CHECK(a.W >= 16, "tamgcn_vgen_de_tail: no LDS left for a dE window at V=%d R=%d", d->V, d->R);
    a.dE = dE; a.pq = d->pq; a.w4 = d->w4; a.b4 = d->b4; a.alpha = d->alpha;
    a.dA_part = dA_part; a.dw4_part = dw4_part; a.db4_part = db4_part; a.dalpha_part = dalpha_part; a.dpq = dpq;
    const int rt = d->R <= 16 ? 1 : 2;
    const size_t lds = vg_tail_lds(d->V, d->R);
    bool launched = false;
    VG_TAIL_CASE(1) else VG_TAIL_CASE(2)
    TG_CHECK(launched, "tamgcn_vgen_de_tail: no instantiation");
    TG_LAUNCH_CHECK("tamgcn_vgen_de_tail");
    return 0;
}
