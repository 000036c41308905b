// ===========================================================================
// weight gradient:  dW[m][k][tap] = sum_{n,t,v} gy(n,m,t,v) * x(n,k,t*stride + tap*dil - pad, v)
//
// An "NT" GEMM whose contraction index p = (n,t,v) is the contiguous axis of BOTH operands.
// A workgroup owns a (2*WMT*16) x (2*WKT*16) tile of dW for all taps (2x2 waves, one
// sub-tile per wave, accumulators never leave registers), walks its share of the samples in
// chunks of BT frames, stages both operand tiles in LDS with 16-byte global loads (rows are
// contiguous along t*V+v), the BatchNorm(-backward)-apply prologue fused into the fill, and
// feeds v_mfma_f32_16x16x4_f32 with column reads that are bank-conflict free for pitches
// == 2 (mod 4).  Partial slabs per n-split are summed by reduce_sum (deterministic).
// ===========================================================================
#include "common.h"

namespace {

struct WgradArgs {
    SrcDev gy, src;
    int N, M, K, T_in, T_out, V, dil, stride, pad;
    float* part; int nsplit;
    int BT, TIN;      // frames per staged chunk (gy side / x side)
    int PY, PX;       // LDS pitches
    int n_per;        // samples per split
    int KTG;          // LDS-DMA kernel: temporal taps (1 = 1x1), one window of the contraction axis per tap
};

__device__ __forceinline__ float wg_apply(float x1, float x2, float c1, float c2, float c0, int act) {
    float v = fmaf(c1, x1, fmaf(c2, x2, c0));
    return act == 1 ? fmaxf(v, 0.f) : v;
}

// fill rows [r0, r0+rows) x [0, len) of an LDS tile from channel-rows of `s`; frames outside
// [0, T) are zero.  f0 = first frame of the tile, V4 = V/4 (VEC) .
template <bool VEC>
__device__ __forceinline__ void wg_fill(float* tile, int pitch, const float* cf, int rows, int nvalid, int ch0,
                                        const SrcDev& s, long long nbase, long long cs, int T, int V, int f0, int frames) {
    const int tid = threadIdx.x;
    const int len = frames * V;
    if constexpr (VEC) {
        const int l4 = len >> 2;
        for (int e = tid; e < rows * l4; e += NTHREADS) {
            int r = e / l4, c4 = e - r * l4;
            int col = c4 << 2;
            int fr = f0 + col / V;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < nvalid && fr >= 0 && fr < T) {
                long long g = nbase + (long long)(ch0 + r) * cs + (long long)f0 * V + col;
                float4 a = *reinterpret_cast<const float4*>(s.x1 + g);
                float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s.x2) b = *reinterpret_cast<const float4*>(s.x2 + g);
                float c1 = cf[r], c2 = cf[rows + r], c0 = cf[2 * rows + r];
                o.x = wg_apply(a.x, b.x, c1, c2, c0, s.act); o.y = wg_apply(a.y, b.y, c1, c2, c0, s.act);
                o.z = wg_apply(a.z, b.z, c1, c2, c0, s.act); o.w = wg_apply(a.w, b.w, c1, c2, c0, s.act);
            }
            float2* d = reinterpret_cast<float2*>(tile + r * pitch + col);
            d[0] = make_float2(o.x, o.y);
            d[1] = make_float2(o.z, o.w);
        }
    } else {
        // V % 4 != 0 (NTU's 25 joints at stride 2): one float per step.  Round 4: the row / frame indices come from reciprocals
        // (two integer divisions per element were ~50 VALU instructions) and four steps' loads are requested together.
        const bool rcp_ok = len >= 4 && len <= 1024 && V >= 4 && rows * len < (1 << 20);
        const float rlen = 1.0f / (float)len, rV = 1.0f / (float)V;
        for (int e0 = tid; e0 < rows * len; e0 += 4 * NTHREADS) {
            float v1[4], v2[4]; int rr[4], cc[4]; bool ok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * NTHREADS;
                const bool in = e < rows * len;
                const int ee = in ? e : 0;
                const int r = rcp_ok ? tg_rcp_div(ee, rlen) : ee / len, col = ee - r * len;
                const int fr = f0 + (rcp_ok ? tg_rcp_div(col, rV) : col / V);
                rr[i] = r; cc[i] = col;
                ok[i] = in && r < nvalid && fr >= 0 && fr < T;
                const long long g = nbase + (long long)(ch0 + (ok[i] ? r : 0)) * cs + (long long)f0 * V + (ok[i] ? col : 0);
                v1[i] = ok[i] ? s.x1[g] : 0.f;
                v2[i] = (ok[i] && s.x2) ? s.x2[g] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * NTHREADS;
                if (e < rows * len) tile[rr[i] * pitch + cc[i]] = ok[i] ? wg_apply(v1[i], v2[i], cf[rr[i]], cf[rows + rr[i]], cf[2 * rows + rr[i]], s.act) : 0.f;
            }
        }
    }
}

constexpr int WG_NPF = 6;     // float4 prefetch slots per thread and operand (1x1 weight-gradient pipeline)

// PS ("p-split", M, K <= 16: the 16-channel temporal branches): the tile is ONE 16x16 MFMA tile; instead of tiling
// (M, K) 2x2 -- three of four waves would idle -- the four waves share it and split the chunk's frames, partial
// accumulators meet in LDS at the end.
template <int KT, int WMT, int WKT, bool VEC, bool PS = false>
__global__ __launch_bounds__(NTHREADS) void wgrad_kernel(const WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BMW = PS ? 16 : 2 * WMT * 16, BKW = PS ? 16 : 2 * WKT * 16;
    constexpr bool PF = VEC && (KT == 1 || PS);   // register-prefetch pipeline (host guarantees the slot bound)
    float* Ys = smem;                         // [BMW][PY]
    float* Xs = Ys + BMW * a.PY;              // [BKW][PX]
    float* cfY = Xs + BKW * a.PX;             // [3][BMW]
    float* cfX = cfY + 3 * BMW;               // [3][BKW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int wr = PS ? 0 : wave >> 1, wc = PS ? 0 : wave & 1;
    const int k0 = blockIdx.x * BKW, m0 = blockIdx.y * BMW, split = blockIdx.z;
    const int V = a.V, V4 = (V + 3) >> 2;
    // a split owns a contiguous range of the (sample, frame chunk) sequence: splits may be finer than samples
    const int cpt = (a.T_out + a.BT - 1) / a.BT;              // frame chunks per sample
    const int c_begin = split * a.n_per, c_end = min(a.N * cpt, c_begin + a.n_per);
    const int mvalid = min(BMW, a.M - m0), kvalid = min(BKW, a.K - k0);

    for (int e = tid; e < BMW; e += NTHREADS) {
        int ch = a.gy.coff + m0 + e;
        bool ok = e < mvalid && a.gy.coef;
        cfY[e] = ok ? a.gy.coef[ch] : 1.f;
        cfY[BMW + e] = (ok && a.gy.x2) ? a.gy.coef[a.gy.ctot + ch] : 0.f;
        cfY[2 * BMW + e] = ok ? a.gy.coef[2 * a.gy.ctot + ch] : 0.f;
    }
    for (int e = tid; e < BKW; e += NTHREADS) {
        int ch = a.src.coff + k0 + e;
        bool ok = e < kvalid && a.src.coef;
        cfX[e] = ok ? a.src.coef[ch] : 1.f;
        cfX[BKW + e] = (ok && a.src.x2) ? a.src.coef[a.src.ctot + ch] : 0.f;
        cfX[2 * BKW + e] = ok ? a.src.coef[2 * a.src.ctot + ch] : 0.f;
    }

    f32x4 acc[KT][WMT][WKT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int x = 0; x < WMT; ++x)
#pragma unroll
            for (int y = 0; y < WKT; ++y) acc[t][x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const long long gy_cs = (long long)a.T_out * V, x_cs = (long long)a.T_in * V;
    const float* yrow = Ys + (wr * WMT * 16 + j) * a.PY;
    const float* xrow = Xs + (wc * WKT * 16 + j) * a.PX;

    // ---- prefetch descriptors (PF only): slot i of this thread -> (row, 4-column group) of each tile
    const int ly4 = (a.BT * V) >> 2, lx4 = (a.TIN * V) >> 2;
    int yr[PF ? WG_NPF : 1], yc[PF ? WG_NPF : 1], xr_[PF ? WG_NPF : 1], xc[PF ? WG_NPF : 1];
    // frame (inside the chunk) of a slot's first element and how many of its 4 elements lie in that frame: for V % 4 != 0
    // (rows only dword aligned -- gfx950 takes such 16-byte loads at full rate) a slot may straddle two frames
    int yf[PF ? WG_NPF : 1], ycn[PF ? WG_NPF : 1], xf[PF ? WG_NPF : 1], xcn[PF ? WG_NPF : 1];
    float4 y1[PF ? WG_NPF : 1], y2[PF ? WG_NPF : 1], x1[PF ? WG_NPF : 1], x2[PF ? WG_NPF : 1];
    if constexpr (PF) {
#pragma unroll
        for (int i = 0; i < WG_NPF; ++i) {
            int e = tid + i * NTHREADS;
            int r = e / ly4; yr[i] = r < BMW ? r : -1; yc[i] = (e - r * ly4) << 2;
            r = e / lx4; xr_[i] = r < BKW ? r : -1; xc[i] = (e - r * lx4) << 2;
            yf[i] = yc[i] / V; ycn[i] = min(4, V - (yc[i] - yf[i] * V));
            xf[i] = xc[i] / V; xcn[i] = min(4, V - (xc[i] - xf[i] * V));
        }
    }
    const bool gy2 = a.gy.x2 != nullptr, sx2 = a.src.x2 != nullptr;
    // elements [0, cn) of a slot are valid iff va, elements [cn, 4) iff vb: a whole-slot 16-byte load when both hold,
    // element loads for a slot that is cut by the start or the end of the row (never touches memory outside the row)
    auto load_slot = [&](const float* p, int cn, bool va, bool vb) -> float4 {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (va && vb) o = *reinterpret_cast<const float4*>(p);
        else if (va || vb) {
            if (cn > 0 ? va : vb) o.x = p[0];
            if (cn > 1 ? va : vb) o.y = p[1];
            if (cn > 2 ? va : vb) o.z = p[2];
            if (cn > 3 ? va : vb) o.w = p[3];
        }
        return o;
    };
    auto prefetch = [&](int n, int t0) {
        if constexpr (PF) {
            const long long yb = (long long)n * a.gy.ctot * gy_cs + (long long)(a.gy.coff + m0) * gy_cs + (long long)t0 * V;
            const int f0 = t0 * a.stride - a.pad;
            const long long xb = (long long)n * a.src.ctot * x_cs + (long long)(a.src.coff + k0) * x_cs + (long long)f0 * V;
#pragma unroll
            for (int i = 0; i < WG_NPF; ++i) {
                y1[i] = make_float4(0.f, 0.f, 0.f, 0.f); y2[i] = y1[i]; x1[i] = y1[i]; x2[i] = y1[i];
                if (yr[i] >= 0 && yr[i] < mvalid) {
                    const int fa = t0 + yf[i], fb = fa + (ycn[i] < 4 ? 1 : 0);
                    const bool va = fa < a.T_out, vb = fb < a.T_out;
                    long long g = yb + (long long)yr[i] * gy_cs + yc[i];
                    y1[i] = load_slot(a.gy.x1 + g, ycn[i], va, vb);
                    if (gy2) y2[i] = load_slot(a.gy.x2 + g, ycn[i], va, vb);
                }
                if (xr_[i] >= 0 && xr_[i] < kvalid) {
                    const int fa = f0 + xf[i], fb = fa + (xcn[i] < 4 ? 1 : 0);
                    const bool va = fa >= 0 && fa < a.T_in, vb = fb >= 0 && fb < a.T_in;
                    long long g = xb + (long long)xr_[i] * x_cs + xc[i];
                    x1[i] = load_slot(a.src.x1 + g, xcn[i], va, vb);
                    if (sx2) x2[i] = load_slot(a.src.x2 + g, xcn[i], va, vb);
                }
            }
        }
    };
    auto commit = [&](int n, int t0) {        // prologue + LDS store of the prefetched chunk (zeros where invalid)
        if constexpr (PF) {
            const int f0 = t0 * a.stride - a.pad;
#pragma unroll
            for (int i = 0; i < WG_NPF; ++i) {
                if (yr[i] >= 0) {
                    const int r = yr[i];
                    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                    const int fa = t0 + yf[i], fb = fa + (ycn[i] < 4 ? 1 : 0);
                    const bool va = fa < a.T_out, vb = fb < a.T_out;
                    if (r < mvalid && (va || vb)) {
                        float c1 = cfY[r], c2 = cfY[BMW + r], c0 = cfY[2 * BMW + r];
                        o.x = wg_apply(y1[i].x, y2[i].x, c1, c2, c0, a.gy.act); o.y = wg_apply(y1[i].y, y2[i].y, c1, c2, c0, a.gy.act);
                        o.z = wg_apply(y1[i].z, y2[i].z, c1, c2, c0, a.gy.act); o.w = wg_apply(y1[i].w, y2[i].w, c1, c2, c0, a.gy.act);
                        if (!(va && vb)) {                        // a slot cut by the end of the row: padding is zero AFTER the prologue
                            const int cn = ycn[i];
                            if (!(cn > 0 ? va : vb)) o.x = 0.f;
                            if (!(cn > 1 ? va : vb)) o.y = 0.f;
                            if (!(cn > 2 ? va : vb)) o.z = 0.f;
                            if (!(cn > 3 ? va : vb)) o.w = 0.f;
                        }
                    }
                    float2* d = reinterpret_cast<float2*>(Ys + r * a.PY + yc[i]);
                    d[0] = make_float2(o.x, o.y); d[1] = make_float2(o.z, o.w);
                }
                if (xr_[i] >= 0) {
                    const int r = xr_[i];
                    const int fa = f0 + xf[i], fb = fa + (xcn[i] < 4 ? 1 : 0);
                    const bool va = fa >= 0 && fa < a.T_in, vb = fb >= 0 && fb < a.T_in;
                    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (r < kvalid && (va || vb)) {
                        float c1 = cfX[r], c2 = cfX[BKW + r], c0 = cfX[2 * BKW + r];
                        o.x = wg_apply(x1[i].x, x2[i].x, c1, c2, c0, a.src.act); o.y = wg_apply(x1[i].y, x2[i].y, c1, c2, c0, a.src.act);
                        o.z = wg_apply(x1[i].z, x2[i].z, c1, c2, c0, a.src.act); o.w = wg_apply(x1[i].w, x2[i].w, c1, c2, c0, a.src.act);
                        if (!(va && vb)) {
                            const int cn = xcn[i];
                            if (!(cn > 0 ? va : vb)) o.x = 0.f;
                            if (!(cn > 1 ? va : vb)) o.y = 0.f;
                            if (!(cn > 2 ? va : vb)) o.z = 0.f;
                            if (!(cn > 3 ? va : vb)) o.w = 0.f;
                        }
                    }
                    float2* d = reinterpret_cast<float2*>(Xs + r * a.PX + xc[i]);
                    d[0] = make_float2(o.x, o.y); d[1] = make_float2(o.z, o.w);
                }
            }
        }
    };

    __syncthreads();                          // coefficient tables visible
    if (c_begin < c_end) prefetch(c_begin / cpt, (c_begin % cpt) * a.BT);
    for (int ci = c_begin; ci < c_end; ++ci) {
        {
            const int n = ci / cpt, t0 = (ci - n * cpt) * a.BT;
            const int bt = min(a.BT, a.T_out - t0);
            const int tin = (bt - 1) * a.stride + (KT - 1) * a.dil + 1;
            __syncthreads();
            if constexpr (PF) {
                commit(n, t0);
            } else {
                wg_fill<VEC>(Ys, a.PY, cfY, BMW, mvalid, a.gy.coff + m0, a.gy, (long long)n * a.gy.ctot * gy_cs, gy_cs,
                             a.T_out, V, t0, bt);
                wg_fill<VEC>(Xs, a.PX, cfX, BKW, kvalid, a.src.coff + k0, a.src, (long long)n * a.src.ctot * x_cs, x_cs,
                             a.T_in, V, t0 * a.stride - a.pad, tin);
            }
            __syncthreads();
            if constexpr (PF) {               // next chunk's loads fly under this chunk's MFMAs
                if (ci + 1 < c_end) prefetch((ci + 1) / cpt, ((ci + 1) % cpt) * a.BT);
            }
            for (int tl = PS ? wave : 0; tl < bt; tl += PS ? 4 : 1) {
#pragma unroll 5
                for (int v4 = 0; v4 < V4; ++v4) {
                    int v = v4 * 4 + kq;
                    bool vok = v < V;
                    int vc = vok ? v : 0;
                    float av[WMT];
#pragma unroll
                    for (int x = 0; x < WMT; ++x) {
                        float t = yrow[x * 16 * a.PY + tl * V + vc];
                        av[x] = vok ? t : 0.f;
                    }
#pragma unroll
                    for (int tap = 0; tap < KT; ++tap) {
                        const int xo = (tl * a.stride + tap * a.dil) * V + vc;
#pragma unroll
                        for (int y = 0; y < WKT; ++y) {
                            float bv = xrow[y * 16 * a.PX + xo];
#pragma unroll
                            for (int x = 0; x < WMT; ++x) acc[tap][x][y] = mfma16(av[x], bv, acc[tap][x][y]);
                        }
                    }
                }
            }
        }
    }
    float* out = a.part + (long long)split * a.M * a.K * KT;
    if constexpr (PS) {                       // sum the four waves' partial tiles through LDS (operand tiles are dead)
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < KT; ++tap)
#pragma unroll
            for (int r = 0; r < 4; ++r) smem[(wave * KT + tap) * 256 + lane * 4 + r] = acc[tap][0][0][r];
        __syncthreads();
        const int l = tid >> 2, r = tid & 3;
        const int m = m0 + (l >> 4) * 4 + r, k = k0 + (l & 15);
        if (m < a.M && k < a.K) {
#pragma unroll
            for (int tap = 0; tap < KT; ++tap) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) t += smem[(w * KT + tap) * 256 + tid];
                out[((long long)m * a.K + k) * KT + tap] = t;
            }
        }
        return;
    }
#pragma unroll
    for (int tap = 0; tap < KT; ++tap)
#pragma unroll
        for (int x = 0; x < WMT; ++x)
#pragma unroll
            for (int y = 0; y < WKT; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int m = m0 + (wr * WMT + x) * 16 + kq * 4 + r;
                    int k = k0 + (wc * WKT + y) * 16 + j;
                    if (m < a.M && k < a.K) out[((long long)m * a.K + k) * KT + tap] = acc[tap][x][y][r];
                }
}


// ===========================================================================
// 1x1 stride-1 weight gradient as an LDS-DMA "NT" GEMM:  dW[m][k] = sum_{n,p} gy(n,m,p) x(n,k,p),
// p = (t, v) contiguous in both operands.
//
//   workgroup   512 threads = 8 waves as 2 (m) x 4 (k); tile (32*WMT) x (64*WKT) of dW, one n-split
//   chunk       32 contraction indices; every operand row is 128 B = 8 slots of 16 B; one dwordx4
//               LDS-DMA piece carries 8 rows (1 KB, lane-linear).  Slot u of row r is stored at slot
//               u ^ (r & 7) (swizzle applied to the per-lane SOURCE address), which makes the ds_read_b128
//               fragment reads below bank-conflict free.
//   contraction MFMA step s of a 16-index block takes p = 4*kq + s: each lane covers four steps with one
//               16-byte read per operand tile (the same permutation on both operands).
//   prologue    per-ROW coefficients (BatchNorm(-backward) apply, two-source combine, ReLU) are lane
//               constants here (lane = row), applied to the fragment registers
//   pipeline    3-stage ring, two chunks in flight, counted vmcnt + one raw s_barrier per chunk
//   row tails   a row (T*V floats) that is not a multiple of 32 ends in a chunk that is fetched from [len - 32, len) --
//               no read past the row -- with the elements the previous chunk already covered zeroed in the gy fragment
//   k x 1       (stride 1, "same" padding) tap kt contracts gy[t] with x[t + kt*dil - pad]: the same GEMM over the
//               window of frames both sides have, i.e. two row offsets and a shorter row.  Taps are a grid axis
//               (blockIdx -> (tap, split, tile)); dW is written [m][k][kt].  Offsets are multiples of V floats:
//               gfx950 takes dword-aligned 16-byte DMA pieces at full rate (tools/probes/unaligned_probe.hip).
// ===========================================================================
constexpr int W_PC = 32, W_NST = 3, W_NT = 512;

// tamgcn_wgrad_pair: rows m >= M0 of the gradient operand come from a second tensor (as its channel gy1.coff + m - M0, with its own
// prologue coefficients); a.M is the stacked extent.  M0 % 8 == 0 (host): a DMA piece of eight rows belongs to one tensor.
struct WgradPair { int M0; SrcDev gy1; };

template <int WMT, int WKT, int NY, int NX, bool SPL, int NST, bool PAIR = false>
#ifndef TG_WKO
#define TG_WKO 0      // knock-out side builds of the weight-gradient kernel (tools/wgrad_knockout.py): 1 one MFMA in eight, 2 no DMA, 4 no fragment reads, 8 no barrier (profiles/r04_wgrad_knockout.txt)
#endif
__global__ __launch_bounds__(W_NT, 2) void wgrad_glds_kernel(const WgradArgs a, int ntk, int ntm, const WgradPair wp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BMW = 2 * WMT * 16, BKW = 4 * WKT * 16;
    constexpr int RY = BMW * NY, RX = BKW * NX, ROWS = RY + RX;
    constexpr int STG = ROWS * W_PC;                              // floats per stage
    constexpr int NPIECE = ROWS / 8;                              // 1 KB pieces per chunk
    constexpr int MAXP = (NPIECE + 7) / 8;                        // per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4, wr = wave >> 2, wc = wave & 3;
    int split, tile, tap;
    {
        const int nt = ntk * ntm, per_tap = nt * a.nsplit;
        int L = blockIdx.x;
        tap = L / per_tap; L -= tap * per_tap;
        if ((a.nsplit & 7) == 0) { const int xcd = L & 7, i = L >> 3; tile = i % nt; split = (i / nt) * 8 + xcd; }
        else { split = L / nt; tile = L - split * nt; }
    }
    const int k0 = (tile % ntk) * BKW, m0 = (tile / ntk) * BMW;
    const long long cs = (long long)a.T_out * a.V;               // channel-row stride of gy (and of x at stride 1)
    const long long csx = (long long)a.T_in * a.V;               // ... of x
    const float rV = 1.0f / (float)a.V;
    // this tap's window: frames t with 0 <= t < T and 0 <= t + dlt < T
    const int dlt = a.KTG > 1 ? tap * a.dil - a.pad : 0;
    const int wlen = (a.T_out - (dlt < 0 ? -dlt : dlt)) * a.V;    // host: >= 2 * W_PC
    const long long ylo = dlt < 0 ? (long long)(-dlt) * a.V : 0, xlo = dlt > 0 ? (long long)dlt * a.V : 0;
    const int cpf = wlen / W_PC, ntail = wlen - cpf * W_PC;       // full chunks, elements of the overlapping last one
    const int cps = cpf + (ntail ? 1 : 0);                        // chunks per sample
    // a split owns a contiguous range of the (n, chunk) sequence: splits may be finer than samples
    const int n_per = (a.N * cps + a.nsplit - 1) / a.nsplit;
    const int c_begin = split * n_per, nch = max(0, min(a.N * cps, c_begin + n_per) - c_begin);

    // ---- DMA descriptors.  Stage rows: [Y1 | Y2 | X1 | X2]; lane -> (row in piece, physical slot)
    const int pr = lane >> 3, ps = lane & 7;
    const int pu = ps ^ pr;                                       // logical 16-byte slot this lane fetches
    const float* p_base[MAXP];
    bool p_ok[MAXP], p_on[MAXP], p_isy[MAXP], p_y1[PAIR ? MAXP : 1];
    int p_dst[MAXP];
    int nissue = 0;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
        const int q = wave + i * 8;
        const bool qok = q < NPIECE;
        const int row0 = (qok ? q : 0) * 8;                       // first stage row of the piece
        const bool isy = row0 < RY;
        int img, r;                                               // image (0/1) and row inside the tile
        if (isy) { img = row0 / BMW; r = row0 - img * BMW + pr; }
        else { img = (row0 - RY) / BKW; r = row0 - RY - img * BKW + pr; }
        const SrcDev& sd = isy ? a.gy : a.src;
        const int ch = (isy ? m0 : k0) + r;
        p_ok[i] = qok && ch < (isy ? a.M : a.K);
        p_base[i] = (img == 0 ? sd.x1 : sd.x2) + (long long)(sd.coff + (p_ok[i] ? ch : 0)) * (isy ? cs : csx) + pu * 4;
        if constexpr (PAIR) {
            p_y1[i] = isy && p_ok[i] && ch >= wp.M0;
            if (p_y1[i]) p_base[i] = (img == 0 ? wp.gy1.x1 : wp.gy1.x2) + (long long)(wp.gy1.coff + ch - wp.M0) * cs + pu * 4;
        }
        p_isy[i] = isy;
        p_dst[i] = row0 * W_PC;
        p_on[i] = __ballot(p_ok[i]) != 0ull;
        nissue += p_on[i] ? 1 : 0;
    }
    const long long ystep = (long long)a.gy.ctot * cs, xstep = (long long)a.src.ctot * csx;
    const long long ystep1 = PAIR ? (long long)wp.gy1.ctot * cs : 0;
    auto issue = [&](int c) {
        if (TG_WKO & 2) return;
        float* st = smem + (c % NST) * STG;
        const int gc = c_begin + c, nn = gc / cps, pc = gc - nn * cps;
        const int po = pc < cpf ? pc * W_PC : wlen - W_PC;        // the row's last, partial chunk: re-fetch the last 32
        const long long oy = (long long)nn * ystep + ylo + po;
        const long long oy1 = PAIR ? (long long)nn * ystep1 + ylo + po : 0;
        // stride 2: this lane's slot starts at p0 = po + 4 pu of frame p0 / V; its x elements sit one frame further per frame
        const long long ox = (long long)nn * xstep + xlo + po + (a.stride == 2 ? tg_rcp_div(po + pu * 4, rV) * a.V : 0);
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            if (p_on[i]) {
                const float* gp = p_base[i] + (p_isy[i] ? oy : ox);
                if constexpr (PAIR) { if (p_y1[i]) gp = p_base[i] + oy1; }
                if (p_ok[i]) __builtin_amdgcn_global_load_lds((tg_gptr)gp, (tg_lptr)(st + p_dst[i]), 16, 0, 0);
            }
        }
    };

    // ---- per-lane row coefficients (lane j <-> row of each fragment tile)
    float cy1[WMT], cy2[WMT], cy0[WMT], cx1[WKT], cx2[WKT], cx0[WKT];
#pragma unroll
    for (int x = 0; x < WMT; ++x) {
        const int m = m0 + (wr * WMT + x) * 16 + j;
        const bool ok = m < a.M && a.gy.coef;
        const int ch = a.gy.coff + (m < a.M ? m : 0);
        cy1[x] = ok ? a.gy.coef[ch] : 1.f;
        cy2[x] = (ok && NY == 2) ? a.gy.coef[a.gy.ctot + ch] : 0.f;
        cy0[x] = ok ? a.gy.coef[2 * a.gy.ctot + ch] : 0.f;
        if constexpr (PAIR) {                                       // a row of the second tensor: its own coefficient table (host: not null)
            if (m < a.M && m >= wp.M0) {
                const int c1 = wp.gy1.coff + m - wp.M0, ct = wp.gy1.ctot;
                cy1[x] = wp.gy1.coef[c1]; cy2[x] = NY == 2 ? wp.gy1.coef[ct + c1] : 0.f; cy0[x] = wp.gy1.coef[2 * ct + c1];
            }
        }
    }
#pragma unroll
    for (int y = 0; y < WKT; ++y) {
        const int k = k0 + (wc * WKT + y) * 16 + j;
        const bool ok = k < a.K && a.src.coef;
        const int ch = a.src.coff + (k < a.K ? k : 0);
        cx1[y] = ok ? a.src.coef[ch] : 1.f;
        cx2[y] = (ok && NX == 2) ? a.src.coef[a.src.ctot + ch] : 0.f;
        cx0[y] = ok ? a.src.coef[2 * a.src.ctot + ch] : 0.f;
    }
    const float loy = a.gy.act == 1 ? 0.f : -__builtin_inff(), lox = a.src.act == 1 ? 0.f : -__builtin_inff();
    const bool yplain = !a.gy.coef && a.gy.act != 1, xplain = !a.src.coef && a.src.act != 1;   // plain tensors skip the prologue

    f32x4 acc[WMT][WKT];
#pragma unroll
    for (int x = 0; x < WMT; ++x)
#pragma unroll
        for (int y = 0; y < WKT; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment offsets inside a stage (floats): row * 32 + 4 * ((4b + kq) ^ (row & 7)), row & 7 == j & 7
    const int yoff = ((wr * WMT) * 16 + j) * W_PC, xoff = (RY + (wc * WKT) * 16 + j) * W_PC;
    const int sl0 = ((kq) ^ (j & 7)) * 4, sl1 = ((4 + kq) ^ (j & 7)) * 4;

    // NST = 3: two chunks in flight; NST = 2 (tiles whose two-stage ring lets a second workgroup share the CU):
    // one chunk in flight per workgroup, the neighbour covers the wait
    if (nch > 0) issue(0);
    if (NST == 3 && nch > 1) issue(1);
    for (int c = 0; c < nch; ++c) {
        tg_wait_vmcnt<15>((NST == 3 && c + 1 < nch) ? nissue : 0);
        if (!(TG_WKO & 8)) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (c + NST - 1 < nch) issue(c + NST - 1);
        const float* st = smem + (c % NST) * STG;
        // one half-chunk's fragments (16 contraction indices): four k4 steps
        auto frag = [&](int b, f32x4 (&avb)[WMT], f32x4 (&bvb)[WKT]) {
            const int sl = b ? sl1 : sl0;
            if (TG_WKO & 4) {
#pragma unroll
                for (int x = 0; x < WMT; ++x) asm volatile("" : "=v"(avb[x]));
#pragma unroll
                for (int y = 0; y < WKT; ++y) asm volatile("" : "=v"(bvb[y]));
                return;
            }
#pragma unroll
            for (int x = 0; x < WMT; ++x) {
                f32x4 v = *reinterpret_cast<const f32x4*>(st + yoff + x * 16 * W_PC + sl);
                if constexpr (NY == 2) {
                    f32x4 v2 = *reinterpret_cast<const f32x4*>(st + BMW * W_PC + yoff + x * 16 * W_PC + sl);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(cy1[x], v[e], fmaf(cy2[x], v2[e], cy0[x])), loy);
                } else if (!yplain) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(cy1[x], v[e], cy0[x]), loy);
                }
                avb[x] = v;
            }
#pragma unroll
            for (int y = 0; y < WKT; ++y) {
                f32x4 v = *reinterpret_cast<const f32x4*>(st + xoff + y * 16 * W_PC + sl);
                if constexpr (NX == 2) {
                    f32x4 v2 = *reinterpret_cast<const f32x4*>(st + BKW * W_PC + xoff + y * 16 * W_PC + sl);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(cx1[y], v[e], fmaf(cx2[y], v2[e], cx0[y])), lox);
                } else if (!xplain) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(cx1[y], v[e], cx0[y]), lox);
                }
                bvb[y] = v;
            }
            if (ntail && (c_begin + c) % cps == cpf) {           // overlapping last chunk: keep only its last ntail elements
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * (4 * b + kq) + e < W_PC - ntail) {
#pragma unroll
                        for (int x = 0; x < WMT; ++x) avb[x][e] = 0.f;
                    }
            }
        };
        f32x4 av[2][WMT], bv[2][WKT];
        frag(0, av[0], bv[0]);
        frag(1, av[1], bv[1]);
        if constexpr (SPL) {                // the lane's eight contraction indices of this chunk = one K = 32 fragment
            bf16x8_t ah[WMT], al[WMT], bh[WKT], bl[WKT];
#pragma unroll
            for (int x = 0; x < WMT; ++x) split_bf16x8(av[0][x], av[1][x], ah[x], al[x]);
#pragma unroll
            for (int y = 0; y < WKT; ++y) split_bf16x8(bv[0][y], bv[1][y], bh[y], bl[y]);
#pragma unroll
            for (int y = 0; y < WKT; ++y)
#pragma unroll
                for (int x = 0; x < WMT; ++x) acc[x][y] = mfma_split(ah[x], al[x], bh[y], bl[y], acc[x][y]);
        } else {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < ((TG_WKO & 1) ? (b ? 0 : 1) : 4); ++e)
#pragma unroll
                    for (int y = 0; y < WKT; ++y)
#pragma unroll
                        for (int x = 0; x < WMT; ++x) acc[x][y] = mfma16(av[b][x][e], bv[b][y][e], acc[x][y]);
        }
    }
    float* out = a.part + (long long)split * a.M * a.K * a.KTG + tap;
#pragma unroll
    for (int x = 0; x < WMT; ++x)
#pragma unroll
        for (int y = 0; y < WKT; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wr * WMT + x) * 16 + kq * 4 + r;
                const int k = k0 + (wc * WKT + y) * 16 + j;
                if (m < a.M && k < a.K) out[((long long)m * a.K + k) * a.KTG] = acc[x][y][r];
            }
}

template <int WMT, int WKT, int NY, int NX, bool SPL, bool PAIR = false>
static int launch_wgrad_glds(WgradArgs& a, hipStream_t s, const WgradPair& wp = WgradPair{}) {
    constexpr int BMW = 2 * WMT * 16, BKW = 4 * WKT * 16;
    constexpr size_t STAGE = sizeof(float) * (size_t)(BMW * NY + BKW * NX) * W_PC;
    // a third stage only where it does not cost the second workgroup per CU
    constexpr int NST = (2 * STAGE <= 80 * 1024 && 3 * STAGE > 80 * 1024) ? 2 : W_NST;
    const size_t lds = NST * STAGE;
    const int ntk = ceil_div(a.K, BKW), ntm = ceil_div(a.M, BMW);
    tg_launch_lds<wgrad_glds_kernel<WMT, WKT, NY, NX, SPL, NST, PAIR>>(160 * 1024, dim3((unsigned)(ntk * ntm * a.nsplit * a.KTG)), dim3(W_NT), lds, s, a, ntk, ntm, wp);
    tamgcn_note_kernel("wgrad_glds_kernel<%d, %d, %d, %d, %s, %d>%s%s", WMT, WKT, NY, NX, SPL ? "split" : "f32", NST, a.KTG > 1 ? " taps" : "", PAIR ? " pair" : "");
    return 0;
}

template <int WMT, int WKT, bool SPL>
static int launch_wgrad_glds_spl(WgradArgs& a, hipStream_t s) {
    const bool y2 = a.gy.x2 != nullptr, x2 = a.src.x2 != nullptr;
    if (y2 && x2) return launch_wgrad_glds<WMT, WKT, 2, 2, SPL>(a, s);
    if (y2) return launch_wgrad_glds<WMT, WKT, 2, 1, SPL>(a, s);
    if (x2) return launch_wgrad_glds<WMT, WKT, 1, 2, SPL>(a, s);
    return launch_wgrad_glds<WMT, WKT, 1, 1, SPL>(a, s);
}

// split-fp32 MFMA (TAMGCN_SPLIT_BF16 >= 1, the default) or the exact fp32-input MFMA (0)
template <int WMT, int WKT>
static int launch_wgrad_glds_src(WgradArgs& a, hipStream_t s) {
    const int mode = tamgcn_split_mode();
    const bool spl = mode >= 1;            // measured faster at every layer shape, HBM-bound ones included (fewer MFMA cycles per byte)
    return spl ? launch_wgrad_glds_spl<WMT, WKT, true>(a, s) : launch_wgrad_glds_spl<WMT, WKT, false>(a, s);
}

static inline int even_pitch(int n) {      // smallest p >= n with p == 2 (mod 4): conflict-free column reads, 8-byte rows
    int p = (n + 3) & ~3;
    return p + 2;
}

template <int KT, int WMT, int WKT, bool PS = false>
static int launch_wgrad(WgradArgs& a, hipStream_t s) {
    constexpr int BMW = PS ? 16 : 2 * WMT * 16, BKW = PS ? 16 : 2 * WKT * 16;
    const int V = a.V;
    // 16-byte slots: always for V % 4 == 0; the p-split kernel also takes rows that are only dword aligned (V = 25), its
    // slots then may straddle two frames -- the chunk must still be whole slots on both sides
    const bool ragged = (V % 4) != 0;
    const bool vec = !ragged || PS;
    int BT = 8;
    if (BT > a.T_out && !ragged) BT = a.T_out;
    size_t lds;
    for (;;) {
        a.BT = BT;
        a.TIN = (BT - 1) * a.stride + (KT - 1) * a.dil + 1;
        a.PY = even_pitch(BT * V);
        a.PX = even_pitch(a.TIN * V);
        lds = sizeof(float) * ((size_t)BMW * a.PY + (size_t)BKW * a.PX + 3 * (BMW + BKW));
        bool slots_ok = !(vec && (KT == 1 || PS)) ||
                        (BMW * (BT * V / 4) <= WG_NPF * NTHREADS && BKW * (a.TIN * V / 4) <= WG_NPF * NTHREADS);
        if (ragged && PS && ((BT * V) % 4 != 0 || (a.TIN * V) % 4 != 0)) slots_ok = false;
        if (PS && lds < sizeof(float) * 4 * KT * 256) lds = sizeof(float) * 4 * KT * 256;   // the final cross-wave reduction
        if ((lds <= 48 * 1024 && slots_ok) || BT == 1) {
            if (!slots_ok) { tamgcn_set_error("tamgcn_wgrad: prefetch slots exceeded (V=%d stride=%d)", V, a.stride); return -1; }
            break;
        }
        BT = BT / 2;
    }
    if (lds > 160 * 1024) { tamgcn_set_error("tamgcn_wgrad: tile does not fit LDS (V=%d)", V); return -1; }
    a.n_per = ceil_div(a.N * ceil_div(a.T_out, a.BT), a.nsplit);          // frame chunks per split
    tamgcn_note_kernel("wgrad_kernel<%d, %d, %d, %s%s>", KT, WMT, WKT, vec ? "true" : "false", PS ? ", p-split" : "");
    dim3 grid(ceil_div(a.K, BKW), ceil_div(a.M, BMW), a.nsplit);
    if (vec) tg_launch_lds<wgrad_kernel<KT, WMT, WKT, true, PS>>(160 * 1024, grid, dim3(NTHREADS), lds, s, a);
    else tg_launch_lds<wgrad_kernel<KT, WMT, WKT, false>>(160 * 1024, grid, dim3(NTHREADS), lds, s, a);
    return 0;
}

// the paired form (tamgcn_wgrad_pair): both gradient tensors carry the two-source BatchNorm-backward prologue, x is plain or one-source
template <int WMT, int WKT>
static int launch_wgrad_glds_pair(WgradArgs& a, hipStream_t s, const WgradPair& wp) {
    const bool spl = tamgcn_split_mode() >= 1, x2 = a.src.x2 != nullptr;
    if (spl) return x2 ? launch_wgrad_glds<WMT, WKT, 2, 2, true, true>(a, s, wp) : launch_wgrad_glds<WMT, WKT, 2, 1, true, true>(a, s, wp);
    return x2 ? launch_wgrad_glds<WMT, WKT, 2, 2, false, true>(a, s, wp) : launch_wgrad_glds<WMT, WKT, 2, 1, false, true>(a, s, wp);
}

// tile shape chosen from (M, K, KT); the host wrapper uses the same rule to size nsplit
static void wgrad_tile(int M, int K, int KT, int* wmt, int* wkt) {
    if (KT == 1) { *wmt = M <= 64 ? 2 : 4; *wkt = K <= 64 ? 2 : 4; }
    else if (KT == 9) { *wmt = 1; *wkt = 1; }
    else { *wmt = M <= 32 ? 1 : 2; *wkt = K <= 32 ? 1 : 2; if (*wmt != *wkt) { *wmt = 2; *wkt = 2; } }
}

}  // namespace

// the LDS-DMA form applies (and with which tile) -- shared by tamgcn_wgrad and tamgcn_wgrad_max_split
static bool wgrad_glds_plan(const tamgcn_wgrad_desc* d, int* wmt, int* wkt) {
    wgrad_tile(d->M, d->K, d->KT, wmt, wkt);
    const bool al16 = (((uintptr_t)d->gy.x1 | (uintptr_t)d->src.x1 | (uintptr_t)(d->gy.x2 ? d->gy.x2 : d->gy.x1) |
                        (uintptr_t)(d->src.x2 ? d->src.x2 : d->src.x1)) & 15) == 0;
    // 1x1, or k x 1 with "same" padding (one window per tap); every window holds at least two 32-element chunks.
    // The 16-channel temporal branches stay on the register-staged kernels (one 16x16 tile: nothing for 8 waves to share;
    // measured r02: N-UCLA step 31.1 vs 30.2 ms, NTU 1.33 vs 1.0 ms per launch), and so do the 32-channel ones where that
    // kernel has its 16-byte form (V % 4 == 0: 51 vs 114 us per launch at N-UCLA; at V = 25 the tap form wins 672 vs 896 us); TAMGCN_WGRAD_TAPS=2 sends them here too,
    // =0 disables the tap form.
    const bool taps = d->KT > 1 && d->pad == d->dil * (d->KT - 1) / 2 && (d->dil * (d->KT - 1)) % 2 == 0 && tamgcn_wgrad_taps() &&
                      (d->M > 32 || d->K > 32 || (d->V % 4 != 0 && (d->M > 16 || d->K > 16)) || tamgcn_wgrad_taps() == 2);
    // a 1x1 conv with temporal stride 2 (V % 4 == 0): gy rows are contiguous, the x slot of contraction index p = t*V + v
    // sits at (2 t) V + v -- a per-lane source offset of the DMA piece, recomputed per chunk (round 4)
    const bool strided = d->KT == 1 && d->pad == 0 && d->stride == 2 && (d->V & 3) == 0 && d->T_out == (d->T_in - 1) / 2 + 1;
    bool glds = (taps || (d->KT == 1 && d->pad == 0)) && ((d->stride == 1 && d->T_in == d->T_out) || strided) && al16 &&
                (long long)(d->T_out - d->pad) * d->V >= 2 * W_PC;
    if (!glds) return false;
    if (d->KT > 1) { *wmt = d->M <= 64 ? 2 : 4; *wkt = d->K <= 64 ? 2 : 4; }      // the 1x1 rule (units of 32)
    // three stages of both operands (every source) must fit the CU's LDS: shrink the tile
    auto fits = [&](int tm, int tk) {
        const size_t rows = (size_t)tm * 32 * (d->gy.x2 ? 2 : 1) + (size_t)tk * 32 * (d->src.x2 ? 2 : 1);
        return sizeof(float) * W_NST * rows * W_PC <= 160 * 1024;
    };
    if (!fits(*wmt, *wkt) && *wmt == 4) *wmt = 2;
    if (!fits(*wmt, *wkt) && *wkt == 4) *wkt = 2;
    if (fits(*wmt, *wkt)) return true;
    wgrad_tile(d->M, d->K, d->KT, wmt, wkt);
    return false;
}

extern "C" int tamgcn_wgrad_max_split(const tamgcn_wgrad_desc* d) {
    if (!d || d->N <= 0 || d->T_out <= 0 || d->V <= 0) return -1;
    int wmt, wkt;
    if (!wgrad_glds_plan(d, &wmt, &wkt)) {
        // register-staged kernel: frame chunks hold at most 8 frames; at least one of those chunks per workgroup
        const long long m = (long long)d->N * ((d->T_out + 7) / 8);
        return (int)(m < d->N ? d->N : (m > 65535 ? 65535 : m));
    }
    const long long chunks = (long long)d->N * (((long long)(d->T_out - d->pad) * d->V) / W_PC);
    const long long m = chunks / 8;                      // at least 8 chunks of 32 per workgroup
    return (int)(m < d->N ? d->N : (m > 65535 ? 65535 : m));
}

extern "C" int tamgcn_wgrad(const tamgcn_wgrad_desc* d, void* stream) {
    TG_CHECK(d && d->gy.x1 && d->src.x1 && d->part, "tamgcn_wgrad: null pointer");
    TG_CHECK(d->N > 0 && d->M > 0 && d->K > 0 && d->T_in > 0 && d->T_out > 0 && d->V > 0 && d->nsplit > 0,
             "tamgcn_wgrad: bad dims");
    TG_CHECK(d->gy.coff + d->M <= d->gy.ctot && d->src.coff + d->K <= d->src.ctot, "tamgcn_wgrad: channel slice out of range");
    TG_CHECK(d->nsplit <= tamgcn_wgrad_max_split(d), "tamgcn_wgrad: nsplit=%d exceeds tamgcn_wgrad_max_split=%d", d->nsplit,
             tamgcn_wgrad_max_split(d));
    WgradArgs a;
    a.gy = make_src(d->gy); a.src = make_src(d->src);
    a.N = d->N; a.M = d->M; a.K = d->K; a.T_in = d->T_in; a.T_out = d->T_out; a.V = d->V;
    a.dil = d->dil; a.stride = d->stride; a.pad = d->pad; a.part = d->part; a.nsplit = d->nsplit;
    hipStream_t s = (hipStream_t)stream;
    int rc, wmt, wkt;
    const bool glds = wgrad_glds_plan(d, &wmt, &wkt);
    a.KTG = glds ? d->KT : 1;
    if (glds) {              // tile = 64 or 128 per side by the same rule as wgrad_tile (wmt: rows/32, wkt: cols/64)
        if (wmt == 2 && wkt == 2) rc = launch_wgrad_glds_src<2, 1>(a, s);
        else if (wmt == 4 && wkt == 2) rc = launch_wgrad_glds_src<4, 1>(a, s);
        else if (wmt == 2 && wkt == 4) rc = launch_wgrad_glds_src<2, 2>(a, s);
        else rc = launch_wgrad_glds_src<4, 2>(a, s);
        if (rc) return rc;
        TG_LAUNCH_CHECK("tamgcn_wgrad");
        return 0;
    }
    if (d->KT == 1) {        // register-staged 1x1 form: one frame of a 128-row tile must fit the prefetch slots (V = 64: 64-row tiles)
        const int per_row = (d->V + 3) / 4;
        if (wmt == 4 && 128 * per_row > WG_NPF * NTHREADS) wmt = 2;
        if (wkt == 4 && 128 * per_row > WG_NPF * NTHREADS) wkt = 2;
    }
    switch (d->KT) {
        case 1:
            if (wmt == 2 && wkt == 2) rc = launch_wgrad<1, 2, 2>(a, s);
            else if (wmt == 4 && wkt == 2) rc = launch_wgrad<1, 4, 2>(a, s);
            else if (wmt == 2 && wkt == 4) rc = launch_wgrad<1, 2, 4>(a, s);
            else rc = launch_wgrad<1, 4, 4>(a, s);
            break;
        // k x 1 kernels: when the preferred tile's line buffer (frames + temporal halo, V joints each) does not fit --
        // V = 64 -- fall back to the next smaller tile instead of refusing
        case 3:
            rc = wmt == 1 ? -1 : launch_wgrad<3, 2, 2>(a, s);
            if (rc == -1) rc = launch_wgrad<3, 1, 1>(a, s);
            break;
        case 5:
            rc = (d->M <= 16 && d->K <= 16 && (d->V % 4 == 0 || d->stride == 1)) ? launch_wgrad<5, 1, 1, true>(a, s) : -1;
            if (rc == -1 && wmt != 1) rc = launch_wgrad<5, 2, 2>(a, s);
            if (rc == -1) rc = launch_wgrad<5, 1, 1>(a, s);
            break;
        case 9: rc = launch_wgrad<9, 1, 1>(a, s); break;
        default: tamgcn_set_error("tamgcn_wgrad: kernel size %d not instantiated (1,3,5,9)", d->KT); return -1;
    }
    if (rc) return rc;
    TG_LAUNCH_CHECK("tamgcn_wgrad");
    return 0;
}


// Two weight gradients against the same x as one launch: rows [0, M0) of the gradient operand from gy0, rows [M0, M0 + M1) from gy1,
// one slab array [nsplit][M0 + M1][K].  nsplit is bounded by tamgcn_wgrad_max_split of the single descriptor with M = M0 + M1.
extern "C" int tamgcn_wgrad_pair(const tamgcn_wgrad_pair_desc* d, void* stream) {
    TG_CHECK(d, "tamgcn_wgrad_pair: null descriptor");
    TG_CHECK(d->gy0.x1 && d->gy1.x1 && d->src.x1 && d->part, "tamgcn_wgrad_pair: null pointer");
    TG_CHECK(d->N > 0 && d->M0 > 0 && d->M1 >= 0 && d->K > 0 && d->T > 0 && d->V > 0 && d->nsplit > 0,
             "tamgcn_wgrad_pair: bad dims N=%d M0=%d M1=%d K=%d T=%d V=%d nsplit=%d", d->N, d->M0, d->M1, d->K, d->T, d->V, d->nsplit);
    TG_CHECK(d->M1 > 0, "tamgcn_wgrad_pair: M1 = 0: nothing to pair (use tamgcn_wgrad)");
    TG_CHECK(d->stride == 1, "tamgcn_wgrad_pair: stride %d: only stride-1 1x1 convolutions pair up", d->stride);
    TG_CHECK(d->M0 % 8 == 0, "tamgcn_wgrad_pair: M0=%d is not a multiple of the chunk's 8-row pieces", d->M0);
    TG_CHECK(d->gy0.coff >= 0 && d->gy0.coff + d->M0 <= d->gy0.ctot && d->gy1.coff >= 0 && d->gy1.coff + d->M1 <= d->gy1.ctot &&
             d->src.coff >= 0 && d->src.coff + d->K <= d->src.ctot, "tamgcn_wgrad_pair: channel slice out of range");
    TG_CHECK(d->gy0.x2 && d->gy1.x2 && d->gy0.coef && d->gy1.coef && d->gy0.act == d->gy1.act,
             "tamgcn_wgrad_pair: both gradient operands carry the two-source prologue (x1, x2, coef)");
    tamgcn_wgrad_desc sd = {};                               // the single weight gradient with the stacked rows: its plan is the pair's
    sd.gy = d->gy0; sd.src = d->src; sd.N = d->N; sd.M = d->M0 + d->M1; sd.K = d->K; sd.T_in = d->T; sd.T_out = d->T; sd.V = d->V;
    sd.KT = 1; sd.dil = 1; sd.stride = 1; sd.pad = 0; sd.part = d->part; sd.nsplit = d->nsplit;
    TG_CHECK(d->nsplit <= tamgcn_wgrad_max_split(&sd), "tamgcn_wgrad_pair: nsplit=%d exceeds tamgcn_wgrad_max_split=%d", d->nsplit,
             tamgcn_wgrad_max_split(&sd));
    int wmt, wkt;
    const bool al1 = (((uintptr_t)d->gy1.x1 | (uintptr_t)d->gy1.x2) & 15) == 0;
    TG_CHECK(wgrad_glds_plan(&sd, &wmt, &wkt) && al1, "tamgcn_wgrad_pair: V=%d T=%d is not a shape of the LDS-DMA weight gradient (or an operand is not 16-byte aligned)", d->V, d->T);
    WgradArgs a = {};
    a.gy = make_src(d->gy0); a.src = make_src(d->src);
    a.N = d->N; a.M = sd.M; a.K = d->K; a.T_in = d->T; a.T_out = d->T; a.V = d->V;
    a.dil = 1; a.stride = 1; a.pad = 0; a.part = d->part; a.nsplit = d->nsplit; a.KTG = 1;
    WgradPair wp;
    wp.M0 = d->M0; wp.gy1 = make_src(d->gy1);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (wmt == 2 && wkt == 2) rc = launch_wgrad_glds_pair<2, 1>(a, s, wp);
    else if (wmt == 4 && wkt == 2) rc = launch_wgrad_glds_pair<4, 1>(a, s, wp);
    else if (wmt == 2 && wkt == 4) rc = launch_wgrad_glds_pair<2, 2>(a, s, wp);
    else rc = launch_wgrad_glds_pair<4, 2>(a, s, wp);
    if (rc) return rc;
    TG_LAUNCH_CHECK("tamgcn_wgrad_pair");
    return 0;
}
