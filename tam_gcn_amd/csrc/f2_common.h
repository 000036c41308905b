// What the three small-batch eval families of the TCN_GCN_unit share (f2.hip: V = 20; f2v.hip: V in FV_JOINTS, compile time;
// f2g.hip: 8 <= V <= 28, run time; include/tamgcn.h has the stages and the algebra): the tiling constants, the A-fragment
// loads and the 16-row MFMA product, the kernel-argument structs, and the host half that turns a descriptor into them -- ONE
// order of checks for every entry point: null descriptor, V, S, pointers, shapes, alignment.
#pragma once
#include "common.h"

namespace {

constexpr int F2_NT = 256;                 // four waves
constexpr int F2_BT = 4;                   // frames of a tile
constexpr int F2_G = 4;                    // 16-k blocks of A in flight per wave
constexpr int F2_KC = 128;                 // K rows of a staged chunk of the gcn stage (f2v; f2g: at most)
constexpr int F2_HF = 15;                  // halo tile: 3*stride + (ks-1)*dil + 1 <= 15 frames
constexpr int F2_PX = 36;                  // xbar / pq pitch (V <= 32 columns in two tiles)
constexpr int F2_CT = 8;                   // channels of a gcn tile
constexpr size_t F2_LDS_MAX = 160 * 1024;  // no launch asks for more dynamic LDS

// A fragment of one 16-k block: lane (j, kq) holds A[row j][k0 + 4*kq + i], i = 0..3 (MFMA step i of the block contracts
// k = k0 + 4*kq + i on BOTH operands: any bijection between (step, kq) and k is a valid K order)
__device__ __forceinline__ void f2_load_a(const float* arow, int K, int k0, int kq, bool vec, float (&a)[4]) {
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
__device__ __forceinline__ void f2_load_group(const float* arow, int K, bool vec, int kb, int kbend, int kbstep, int kq, float (&dst)[F2_G][4]) {
#pragma unroll
    for (int g = 0; g < F2_G; ++g) {
        const int b = kb + g * kbstep;
        if (b < kbend) f2_load_a(arow, K, b * 16, kq, vec, dst[g]);
        else { dst[g][0] = dst[g][1] = dst[g][2] = dst[g][3] = 0.f; }
    }
}

// acc[ct] += A[16 rows][16-k blocks kb, kb + kbstep, ... < kbend] * B; this lane's B value for tile ct at row k is bf(k, ct).
// A fragments are fetched four blocks at a time, one group ahead: with one block in flight the loop was one L2 round trip
// (~0.8 us) per 20 MFMAs (~0.1 us).
template <int NCT, class BF>
__device__ __forceinline__ void f2_gemm16(f32x4 (&acc)[NCT], const float* arow, int K, bool vec, int kb, int kbend, int kbstep, int kq, BF bf) {
    constexpr int G = F2_G;
    float a[G][4], an[G][4];
    f2_load_group(arow, K, vec, kb, kbend, kbstep, kq, a);
    for (; kb < kbend; kb += G * kbstep) {
        f2_load_group(arow, K, vec, kb + G * kbstep, kbend, kbstep, kq, an);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int b = kb + g * kbstep;
            if (b < kbend) {                                       // wave-uniform: a whole block of 4 x NCT MFMAs
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

// ---- kernel arguments of f2 and f2v (f2g.hip has its own: these fields and V, kc) ------------------------------------------
struct F2GcnArgs {
    int N, Cin, Cout, T, S, R, res_mode;
    const float *x, *w12, *b12, *w4, *b4, *A, *alpha, *w3, *b3, *sy, *ty, *wd, *bd, *xpart;
    float *E, *sum, *diff;
    int vec12, vec4, vec3, vecd;
    int ntp;                             // f2v_e: frame phases of the xbar sum (4, or 2 where 4 partial tiles do not fit LDS)
};

struct F2GemmArgs {
    int N, K, M, T, mode, relu_rows, vec;
    const float *x, *w, *b, *add;
    float* out;
};

struct F2TcnArgs {
    int N, Cin, Cout, T, T2, stride, Cb, nb, ks, res_mode, vect, vecr;
    int dil[4];
    const float* h;                      // entry outputs (ReLU applied) of branches 0..nb, then the plain branch
    const float* wt[4]; const float* bt[4];   // [Cb][Cb*ks] folded, [Cb]
    const float *sp, *tp;                // pooled branch's BatchNorm as an affine [Cb]
    const float *x, *wr, *br;            // block input (N, Cin, T, V); folded residual conv [Cout][Cin], [Cout]
    float* out;                          // (N, Cout, T2, V)
    float* xpart;                        // NULL | (N, ceil(T2 / 4), Cout, frame): sum over each tile's frames of out (the next block's xbar)
};

// Grouped launches (include/tamgcn.h, "grouped"): samples [g*npg, (g+1)*npg) use the g-th of the parameter arrays that follow
// one another densely behind group 0's.  g comes from blockIdx.y alone: the offset bases stay scalar.  VV = V * V.
__device__ __forceinline__ F2GcnArgs f2_group(F2GcnArgs a, int g, int VV) {
    const long long SC = (long long)a.S * a.Cout;
    a.w12 += g * (long long)a.S * 2 * a.R * a.Cin; a.b12 += g * a.S * 2 * a.R;
    a.w4 += g * SC * a.R; a.b4 += g * SC;
    a.A += g * a.S * VV; a.alpha += g;
    a.w3 += g * SC * a.Cin; a.b3 += g * SC;
    a.sy += g * a.Cout; a.ty += g * a.Cout;
    if (a.res_mode == 2) { a.wd += (long long)g * a.Cout * a.Cin; a.bd += g * a.Cout; }
    return a;
}
__device__ __forceinline__ F2GemmArgs f2_group(F2GemmArgs a, int g) {
    a.w += (long long)g * a.M * a.K;
    a.b += g * a.M;
    return a;
}

// ---- host -----------------------------------------------------------------------------------------------------------
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool f2_al(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// The dynamic-LDS requests from the pitches of a geometry (VP: frame, PD: D, PB: tile, PH: halo tile; ES: floats of a subset's
// E run): what the kernels lay out.  f2.hip's tcn keeps its two regions apart and has its own formula.
constexpr size_t f2_e_lds(int Cin, int R, int ntp, int VP, int PD) {
    const int Kp = (Cin + 15) & ~15, R2p = 2 * R < 16 ? 16 : 2 * R, Rp = (R + 15) & ~15;
    const size_t d = (size_t)Rp * PD, xp = (size_t)ntp * Kp * VP;
    return sizeof(float) * ((size_t)Kp * F2_PX + (size_t)R2p * F2_PX + 64 * F2_PX + (d > xp ? d : xp));
}
constexpr size_t f2_gcn_lds(int Cin, int kc, int PB, int ES) {
    const int Kp = (Cin + 15) & ~15;
    return sizeof(float) * ((size_t)(Kp < kc ? Kp : kc) * PB + 2 * 32 * PB + 3 * (size_t)ES);
}
constexpr size_t f2_gemm_lds(int K, int PB) { return sizeof(float) * ((size_t)((K + 15) & ~15) * PB + 4 * 16 * PB); }
constexpr size_t f2_tcn_lds(int Cin, int Cb, int res_mode, int PB, int PH) {
    const size_t xs = (size_t)(res_mode == 2 ? (Cin + 15) & ~15 : 0) * PB, hs = (size_t)Cb * PH;
    return sizeof(float) * ((size_t)5 * 16 * PB + (xs > hs ? xs : hs));
}

// What differs between the families in the checks of a descriptor: who is served, and the texts of three refusals.
struct F2Family {
    bool (*serves)(int V);
    const char* serves_txt;              // told with a refused V or S
    const char* null_txt;                // told with a null descriptor
    int xalign;                          // bytes the block's input and output are aligned to: 16 (f2 reads them in aligned pieces) or 4
    const char* gcn_align_txt;           // told with a misaligned x, E or xpart of a gcn descriptor
    const char* tcn_align_txt;           // told with a misaligned h, x, out or xpart of a tcn descriptor
    bool v_with_s;                       // a gcn descriptor's refused V is printed with its S (f2)
};
// the alignment texts of the families that read x and write out element-wise (f2v, f2g)
constexpr const char* F2_GCN_ALIGN4_TXT = "x must be 4-byte, E and xpart 16-byte aligned";
constexpr const char* F2_TCN_ALIGN4_TXT = "h and xpart must be 16-byte, x and out 4-byte aligned";

// descriptor -> arguments of the e and gcn kernels (A: the family's struct; a field only one family has is that family's to
// set); need_out: the gcn stage, which writes sum and diff
template <class A>
int f2_gcn_args(const tamgcn_f2_gcn_desc* d, A* a, const F2Family& fam, bool need_out, const char* who) {
    TG_CHECK(d, "%s: %s", who, fam.null_txt);
    if (!fam.serves(d->V)) {
        if (fam.v_with_s) tamgcn_set_error("%s: V=%d S=%d (%s)", who, d->V, d->S, fam.serves_txt);
        else tamgcn_set_error("%s: V=%d (%s)", who, d->V, fam.serves_txt);
        return -1;
    }
    TG_CHECK(d->S == 3, "%s: V=%d S=%d (%s)", who, d->V, d->S, fam.serves_txt);
    TG_CHECK(d->x && d->w12 && d->b12 && d->w4 && d->b4 && d->A && d->alpha && d->w3 && d->b3 && d->sy && d->ty && d->E,
             "%s: null pointer", who);
    TG_CHECK(d->N > 0 && d->T > 0 && d->Cin > 0 && d->Cin <= 256 && d->Cout > 0 && d->Cout % 16 == 0,
             "%s: bad shape N=%d T=%d Cin=%d Cout=%d (Cin <= 256, Cout %% 16 == 0)", who, d->N, d->T, d->Cin, d->Cout);
    TG_CHECK(d->R >= 1 && d->R <= 32, "%s: R=%d outside 1..32", who, d->R);
    TG_CHECK(d->res_mode >= 0 && d->res_mode <= 2, "%s: res_mode=%d", who, d->res_mode);
    TG_CHECK(d->res_mode != 1 || d->Cin == d->Cout, "%s: identity residual needs Cin == Cout", who);
    TG_CHECK(d->res_mode != 2 || (d->wd && d->bd), "%s: convolutional residual without weights", who);
    TG_CHECK(f2_al(d->x, fam.xalign) && al16(d->E) && (!d->xpart || al16(d->xpart)), "%s: %s", who, fam.gcn_align_txt);
    TG_CHECK(!need_out || (d->sum && d->diff && al16(d->sum) && al16(d->diff)), "%s: null or misaligned output", who);
    a->N = d->N; a->Cin = d->Cin; a->Cout = d->Cout; a->T = d->T; a->S = d->S; a->R = d->R; a->res_mode = d->res_mode;
    a->x = d->x; a->w12 = d->w12; a->b12 = d->b12; a->w4 = d->w4; a->b4 = d->b4; a->A = d->A; a->alpha = d->alpha;
    a->w3 = d->w3; a->b3 = d->b3; a->sy = d->sy; a->ty = d->ty; a->wd = d->wd; a->bd = d->bd;
    a->E = d->E; a->sum = d->sum; a->diff = d->diff; a->xpart = d->xpart;
    a->vec12 = d->Cin % 16 == 0 && al16(d->w12);
    a->vec3 = d->Cin % 16 == 0 && al16(d->w3);
    a->vecd = d->res_mode == 2 && d->Cin % 16 == 0 && al16(d->wd);
    a->vec4 = d->R % 16 == 0 && al16(d->w4);
    a->ntp = 4;
    return 0;
}

// x, add and out are the families' own buffers: 16-byte aligned frames everywhere
template <class A>
int f2_gemm_args(const tamgcn_f2_gemm_desc* d, A* a, const F2Family& fam, const char* who) {
    TG_CHECK(d, "%s: %s", who, fam.null_txt);
    TG_CHECK(fam.serves(d->V), "%s: V=%d (%s)", who, d->V, fam.serves_txt);
    TG_CHECK(d->x && d->w && d->b && d->out, "%s: null pointer", who);
    TG_CHECK(d->N > 0 && d->T > 0 && d->K > 0 && d->K <= 256 && d->M > 0 && d->M % 16 == 0,
             "%s: bad shape N=%d T=%d K=%d M=%d (K <= 256, M %% 16 == 0)", who, d->N, d->T, d->K, d->M);
    TG_CHECK(d->mode == 0 || d->mode == 1, "%s: mode=%d", who, d->mode);
    TG_CHECK(d->mode != 0 || d->add, "%s: mode 0 needs the addend", who);
    TG_CHECK(al16(d->x) && al16(d->out) && (!d->add || al16(d->add)), "%s: activations must be 16-byte aligned", who);
    a->N = d->N; a->K = d->K; a->M = d->M; a->T = d->T; a->mode = d->mode; a->relu_rows = d->relu_rows;
    a->vec = d->K % 16 == 0 && al16(d->w);
    a->x = d->x; a->w = d->w; a->b = d->b; a->add = d->add; a->out = d->out;
    return 0;
}

template <class A>
int f2_tcn_args(const tamgcn_f2_tcn_desc* d, A* a, const F2Family& fam, const char* who) {
    TG_CHECK(d, "%s: %s", who, fam.null_txt);
    TG_CHECK(fam.serves(d->V), "%s: V=%d (%s)", who, d->V, fam.serves_txt);
    TG_CHECK(d->h && d->out && d->sp && d->tp, "%s: null pointer", who);
    TG_CHECK(d->N > 0 && d->T > 0 && d->Cout > 0 && d->Cout % 16 == 0 && d->stride >= 1 && d->stride <= 2,
             "%s: bad shape N=%d T=%d Cout=%d stride=%d", who, d->N, d->T, d->Cout, d->stride);
    TG_CHECK(d->nb >= 1 && d->nb <= 4 && d->Cb > 0 && d->Cb % 16 == 0 && d->Cb <= 64 && (d->nb + 2) * d->Cb == d->Cout,
             "%s: nb=%d Cb=%d Cout=%d (Cb %% 16 == 0, Cb <= 64, (nb + 2) Cb == Cout)", who, d->nb, d->Cb, d->Cout);
    TG_CHECK(d->ks >= 1 && d->ks % 2 == 1, "%s: kernel size %d", who, d->ks);
    for (int b = 0; b < d->nb; ++b) {
        TG_CHECK(d->wt[b] && d->bt[b] && d->dil[b] >= 1, "%s: branch %d: null weights or dilation %d", who, b, d->dil[b]);
        TG_CHECK((F2_BT - 1) * d->stride + (d->ks - 1) * d->dil[b] + 1 <= F2_HF, "%s: branch %d: halo of k=%d dilation %d stride %d exceeds %d frames",
                 who, b, d->ks, d->dil[b], d->stride, F2_HF);
    }
    TG_CHECK(d->res_mode >= 0 && d->res_mode <= 2, "%s: res_mode=%d", who, d->res_mode);
    TG_CHECK(d->res_mode == 0 || d->x, "%s: residual without the block input", who);
    TG_CHECK(d->res_mode != 1 || (d->Cin == d->Cout && d->stride == 1), "%s: identity residual needs Cin == Cout, stride 1", who);
    TG_CHECK(d->res_mode != 2 || (d->wr && d->br && d->Cin > 0 && d->Cin <= 256), "%s: convolutional residual: weights / Cin=%d", who, d->Cin);
    TG_CHECK(al16(d->h) && f2_al(d->out, fam.xalign) && (!d->x || f2_al(d->x, fam.xalign)) && (!d->xpart || al16(d->xpart)),
             "%s: %s", who, fam.tcn_align_txt);
    a->N = d->N; a->Cin = d->Cin; a->Cout = d->Cout; a->T = d->T; a->stride = d->stride; a->T2 = (d->T - 1) / d->stride + 1;
    a->Cb = d->Cb; a->nb = d->nb; a->ks = d->ks; a->res_mode = d->res_mode;
    bool vt = (d->Cb * d->ks) % 16 == 0;
    for (int b = 0; b < 4; ++b) {
        a->dil[b] = b < d->nb ? d->dil[b] : 1;
        a->wt[b] = b < d->nb ? d->wt[b] : nullptr;
        a->bt[b] = b < d->nb ? d->bt[b] : nullptr;
        if (b < d->nb) vt = vt && al16(d->wt[b]);
    }
    a->vect = vt;
    a->vecr = d->res_mode == 2 && d->Cin % 16 == 0 && al16(d->wr);
    a->h = d->h; a->sp = d->sp; a->tp = d->tp; a->x = d->x; a->wr = d->wr; a->br = d->br; a->out = d->out; a->xpart = d->xpart;
    return 0;
}

// Grouped launches: groups >= 1, N a multiple of it; and where a launch reads a weight array in 16-byte pieces the group
// stride must keep the pieces aligned.  That second condition cannot fail today -- a vector path needs a row length that is a
// multiple of 16, and every group stride is a multiple of the row length -- it is checked so that a new vec condition cannot
// break it silently.  groups == 0 is the plain entry point: nothing to check.
inline int f2_groups_arg(int groups, const char* who) {
    TG_CHECK(groups >= 1, "%s: groups=%d", who, groups);
    return 0;
}
inline int f2_groups_ok(int N, int groups, const char* who) {
    TG_CHECK(groups >= 1 && N % groups == 0, "%s: N=%d is not a multiple of groups=%d", who, N, groups);
    return 0;
}
inline int f2_group_stride_ok(bool vec, long long stride, const char* who, const char* what) {
    TG_CHECK(!vec || stride % 4 == 0, "%s: group stride of %s (%lld floats) breaks the 16-byte alignment of its vector path", who, what, stride);
    return 0;
}
inline int f2_gcn_groups_ok(const F2GcnArgs& a, int groups, const char* who) {
    if (!groups) return 0;
    return f2_groups_ok(a.N, groups, who) || f2_group_stride_ok(a.vec12, (long long)a.S * 2 * a.R * a.Cin, who, "w12") ||
           f2_group_stride_ok(a.vec4, (long long)a.S * a.Cout * a.R, who, "w4") || f2_group_stride_ok(a.vec3, (long long)a.S * a.Cout * a.Cin, who, "w3") ||
           f2_group_stride_ok(a.vecd, (long long)a.Cout * a.Cin, who, "wd");
}
inline int f2_gemm_groups_ok(const F2GemmArgs& a, int groups, const char* who) {
    if (!groups) return 0;
    return f2_groups_ok(a.N, groups, who) || f2_group_stride_ok(a.vec, (long long)a.M * a.K, who, "w");
}
inline int f2_tcn_groups_ok(const F2TcnArgs& a, int groups, const char* who) {
    if (!groups) return 0;
    return f2_groups_ok(a.N, groups, who) || f2_group_stride_ok(a.vect, (long long)a.Cb * a.Cb * a.ks, who, "wt") ||
           f2_group_stride_ok(a.vecr, (long long)a.Cout * a.Cin, who, "wr");
}

}  // namespace
