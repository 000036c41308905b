// f2g: the small-batch eval-mode TCN_GCN_unit (f2.hip's family: same four stages, same algebra, include/tamgcn.h) for ANY
// joint count 8 <= V <= 28, with V a KERNEL ARGUMENT.  f2v.hip instantiates its kernels per joint count (17, 18, 25) and f2.hip
// is written for 20; every other skeleton used to take the general eval path at batch 1.  This file is to f2v.hip what vgen.hip
// is to ctrgc_tiled.hip: the SAME stage bodies (f2x_body.h, which has the layout), instantiated only on what sizes a register
// array or fixes an LDS pitch -- the frame pitch VP = (V + 3) & ~3 in {8, 12, 16, 20, 24, 28}: six instantiations per stage
// serve 21 joint counts.
//
//   run time    everything f2v derives from V * VP (FgRt): the E run of a channel (EC = V * VP floats), its column tiles, the D
//               pitch (ECT * 16 + 4: conflict-free for every ECT), the 1 KB DMA pieces of a subset's E run, and every
//               `joint < V` predicate.  The last piece of a frame of the contiguous input keeps its first V - (VP - 4) lanes
//               (1..4, a run-time count); at V % 4 == 0 nothing is padded.  Register arrays are sized for V = VP and guarded
//               by wave-uniform run-time counts.
//   LDS         f2v's constants do not fit at the wide end: the gcn stage at V = 28 holds three E runs of 25.6 KB and two
//               partial x3 tiles of 29.7 KB, which leaves 52 KB for the K chunk, not the 59 KB of 128 rows.  The host picks the
//               K chunk per geometry (fg_gcn_kc: the largest multiple of 16 up to 128 that fits 160 KB; 112 rows at V = 28, 128
//               everywhere else), and the E builder takes two frame phases instead of four where four partial tiles do not
//               fit (f2v's rule).  tamgcn_f2g_lds_bytes reports every stage's request; nothing above 160 KB is launched.
//
// S = 3.  No grouped entry points.
#include "f2x_body.h"

namespace {

constexpr int FG_VMIN = 8, FG_VMAX = 28;

// The run-time half of the geometry: what V * VP fixes.
struct FgRt {
    int V, EC, ECT, PD, EPC, ES;
    __host__ __device__ FgRt(int V_, int VP) {
        V = V_;
        EC = V * VP;                                   // floats of one channel of E: rows u of VP
        ECT = (EC + 15) >> 4;                          // column tiles of the E product
        PD = ECT * 16 + 4;                             // D pitch (4 PD % 64 == 16 for every ECT)
        EPC = (F2_CT * EC + 255) >> 8;                 // 1 KB DMA pieces of one subset's E run (F2_CT * EC >= 512)
        ES = EPC * 256;
    }
};

// What the frame pitch fixes, on top of FgRt for the joint count of this launch.
template <int VP_> struct FgGeo : FgRt {
    static constexpr bool STATIC_V = false;
    static constexpr int VP = VP_;
    static constexpr int QF = VP / 4;                  // 16-byte pieces per frame
    static constexpr int NC = F2_BT * VP;              // columns of a tile
    static constexpr int NCT = NC / 16;                // MFMA column tiles
    static constexpr int PB = NC + 4;                  // tile pitch: the four k rows of a fragment read sit 16 banks apart
    static constexpr int PH = F2_HF * VP + 4;          // halo tile pitch
    static constexpr int NIT = ((VP * VP + 15) / 16 + 3) / 4;   // E column tiles per wave at V = VP
    static constexpr int NB = VP / 4;                  // 64 * VP / 256: pq elements per thread at R = 32, V = VP
    static_assert(VP % 4 == 0 && VP >= 8 && VP <= 28 && NC % 16 == 0, "geometry: whole MFMA tiles, xbar in two tiles");
    static_assert((4 * PB) % 64 == 16, "conflict-free pitch");
    int KC;                                            // K rows of a staged chunk of the gcn stage (the other stages: unused)
    __device__ FgGeo(int V, int kc = F2_KC) : FgRt(V, VP_), KC(kc) {}
};

// The kernel arguments: f2_common.h's fields and V, kc, in the order this family's kernels have always read them.
struct FgGcnArgs {
    int N, Cin, Cout, T, V, S, R, res_mode;
    const float *x, *w12, *b12, *w4, *b4, *A, *alpha, *w3, *b3, *sy, *ty, *wd, *bd, *xpart;
    float *E, *sum, *diff;
    int vec12, vec4, vec3, vecd;
    int ntp;                             // f2g_e: frame phases of the xbar sum (4, or 2 where 4 partial tiles do not fit LDS)
    int kc;                              // f2g_gcn: K rows of a staged chunk (a multiple of 16, <= F2_KC)
};
struct FgGemmArgs {
    int N, K, M, T, V, mode, relu_rows, vec;
    const float *x, *w, *b, *add;
    float* out;
};
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

template <int VP> __global__ __launch_bounds__(F2_NT) void f2g_e_kernel(const FgGcnArgs a) { f2x_e_body(FgGeo<VP>(a.V), a); }
// (the chunk clamped to K: the loop then steps by what it stages, the form this family's gcn kernels were measured in)
template <int VP> __global__ __launch_bounds__(F2_NT) void f2g_gcn_kernel(const FgGcnArgs a) {
    f2x_gcn_body(FgGeo<VP>(a.V, min(a.kc, (a.Cin + 15) & ~15)), a);
}
template <int VP> __global__ __launch_bounds__(F2_NT) void f2g_gemm_kernel(const FgGemmArgs a) { f2x_gemm_body(FgGeo<VP>(a.V), a); }
template <int VP> __global__ __launch_bounds__(F2_NT) void f2g_tcn_kernel(const FgTcnArgs a) { f2x_tcn_body(FgGeo<VP>(a.V), a, 0); }

// ---- host -----------------------------------------------------------------------------------------------------------
#define FG_PITCHES(X) X(8) X(12) X(16) X(20) X(24) X(28)
#define FG_SERVES "this family serves 8 <= V <= 28, S = 3"

bool fg_served(int V) { return V >= FG_VMIN && V <= FG_VMAX; }
inline int fg_vp(int V) { return (V + 3) & ~3; }
const F2Family FG_FAMILY = {fg_served, FG_SERVES, "null descriptor (V=n/a; " FG_SERVES ")", 4, F2_GCN_ALIGN4_TXT, F2_TCN_ALIGN4_TXT, false};

// The LDS requests, from the joint count: f2_common.h's formulas at this geometry's pitches.
size_t fg_e_lds(int V, int Cin, int R, int ntp) { return f2_e_lds(Cin, R, ntp, fg_vp(V), FgRt(V, fg_vp(V)).PD); }
int fg_e_ntp(int V, int Cin, int R) { return fg_e_lds(V, Cin, R, 4) <= F2_LDS_MAX ? 4 : 2; }
size_t fg_gcn_lds(int V, int Cin, int kc) { return f2_gcn_lds(Cin, kc, F2_BT * fg_vp(V) + 4, FgRt(V, fg_vp(V)).ES); }
// the K chunk: the largest multiple of 16 up to F2_KC with which the stage fits (112 rows at V = 28, F2_KC below)
int fg_gcn_kc(int V, int Cin) {
    int kc = F2_KC;
    while (kc > 16 && fg_gcn_lds(V, Cin, kc) > F2_LDS_MAX) kc -= 16;
    return kc;
}
size_t fg_gemm_lds(int V, int K) { return f2_gemm_lds(K, F2_BT * fg_vp(V) + 4); }
size_t fg_tcn_lds(int V, int Cin, int Cb, int res_mode) { return f2_tcn_lds(Cin, Cb, res_mode, F2_BT * fg_vp(V) + 4, F2_HF * fg_vp(V) + 4); }

#define FG_LAUNCH_CASE(p) case p: tg_launch_lds<FG_KERNEL<p>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a); break;

int fg_e_launch(const tamgcn_f2_gcn_desc* d, void* stream, const char* who) {
    FgGcnArgs a;
    if (f2_gcn_args(d, &a, FG_FAMILY, false, who)) return -1;
    a.V = d->V;
    a.kc = F2_KC;
    a.ntp = fg_e_ntp(d->V, d->Cin, d->R);
    const size_t lds = fg_e_lds(d->V, d->Cin, d->R, a.ntp);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
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
    if (f2_gcn_args(d, &a, FG_FAMILY, true, who)) return -1;
    a.V = d->V;
    a.kc = fg_gcn_kc(d->V, d->Cin);
    const size_t lds = fg_gcn_lds(d->V, d->Cin, a.kc);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(ceil_div(d->T, F2_BT) * (d->Cout / F2_CT), d->N);
#define FG_KERNEL f2g_gcn_kernel
    switch (fg_vp(d->V)) { FG_PITCHES(FG_LAUNCH_CASE) }
#undef FG_KERNEL
    tamgcn_note_kernel("f2g_gcn_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int fg_gemm_launch(const tamgcn_f2_gemm_desc* d, void* stream, const char* who) {
    FgGemmArgs a;
    if (f2_gemm_args(d, &a, FG_FAMILY, who)) return -1;
    a.V = d->V;
    const size_t lds = fg_gemm_lds(d->V, d->K);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(ceil_div(d->T, F2_BT) * (d->M / 16), d->N);
#define FG_KERNEL f2g_gemm_kernel
    switch (fg_vp(d->V)) { FG_PITCHES(FG_LAUNCH_CASE) }
#undef FG_KERNEL
    tamgcn_note_kernel("f2g_gemm_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int fg_tcn_launch(const tamgcn_f2_tcn_desc* d, void* stream, const char* who) {
    FgTcnArgs a;
    if (f2_tcn_args(d, &a, FG_FAMILY, who)) return -1;
    a.V = d->V;
    const size_t lds = fg_tcn_lds(d->V, d->Cin, d->Cb, d->res_mode);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    const dim3 grid(ceil_div(a.T2, F2_BT) * (d->Cout / 16), d->N);
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
    return lds <= F2_LDS_MAX ? (int)lds : -1;
}

extern "C" int tamgcn_f2g_e(const tamgcn_f2_gcn_desc* d, void* stream) { return fg_e_launch(d, stream, "tamgcn_f2g_e"); }
extern "C" int tamgcn_f2g_gcn(const tamgcn_f2_gcn_desc* d, void* stream) { return fg_gcn_launch(d, stream, "tamgcn_f2g_gcn"); }
extern "C" int tamgcn_f2g_gemm(const tamgcn_f2_gemm_desc* d, void* stream) { return fg_gemm_launch(d, stream, "tamgcn_f2g_gemm"); }
extern "C" int tamgcn_f2g_tcn(const tamgcn_f2_tcn_desc* d, void* stream) { return fg_tcn_launch(d, stream, "tamgcn_f2g_tcn"); }
