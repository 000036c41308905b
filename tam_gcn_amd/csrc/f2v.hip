// f2v: the small-batch eval-mode TCN_GCN_unit (f2.hip's family: same four stages, same algebra, include/tamgcn.h) for
// skeletons whose joint count is NOT a multiple of four -- NTU-RGB+D's V = 25, COCO's 17, OpenPose's 18 -- with V a TEMPLATE
// PARAMETER.  The stage bodies are f2x_body.h's (its header has the layout: frames padded to VP floats, whole MFMA tiles, K in
// chunks), shared with f2g.hip; this file holds the compile-time geometry FvGeo<V>, under which every geometry value of a
// body is a constant, the kernels -- plain and grouped -- instantiated for every V of FV_JOINTS (17 = COCO / YOLO-pose,
// 18 = OpenPose, 25 = NTU-RGB+D), S = 3, and their launches.
#include "f2x_body.h"

namespace {

template <int V_> struct FvGeo {
    static constexpr bool STATIC_V = true;
    static constexpr int V = V_;
    static constexpr int VP = (V + 3) & ~3;            // floats per frame in LDS and in the family's own buffers
    static constexpr int QF = VP / 4;                  // 16-byte pieces per frame
    static constexpr int NC = F2_BT * VP;              // columns of a tile
    static constexpr int NCT = NC / 16;                // MFMA column tiles
    static constexpr int PB = NC + 4;                  // tile pitch: the four k rows of a fragment read sit 16 banks apart
    static constexpr int EC = V * VP;                  // floats of one channel of E: rows u of VP
    static constexpr int ECT = (EC + 15) / 16;         // column tiles of the E product
    static constexpr int PD = ECT * 16 + 4;            // D pitch
    static constexpr int PH = F2_HF * VP + 4;          // halo tile pitch
    static constexpr int EPC = (F2_CT * EC + 255) / 256;   // 1 KB DMA pieces of one subset's E run
    static constexpr int ES = EPC * 256;
    static constexpr int KC = F2_KC;                   // K rows of a staged chunk of the gcn stage
    static constexpr int NIT = (ECT + 3) / 4;          // E column tiles per wave
    static constexpr int NB = (64 * V + F2_NT - 1) / F2_NT;   // pq elements per thread at R = 32
    static_assert(NC % 16 == 0 && V <= 32 && V % 4 != 0, "geometry: whole MFMA tiles, xbar in two tiles, unaligned rows");
    static_assert((4 * PB) % 64 == 16 && (4 * PD) % 64 == 16, "conflict-free pitches");
    static_assert((EC * 4) % 16 == 0 && F2_CT * EC >= 256, "E runs are 16-byte aligned");
};

template <int V> __global__ __launch_bounds__(F2_NT) void f2v_e_kernel(const F2GcnArgs a) { f2x_e_body(FvGeo<V>(), a); }
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_e_grouped_kernel(const F2GcnArgs a, int npg) {
    f2x_e_body(FvGeo<V>(), f2_group(a, blockIdx.y / npg, V * V));
}
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_gcn_kernel(const F2GcnArgs a) { f2x_gcn_body(FvGeo<V>(), a); }
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_gcn_grouped_kernel(const F2GcnArgs a, int npg) {
    f2x_gcn_body(FvGeo<V>(), f2_group(a, blockIdx.y / npg, V * V));
}
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_gemm_kernel(const F2GemmArgs a) { f2x_gemm_body(FvGeo<V>(), a); }
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_gemm_grouped_kernel(const F2GemmArgs a, int npg) {
    f2x_gemm_body(FvGeo<V>(), f2_group(a, blockIdx.y / npg));
}
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_tcn_kernel(const F2TcnArgs a) { f2x_tcn_body(FvGeo<V>(), a, 0); }
template <int V> __global__ __launch_bounds__(F2_NT) void f2v_tcn_grouped_kernel(const F2TcnArgs a, int npg) {
    f2x_tcn_body(FvGeo<V>(), a, blockIdx.y / npg);
}

// ---- host -----------------------------------------------------------------------------------------------------------
// The joint counts the family is instantiated for: THE list (tam_gcn_amd/f2v.py mirrors it as JOINTS).  Serving another
// skeleton with V % 4 != 0 is one more X(..) here -- after reading FvGeo's asserts and f2x_stage's `last` for that V.
#define FV_JOINTS(X) X(17) X(18) X(25)

constexpr int FV_V = 25;                               // the widest geometry of the list: what F2_LDS_MAX has to hold (asserted below)

#define FV_JOINT_TXT(v) " V = " #v ","
#define FV_BUILT_FOR "this family is built for" FV_JOINTS(FV_JOINT_TXT) " S = 3"

// Everything of the host half that depends on the geometry: the LDS requests and the launches, per served V.
// groups == 0: the plain entry point; otherwise the grouped one.
template <int V> struct FvHost {
using GV = FvGeo<V>;

static constexpr size_t fv_e_lds(int Cin, int R, int ntp) { return f2_e_lds(Cin, R, ntp, GV::VP, GV::PD); }
static constexpr size_t fv_gcn_lds(int Cin) { return f2_gcn_lds(Cin, GV::KC, GV::PB, GV::ES); }
static constexpr size_t fv_gemm_lds(int K) { return f2_gemm_lds(K, GV::PB); }
static constexpr size_t fv_tcn_lds(int Cin, int Cb, int res_mode) { return f2_tcn_lds(Cin, Cb, res_mode, GV::PB, GV::PH); }

static int fv_e_launch(F2GcnArgs& a, int groups, void* stream, const char* who) {
    a.ntp = fv_e_lds(a.Cin, a.R, 4) <= F2_LDS_MAX ? 4 : 2;
    const size_t lds = fv_e_lds(a.Cin, a.R, a.ntp);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    if (f2_gcn_groups_ok(a, groups, who)) return -1;
    const dim3 grid(a.S * (a.Cout / 16), a.N);
    if (groups) {
        tg_launch_lds<f2v_e_grouped_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a, a.N / groups);
        tamgcn_note_kernel("f2v_e_grouped_kernel");
    } else {
        tg_launch_lds<f2v_e_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a);
        tamgcn_note_kernel("f2v_e_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

static int fv_gcn_launch(F2GcnArgs& a, int groups, void* stream, const char* who) {
    const size_t lds = fv_gcn_lds(a.Cin);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    if (f2_gcn_groups_ok(a, groups, who)) return -1;
    const dim3 grid(ceil_div(a.T, F2_BT) * (a.Cout / F2_CT), a.N);
    if (groups) {
        tg_launch_lds<f2v_gcn_grouped_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a, a.N / groups);
        tamgcn_note_kernel("f2v_gcn_grouped_kernel");
    } else {
        tg_launch_lds<f2v_gcn_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a);
        tamgcn_note_kernel("f2v_gcn_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

static int fv_gemm_launch(F2GemmArgs& a, int groups, void* stream, const char* who) {
    const size_t lds = fv_gemm_lds(a.K);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    if (f2_gemm_groups_ok(a, groups, who)) return -1;
    const dim3 grid(ceil_div(a.T, F2_BT) * (a.M / 16), a.N);
    if (groups) {
        tg_launch_lds<f2v_gemm_grouped_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a, a.N / groups);
        tamgcn_note_kernel("f2v_gemm_grouped_kernel");
    } else {
        tg_launch_lds<f2v_gemm_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a);
        tamgcn_note_kernel("f2v_gemm_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}

static int fv_tcn_launch(F2TcnArgs& a, int groups, void* stream, const char* who) {
    const size_t lds = fv_tcn_lds(a.Cin, a.Cb, a.res_mode);
    TG_CHECK(lds <= F2_LDS_MAX, "%s: %zu bytes of LDS", who, lds);
    if (f2_tcn_groups_ok(a, groups, who)) return -1;
    const dim3 grid(ceil_div(a.T2, F2_BT) * (a.Cout / 16), a.N);
    if (groups) {
        tg_launch_lds<f2v_tcn_grouped_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a, a.N / groups);
        tamgcn_note_kernel("f2v_tcn_grouped_kernel");
    } else {
        tg_launch_lds<f2v_tcn_kernel<V>>(F2_LDS_MAX, grid, dim3(F2_NT), lds, (hipStream_t)stream, a);
        tamgcn_note_kernel("f2v_tcn_kernel");
    }
    TG_LAUNCH_CHECK(who);
    return 0;
}
};  // FvHost

static_assert(FvHost<FV_V>::fv_e_lds(256, 32, 2) <= F2_LDS_MAX && FvHost<FV_V>::fv_gcn_lds(256) <= F2_LDS_MAX &&
              FvHost<FV_V>::fv_gemm_lds(256) <= F2_LDS_MAX && FvHost<FV_V>::fv_tcn_lds(256, 64, 2) <= F2_LDS_MAX,
              "the widest served geometry fits the LDS cap at the stock model's widest layers");

// One row of launchers per served joint count; the entry points pick theirs by d->V.  Any other V is refused on the host
// (f2_common.h: right after the null descriptor, before a pointer of the descriptor is looked at).
struct FvRow {
    int V;
    int (*e)(F2GcnArgs&, int, void*, const char*);
    int (*gcn)(F2GcnArgs&, int, void*, const char*);
    int (*gemm)(F2GemmArgs&, int, void*, const char*);
    int (*tcn)(F2TcnArgs&, int, void*, const char*);
};
#define FV_ROW(v) {v, FvHost<v>::fv_e_launch, FvHost<v>::fv_gcn_launch, FvHost<v>::fv_gemm_launch, FvHost<v>::fv_tcn_launch},
const FvRow FV_ROWS[] = {FV_JOINTS(FV_ROW)};

const FvRow* fv_row(int V) {
    for (const FvRow& r : FV_ROWS)
        if (r.V == V) return &r;
    return nullptr;
}
bool fv_served(int V) { return fv_row(V) != nullptr; }
const F2Family FV_FAMILY = {fv_served, FV_BUILT_FOR, "null pointer", 4, F2_GCN_ALIGN4_TXT, F2_TCN_ALIGN4_TXT, false};

int fv_e_launch(const tamgcn_f2_gcn_desc* d, int groups, void* stream, const char* who) {
    F2GcnArgs a;
    return f2_gcn_args(d, &a, FV_FAMILY, false, who) ? -1 : fv_row(d->V)->e(a, groups, stream, who);
}
int fv_gcn_launch(const tamgcn_f2_gcn_desc* d, int groups, void* stream, const char* who) {
    F2GcnArgs a;
    return f2_gcn_args(d, &a, FV_FAMILY, true, who) ? -1 : fv_row(d->V)->gcn(a, groups, stream, who);
}
int fv_gemm_launch(const tamgcn_f2_gemm_desc* d, int groups, void* stream, const char* who) {
    F2GemmArgs a;
    return f2_gemm_args(d, &a, FV_FAMILY, who) ? -1 : fv_row(d->V)->gemm(a, groups, stream, who);
}
int fv_tcn_launch(const tamgcn_f2_tcn_desc* d, int groups, void* stream, const char* who) {
    F2TcnArgs a;
    return f2_tcn_args(d, &a, FV_FAMILY, who) ? -1 : fv_row(d->V)->tcn(a, groups, stream, who);
}

}  // namespace

extern "C" int tamgcn_f2v_e(const tamgcn_f2_gcn_desc* d, void* stream) { return fv_e_launch(d, 0, stream, "tamgcn_f2v_e"); }
extern "C" int tamgcn_f2v_gcn(const tamgcn_f2_gcn_desc* d, void* stream) { return fv_gcn_launch(d, 0, stream, "tamgcn_f2v_gcn"); }
extern "C" int tamgcn_f2v_gemm(const tamgcn_f2_gemm_desc* d, void* stream) { return fv_gemm_launch(d, 0, stream, "tamgcn_f2v_gemm"); }
extern "C" int tamgcn_f2v_tcn(const tamgcn_f2_tcn_desc* d, void* stream) { return fv_tcn_launch(d, 0, stream, "tamgcn_f2v_tcn"); }

extern "C" int tamgcn_f2v_e_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2v_e_grouped") ? -1 : fv_e_launch(d, groups, stream, "tamgcn_f2v_e_grouped");
}
extern "C" int tamgcn_f2v_gcn_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2v_gcn_grouped") ? -1 : fv_gcn_launch(d, groups, stream, "tamgcn_f2v_gcn_grouped");
}
extern "C" int tamgcn_f2v_gemm_grouped(const tamgcn_f2_gemm_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2v_gemm_grouped") ? -1 : fv_gemm_launch(d, groups, stream, "tamgcn_f2v_gemm_grouped");
}
extern "C" int tamgcn_f2v_tcn_grouped(const tamgcn_f2_tcn_desc* d, int groups, void* stream) {
    return f2_groups_arg(groups, "tamgcn_f2v_tcn_grouped") ? -1 : fv_tcn_launch(d, groups, stream, "tamgcn_f2v_tcn_grouped");
}
