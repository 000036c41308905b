// f2s: the eval-mode st_gcn block (models/stgcn.py) for small batches -- two launches per block (include/tamgcn.h "f2s").
//
//   tamgcn_f2s_gcn   h = relu( sum_k (Wg_k x) Ae_k + bg )          graph convolution, tcn.0 (BatchNorm) and the ReLU folded
//   tamgcn_f2s_tcn   out = relu( Wt * h + bt + res )               9 x 1 temporal conv, tcn.3 folded, residual, ReLU
//   tamgcn_f2s_gcn_grouped, tamgcn_f2s_tcn_grouped                 the same for `groups` models of one geometry in one launch
//                                                                  (include/tamgcn.h "f2s grouped"): the same kernel text, GROUPED
//
// Both are GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32) whose columns are the FLAT (frame, joint) index of a frame tile:
// x, h and out are contiguous (N, C, T, V), so the 16 columns of a B fragment are 16 consecutive floats of a channel row
// whatever V is -- no joint padding in HBM and none in the GEMM.  A temporal tap is a shift of that flat index by a
// multiple of V.  A workgroup (four waves) owns 16 output channels x one tile of `tf` frames (at most 64 columns: four
// 16-column pieces) of one sample.  At one clip there are far fewer workgroups than CUs and a workgroup's time is a chain
// of memory latencies, so the CONTRACTION is what the four waves split: wave w takes the chunks w, w + 4, ... of the
// contraction index for all column pieces, its operand registers ping-pong over two chunks (the next chunk's 17 loads are
// issued before the current chunk's MFMAs: 17..34 independent loads in flight per wave), and the four partial tiles are
// added in LDS in wave order -- a fixed order: two launches are bit-equal.  Weights are read as A fragments straight from L2, a float4 per lane (MFMA step j
// contracts index 4*(lane>>4) + j of a 16-index chunk; both operands agree); the activations are read as B fragments
// straight from L2 as well: no element is needed twice by one wave except through the taps, which the vector cache
// serves, so the 393 KB tcn tile of a 256-channel block is never staged anywhere.
//
// The gcn kernel contracts the channels first (y_k = Wg_k x, K accumulators per column piece), leaves y in LDS with
// frames padded to VP = (V + 3) & ~3 floats (pads zero), and contracts the joints there: rows (channel, frame), A = y_k,
// B = Ae_k from LDS (rows >= V and columns >= V zero).  No atomics.  Every store is masked to its array and every load whose
// index falls outside reads element 0 of the same array instead (fs_load_b) and contributes zero: nothing is read or
// written past an operand.
#include "f2s_common.h"

namespace {

// npg: samples per group of a grouped launch (include/tamgcn.h "f2s grouped"); the plain kernels do not read it
struct FsGcnArgs {
    int N, Cin, Cout, T, V, tf, npg;
    bool vec;
    const float* x; const float* Ae; const float* wg; const float* bg;
    float* h;
};

// GROUPED: samples [g npg, (g + 1) npg) read the g-th of the parameter arrays that follow one another densely behind group 0's.
// g comes from blockIdx.z alone, so the offset bases stay scalar; everything below is the plain kernel's.
template <int K, bool GROUPED>
__global__ __launch_bounds__(FS_NT) void f2s_gcn_kernel(FsGcnArgs a) {
    __shared__ float ys[K * FS_CT * FS_YP];
    __shared__ float as[K * 32 * FS_AP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V, VP = (V + 3) & ~3, Cin = a.Cin, T = a.T;
    const int t0 = blockIdx.x * a.tf, c0 = blockIdx.y * FS_CT, n = blockIdx.z;
    const int tf = min(a.tf, T - t0);
    const int ncols = tf * V;
    if (GROUPED) {
        const int g = n / a.npg;
        a.Ae += g * K * V * V;
        a.wg += (long long)g * K * a.Cout * Cin;
        a.bg += g * a.Cout * V;
    }

    // Ae -> LDS, zero outside V x V; y's rows zeroed (the pad joints stay zero, the partial sums start from zero)
    for (int i = tid; i < K * 32 * FS_AP; i += FS_NT) {
        const int k = i / (32 * FS_AP), r = (i / FS_AP) % 32, w = i % FS_AP;
        as[i] = (r < V && w < V) ? a.Ae[(k * V + r) * V + w] : 0.f;
    }
    for (int i = tid; i < K * FS_CT * FS_YP; i += FS_NT) ys[i] = 0.f;

    // ---- y_k[c][col] = sum_ci Wg[k][c0 + c][ci] x[n][ci][t0*V + col]: wave w contracts the chunks w, w + 4, ... -----------
    const float* xn = a.x + ((long long)n * Cin * T + t0) * V;
    const long long xrow = (long long)T * V;
    int col[FS_NP]; bool cok[FS_NP];
#pragma unroll
    for (int p = 0; p < FS_NP; ++p) {
        col[p] = p * 16 + li;
        cok[p] = col[p] < ncols;
    }
    f32x4 acc[K][FS_NP];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int p = 0; p < FS_NP; ++p) acc[k][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nchunk = (Cin + 15) >> 4;
    if (wave < nchunk) {
        const float* wrow[K];
#pragma unroll
        for (int k = 0; k < K; ++k) wrow[k] = a.wg + ((long long)k * a.Cout + c0 + li) * Cin;
        f32x4 A0[K], A1[K];
        float B0[FS_NP][4], B1[FS_NP][4];
        auto fetch = [&](int ch, f32x4(&Ao)[K], float(&Bo)[FS_NP][4]) {      // a chunk past the end loads element 0 and gives zeros
            const int base = ch * 16 + 4 * kq;
#pragma unroll
            for (int k = 0; k < K; ++k) Ao[k] = fs_load_a(wrow[k], base, Cin, a.vec);
#pragma unroll
            for (int p = 0; p < FS_NP; ++p)
#pragma unroll
                for (int j = 0; j < 4; ++j) Bo[p][j] = fs_load_b(xn, (base + j) * xrow + col[p], cok[p] && base + j < Cin);
        };
        auto mma = [&](const f32x4(&Ai)[K], const float(&Bi)[FS_NP][4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int p = 0; p < FS_NP; ++p) acc[k][p] = mfma16(Ai[k][j], Bi[p][j], acc[k][p]);
        };
        fetch(wave, A0, B0);
        for (int ch = wave; ch < nchunk; ch += 8) {                          // two chunks per pass, the operands ping-pong
            fetch(ch + 4, A1, B1);
            mma(A0, B0);
            fetch(ch + 8, A0, B0);
            mma(A1, B1);
        }
    }
    // the four partial tiles are added into y in wave order (a wave without a chunk adds nothing)
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w && wave < nchunk) {
#pragma unroll
            for (int p = 0; p < FS_NP; ++p)
                if (cok[p]) {
                    const int t = col[p] / V, v = col[p] - t * V;
#pragma unroll
                    for (int k = 0; k < K; ++k)
#pragma unroll
                        for (int r = 0; r < 4; ++r) ys[(k * FS_CT + 4 * kq + r) * FS_YP + t * VP + v] += acc[k][p][r];
                }
        }
    }
    __syncthreads();

    // ---- h[c][t][w] = relu( sum_k sum_v y_k[c][t][v] Ae[k][v][w] + bg[c][w] ): one frame per wave and pass ---------------
    const int nw = (V + 15) >> 4;                                            // 16-column pieces of w: 1 or 2
    for (int t = wave; t < tf; t += 4) {
        f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < K; ++k)
            for (int v0 = 0; v0 < VP; v0 += 4) {
                const float av = ys[(k * FS_CT + li) * FS_YP + t * VP + v0 + kq];
                const float* br = as + (k * 32 + v0 + kq) * FS_AP + li;
                o[0] = mfma16(av, br[0], o[0]);
                if (nw > 1) o[1] = mfma16(av, br[16], o[1]);
            }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int w = p * 16 + li;
            if (p < nw && w < V) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = c0 + 4 * kq + r;
                    a.h[(((long long)n * a.Cout + c) * T + t0 + t) * V + w] = fmaxf(o[p][r] + a.bg[c * V + w], 0.f);
                }
            }
        }
    }
}

struct FsTcnArgs {
    int N, Cin, Cout, T, T2, V, stride, res_mode, tf, npg;
    bool vect, vecr;
    const float* h; const float* wt; const float* bt; const float* x; const float* wr; const float* br;
    float* out;
};

template <bool GROUPED>
__global__ __launch_bounds__(FS_NT) void f2s_tcn_kernel(FsTcnArgs a) {
    __shared__ float red[FS_CT * FS_RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V, T = a.T, C = a.Cout, s = a.stride;
    const int t0 = blockIdx.x * a.tf, c0 = blockIdx.y * FS_CT, n = blockIdx.z;
    const int tf = min(a.tf, a.T2 - t0);
    const int ncols = tf * V;
    if (GROUPED) {                                                           // as in f2s_gcn_kernel
        const int g = n / a.npg;
        a.wt += (long long)g * C * C * FS_KT;
        a.bt += g * C;
        if (a.res_mode == 2) {
            a.wr += (long long)g * C * a.Cin;
            a.br += g * C;
        }
    }

    int col[FS_NP], fr0[FS_NP], off0[FS_NP]; bool cok[FS_NP];
#pragma unroll
    for (int p = 0; p < FS_NP; ++p) {
        col[p] = p * 16 + li;
        cok[p] = col[p] < ncols;
        const int tl = col[p] / V, v = col[p] - tl * V;
        fr0[p] = (t0 + tl) * s - (FS_KT - 1) / 2;                            // frame of tap 0
        off0[p] = fr0[p] * V + v;                                            // ... and its offset in a channel row of h
    }
    f32x4 acc[FS_NP];
#pragma unroll
    for (int p = 0; p < FS_NP; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long hrow = (long long)T * V;

    // ---- sum over q = c' * 9 + tap of Wt[c][q] * h[n][c'][frame(tap)][v]: wave w contracts the chunks w, w + 4, ... --------
    {
        const int Q = C * FS_KT;                                             // a multiple of 16
        const float* wrow = a.wt + (long long)(c0 + li) * Q;
        const float* hn = a.h + (long long)n * C * hrow;
        f32x4 A0, A1;
        float B0[FS_NP][4], B1[FS_NP][4];
        auto fetch = [&](int ch, f32x4& Ao, float(&Bo)[FS_NP][4]) {          // a chunk past the end loads element 0 and gives zeros
            const int base = ch * 16 + 4 * kq;
            Ao = fs_load_a(wrow, base, Q, a.vect);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = base + j, cp = q / FS_KT, tap = q - cp * FS_KT;
#pragma unroll
                for (int p = 0; p < FS_NP; ++p)
                    Bo[p][j] = fs_load_b(hn, cp * hrow + off0[p] + tap * V, q < Q && cok[p] && (unsigned)(fr0[p] + tap) < (unsigned)T);
            }
        };
        auto mma = [&](const f32x4& Ai, const float(&Bi)[FS_NP][4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < FS_NP; ++p) acc[p] = mfma16(Ai[j], Bi[p][j], acc[p]);
        };
        const int nchunk = Q >> 4;                                           // >= 9
        fetch(wave, A0, B0);
        for (int ch = wave; ch < nchunk; ch += 8) {                          // two chunks per pass, the operands ping-pong
            fetch(ch + 4, A1, B1);
            mma(A0, B0);
            fetch(ch + 8, A0, B0);
            mma(A1, B1);
        }
    }
    // ---- the strided 1 x 1 residual conv: + sum_ci Wr[c][ci] x[n][ci][tau*s][v], chunks split the same way ------------------
    const long long xrow = (long long)T * V;
    if (a.res_mode == 2) {
        const int Cin = a.Cin;
        const float* wrow = a.wr + (long long)(c0 + li) * Cin;
        const float* xn = a.x + (long long)n * Cin * xrow;
        for (int ch = wave; ch < ((Cin + 15) >> 4); ch += 4) {
            const int base = ch * 16 + 4 * kq;
            const f32x4 A = fs_load_a(wrow, base, Cin, a.vecr);
            float B[FS_NP][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < FS_NP; ++p)                               // frame tau*s: always inside [0, T)
                    B[p][j] = fs_load_b(xn, (base + j) * xrow + off0[p] + ((FS_KT - 1) / 2) * V, cok[p] && base + j < Cin);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < FS_NP; ++p)
                    acc[p] = mfma16(A[j], B[p][j], acc[p]);
        }
    }
    // ---- the four partial tiles are added in LDS in wave order ----------------------------------------------------------------
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int p = 0; p < FS_NP; ++p)
                if (cok[p]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* d = red + (4 * kq + r) * FS_RP + col[p];
                        *d = w == 0 ? acc[p][r] : *d + acc[p][r];
                    }
                }
        }
        __syncthreads();
    }
    // ---- + bt (+ br) + identity residual, ReLU: 16 channels x ncols, consecutive threads on consecutive columns ---------------
    for (int i = tid; i < FS_CT * FS_MAXCOLS; i += FS_NT) {
        const int cl = i / FS_MAXCOLS, cc = i - cl * FS_MAXCOLS;
        if (cc < ncols) {
            const int c = c0 + cl;
            const long long o = (((long long)n * C + c) * a.T2 + t0) * V + cc;
            float v = red[cl * FS_RP + cc] + a.bt[c];
            if (a.res_mode == 2) v += a.br[c];
            if (a.res_mode == 1) v += a.x[o];                                // stride 1, Cin == Cout: x has out's layout
            a.out[o] = fmaxf(v, 0.f);
        }
    }
}

}  // namespace

extern "C" int tamgcn_f2s_supported(int V, int K, int Cin, int Cout, int KT, int stride) { return fs_geometry_ok(V, K, Cin, Cout, KT, stride); }

namespace {

// groups == 0: the plain entry point; otherwise the grouped one (d->N the total, every check on the total).
int fs_groups_ok(int N, int groups, const char* who) {
    TG_CHECK(groups >= 1 && N % groups == 0, "%s: N=%d is not a multiple of groups=%d", who, N, groups);
    return 0;
}
int fs_group_stride_ok(bool vec, long long stride, const char* who, const char* what) {
    TG_CHECK(!vec || stride % 4 == 0, "%s: group stride of %s (%lld floats) breaks the 16-byte alignment of its vector path", who, what, stride);
    return 0;
}

template <int K>
void fs_gcn_run(const FsGcnArgs& a, bool grouped, const dim3& grid, hipStream_t st) {
    if (grouped) hipLaunchKernelGGL((f2s_gcn_kernel<K, true>), grid, dim3(FS_NT), 0, st, a);
    else hipLaunchKernelGGL((f2s_gcn_kernel<K, false>), grid, dim3(FS_NT), 0, st, a);
}

int fs_gcn_launch(const tamgcn_f2s_gcn_desc* d, int groups, void* stream, const char* who) {
    TG_CHECK(d, "%s: null descriptor", who);
    TG_CHECK(d->x && d->Ae && d->wg && d->bg && d->h, "%s: null pointer", who);
    TG_CHECK(d->N >= 1 && d->T >= 1 && d->N <= 65535, "%s: bad dims N=%d T=%d", who, d->N, d->T);
    TG_CHECK(fs_geometry_ok(d->V, d->K, d->Cin, d->Cout, FS_KT, 1),
             "%s: V=%d K=%d Cin=%d Cout=%d outside 2 <= V <= 32, 1 <= K <= 3, 1 <= Cin <= 256, Cout %% 16 == 0, Cout <= 256", who, d->V, d->K,
             d->Cin, d->Cout);
    TG_CHECK((long long)d->N * (d->Cin > d->Cout ? d->Cin : d->Cout) * d->T * d->V < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    FsGcnArgs a;
    a.N = d->N; a.Cin = d->Cin; a.Cout = d->Cout; a.T = d->T; a.V = d->V; a.tf = fs_tf(d->V);
    a.vec = d->Cin % 4 == 0 && fs_al16(d->wg);
    if (groups && (fs_groups_ok(d->N, groups, who) || fs_group_stride_ok(a.vec, (long long)d->K * d->Cout * d->Cin, who, "wg"))) return -1;
    a.npg = groups ? d->N / groups : d->N;
    a.x = d->x; a.Ae = d->Ae; a.wg = d->wg; a.bg = d->bg; a.h = d->h;
    const dim3 grid(ceil_div(d->T, a.tf), d->Cout / FS_CT, d->N);
    if (d->K == 1) fs_gcn_run<1>(a, groups != 0, grid, (hipStream_t)stream);
    else if (d->K == 2) fs_gcn_run<2>(a, groups != 0, grid, (hipStream_t)stream);
    else fs_gcn_run<3>(a, groups != 0, grid, (hipStream_t)stream);
    tamgcn_note_kernel(groups ? "f2s_gcn_grouped_kernel<%d>" : "f2s_gcn_kernel<%d>", d->K);
    TG_LAUNCH_CHECK(who);
    return 0;
}

int fs_tcn_launch(const tamgcn_f2s_tcn_desc* d, int groups, void* stream, const char* who) {
    TG_CHECK(d, "%s: null descriptor", who);
    TG_CHECK(d->h && d->wt && d->bt && d->out, "%s: null pointer", who);
    TG_CHECK(d->N >= 1 && d->T >= 1 && d->N <= 65535, "%s: bad dims N=%d T=%d", who, d->N, d->T);
    TG_CHECK(d->res_mode >= 0 && d->res_mode <= 2, "%s: res_mode=%d outside 0..2", who, d->res_mode);
    const int Cin = d->res_mode == 2 ? d->Cin : d->Cout;
    TG_CHECK(fs_geometry_ok(d->V, 1, Cin, d->Cout, d->KT, d->stride),
             "%s: V=%d Cin=%d Cout=%d KT=%d stride=%d outside 2 <= V <= 32, 1 <= Cin <= 256, Cout %% 16 == 0, Cout <= 256, KT == 9, stride 1 | 2",
             who, d->V, Cin, d->Cout, d->KT, d->stride);
    TG_CHECK(d->res_mode == 0 || d->x, "%s: res_mode=%d needs x", who, d->res_mode);
    TG_CHECK(d->res_mode != 1 || d->stride == 1, "%s: the identity residual (x of out's shape) needs stride 1", who);
    TG_CHECK(d->res_mode != 2 || (d->wr && d->br), "%s: res_mode=2 needs wr and br", who);
    TG_CHECK((long long)d->N * (Cin > d->Cout ? Cin : d->Cout) * d->T * d->V < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    FsTcnArgs a;
    a.N = d->N; a.Cin = Cin; a.Cout = d->Cout; a.T = d->T; a.T2 = (d->T - 1) / d->stride + 1; a.V = d->V; a.stride = d->stride;
    a.res_mode = d->res_mode; a.tf = fs_tf(d->V);
    a.vect = fs_al16(d->wt);                                                 // rows of 9 * Cout floats: a multiple of 16
    a.vecr = d->res_mode == 2 && Cin % 4 == 0 && fs_al16(d->wr);
    if (groups && (fs_groups_ok(d->N, groups, who) || fs_group_stride_ok(a.vect, (long long)d->Cout * d->Cout * FS_KT, who, "wt") ||
                   fs_group_stride_ok(a.vecr, (long long)d->Cout * Cin, who, "wr")))
        return -1;
    a.npg = groups ? d->N / groups : d->N;
    a.h = d->h; a.wt = d->wt; a.bt = d->bt; a.x = d->x; a.wr = d->wr; a.br = d->br; a.out = d->out;
    const dim3 grid(ceil_div(a.T2, a.tf), d->Cout / FS_CT, d->N);
    if (groups) hipLaunchKernelGGL(f2s_tcn_kernel<true>, grid, dim3(FS_NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(f2s_tcn_kernel<false>, grid, dim3(FS_NT), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel(groups ? "f2s_tcn_grouped_kernel" : "f2s_tcn_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" int tamgcn_f2s_gcn(const tamgcn_f2s_gcn_desc* d, void* stream) { return fs_gcn_launch(d, 0, stream, "tamgcn_f2s_gcn"); }
extern "C" int tamgcn_f2s_tcn(const tamgcn_f2s_tcn_desc* d, void* stream) { return fs_tcn_launch(d, 0, stream, "tamgcn_f2s_tcn"); }

// include/tamgcn.h "f2s grouped": `groups` models of one geometry in the same launch
extern "C" int tamgcn_f2s_gcn_grouped(const tamgcn_f2s_gcn_desc* d, int groups, void* stream) {
    const char* who = "tamgcn_f2s_gcn_grouped";
    TG_CHECK(groups >= 1, "%s: groups=%d", who, groups);
    return fs_gcn_launch(d, groups, stream, who);
}
extern "C" int tamgcn_f2s_tcn_grouped(const tamgcn_f2s_tcn_desc* d, int groups, void* stream) {
    const char* who = "tamgcn_f2s_tcn_grouped";
    TG_CHECK(groups >= 1, "%s: groups=%d", who, groups);
    return fs_tcn_launch(d, groups, stream, who);
}
