// f2s_bwd: the DATA gradient of the eval-mode st_gcn block (f2s.hip) for small batches -- two launches per block, in reverse
// (include/tamgcn.h "f2s backward").  In eval mode the block is piecewise linear in x with static folded weights, so its input
// gradient has the forward's shape: one 9 x 1 temporal GEMM and one graph-convolution GEMM, masked by the two ReLUs, whose
// masks are read from the tensors the forward produced (h and out).  No weight gradient is computed.
//
//   tamgcn_f2s_tcn_bwd   dh = [h > 0] * ( Wt^T (*) gz ),  gz = gout * [out > 0]        the transposed 9 x 1 conv over T2 -> T frames
//   tamgcn_f2s_gcn_bwd   dx = sum_k Wg_k^T (dh Ae_k^T) + res                            res = 0 | gz | up-sampled Wr^T gz
//
// The forward's discipline (f2s.hip): v_mfma_f32_16x16x4_f32, columns = the flat (frame, joint) index of a frame tile of the
// kernel's OUTPUT (dh, dx: T frames), a workgroup of four waves owns 16 output channels x one tile, the waves split the
// contraction (chunks w, w + 4, ...), operands ping-pong over two chunks, the four partial tiles are added in LDS in wave
// order (two launches are bit-equal), no atomics, every store masked to its array, every load whose index falls outside reads
// element 0 of its array and contributes zero.  gz is never materialised: a B fragment of it is two loads (gout, out) and a
// select on out's sign where the operand meets its MFMA (fs_load_gz / fs_gz say why not at the load).  Under stride 2 a column meets only every other tap (the others are zero operands: the strided blocks are 2 of 10).
// The weights arrive transposed (the host does that once per fold): wtb[c'][c][tap], wgb[k][ci][c], wrb[ci][c], so that an A
// fragment is again four consecutive floats of a row.  gcn_bwd's rows are the block's INPUT channels, any 1 <= Cin <= 256 (3 in
// the first block): rows >= Cin read row 0 of the weights, contribute zero and are not stored.
#include "f2s_common.h"

namespace {

// gz at index i of (gout, out) is gout[i] where ok and out[i] > 0 (strictly, as torch's ReLU backward), else zero -- in two steps.
// The loads are unconditional (index 0 where !ok) and only out's value is masked, by an index condition (fs_keep): nothing here
// depends on a loaded value, so a chunk's loads leave together.  The select on out's sign happens where the operand is used, one
// chunk later (fs_gz); done at the load it puts a full wait behind every single load.  (A 32-bit index: every tensor of a launch
// holds fewer than 2^31 elements.)
__device__ __forceinline__ void fs_load_gz(const float* __restrict__ g, const float* __restrict__ o, int i, bool ok, float& gv, float& ov) {
    const unsigned j = ok ? (unsigned)i : 0u;
    gv = g[j];
    ov = fs_keep(o[j], ok);
}
__device__ __forceinline__ float fs_gz(float gv, float ov) { return ov > 0.f ? gv : 0.f; }

struct FsTcnBwdArgs {
    int N, C, T, T2, V, stride, tf;
    bool vect;
    const float* gout; const float* out; const float* h; const float* wtb;
    float* dh;
};

// S: the temporal stride.  S = 1 (8 of 10 blocks): tau = t + 4 - tap, the forward's addressing mirrored -- one multiply per tap,
// not per element (a VALU instruction takes an MFMA's issue slot on its SIMD: the operand arithmetic is what bounds this loop).
template <int S>
__global__ __launch_bounds__(FS_NT) void f2s_tcn_bwd_kernel(FsTcnBwdArgs a) {
    __shared__ float red[FS_CT * FS_RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V, T = a.T, T2 = a.T2, C = a.C;
    const int t0 = blockIdx.x * a.tf, c0 = blockIdx.y * FS_CT, n = blockIdx.z;
    const int tf = min(a.tf, T - t0);
    const int ncols = tf * V;

    int col[FS_NP], num0[FS_NP], vj[FS_NP], off0[FS_NP]; bool cok[FS_NP];
#pragma unroll
    for (int p = 0; p < FS_NP; ++p) {
        col[p] = p * 16 + li;
        cok[p] = col[p] < ncols;
        const int tl = col[p] / V;
        vj[p] = col[p] - tl * V;
        num0[p] = t0 + tl + (FS_KT - 1) / 2;                                 // tau * s of tap 0
        off0[p] = num0[p] * V + vj[p];                                       // S = 1: tap 0's offset in a channel row of gout
    }
    f32x4 acc[FS_NP];
#pragma unroll
    for (int p = 0; p < FS_NP; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int grow = T2 * V;

    // ---- sum over q = c * 9 + tap of wtb[c'][q] * gz[n][c][(t + 4 - tap) / s][v]: wave w contracts the chunks w, w + 4, ... ----
    {
        const int Q = C * FS_KT;                                             // a multiple of 16
        const float* wrow = a.wtb + (long long)(c0 + li) * Q;
        const float* gn = a.gout + (long long)n * C * grow;                  // wave-uniform bases; the lane offsets stay below 2^31
        const float* on = a.out + (long long)n * C * grow;
        f32x4 A0, A1;
        float G0[FS_NP][4], O0[FS_NP][4], G1[FS_NP][4], O1[FS_NP][4];
        auto fetch = [&](int ch, f32x4& Ao, float(&Go)[FS_NP][4], float(&Oo)[FS_NP][4]) {      // a chunk past the end gives zeros
            const int base = ch * 16 + 4 * kq;
            Ao = fs_load_a(wrow, base, Q, a.vect);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = base + j, cc = q / FS_KT, tap = q - cc * FS_KT;
                const int crow = (int)((unsigned)cc * (unsigned)grow), cq = crow - tap * V;     // (a chunk past the end may wrap: unused)
#pragma unroll
                for (int p = 0; p < FS_NP; ++p) {
                    const int num = num0[p] - tap;                           // >= -4; an odd one meets no output frame under stride 2
                    if constexpr (S == 1) {
                        fs_load_gz(gn, on, cq + off0[p], (q < Q) & cok[p] & ((unsigned)num < (unsigned)T2), Go[p][j], Oo[p][j]);
                    } else {
                        const int tau = num >> 1;
                        fs_load_gz(gn, on, crow + tau * V + vj[p], (q < Q) & cok[p] & !(num & 1) & ((unsigned)tau < (unsigned)T2), Go[p][j], Oo[p][j]);
                    }
                }
            }
        };
        auto mma = [&](const f32x4& Ai, const float(&Gi)[FS_NP][4], const float(&Oi)[FS_NP][4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < FS_NP; ++p) acc[p] = mfma16(Ai[j], fs_gz(Gi[p][j], Oi[p][j]), acc[p]);
        };
        const int nchunk = Q >> 4;                                           // >= 9
        fetch(wave, A0, G0, O0);
        for (int ch = wave; ch < nchunk; ch += 8) {                          // two chunks per pass, the operands ping-pong
            fetch(ch + 4, A1, G1, O1);
            mma(A0, G0, O0);
            fetch(ch + 8, A0, G0, O0);
            mma(A1, G1, O1);
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
    // ---- the gcn's ReLU mask from h: 16 channels x ncols, consecutive threads on consecutive columns ---------------------------
    for (int i = tid; i < FS_CT * FS_MAXCOLS; i += FS_NT) {
        const int cl = i / FS_MAXCOLS, cc = i - cl * FS_MAXCOLS;
        if (cc < ncols) {
            const long long o = (((long long)n * C + c0 + cl) * T + t0) * V + cc;
            a.dh[o] = a.h[o] > 0.f ? red[cl * FS_RP + cc] : 0.f;
        }
    }
}

struct FsGcnBwdArgs {
    int N, Cin, Cout, T, T2, V, stride, res_mode, tf;
    bool vec, vecr;
    const float* dh; const float* Ae; const float* wgb; const float* gout; const float* out; const float* wrb;
    float* dx;
};

// RES2: the residual conv's gradient is a second accumulator of the channel contraction (it skips the joints)
template <int K, bool RES2>
__global__ __launch_bounds__(FS_NT) void f2s_gcn_bwd_kernel(FsGcnBwdArgs a) {
    constexpr int KY = K + (RES2 ? 1 : 0);
    __shared__ float ys[KY * FS_CT * FS_YP];
    __shared__ float as[K * 32 * FS_AP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V, VP = (V + 3) & ~3, Cin = a.Cin, Cout = a.Cout, T = a.T, s = a.stride;
    const int t0 = blockIdx.x * a.tf, c0 = blockIdx.y * FS_CT, n = blockIdx.z;
    const int tf = min(a.tf, T - t0);
    const int ncols = tf * V;

    // Ae^T -> LDS (as[k][w][v] = Ae[k][v][w]), zero outside V x V; y's rows zeroed (pad joints stay zero, partial sums start from zero)
    for (int i = tid; i < K * 32 * FS_AP; i += FS_NT) {
        const int k = i / (32 * FS_AP), w = (i / FS_AP) % 32, v = i % FS_AP;
        as[i] = (w < V && v < V) ? a.Ae[(k * V + v) * V + w] : 0.f;
    }
    for (int i = tid; i < KY * FS_CT * FS_YP; i += FS_NT) ys[i] = 0.f;

    // ---- y_k[ci][col] = sum_c wgb[k][c0 + ci][c] dh[n][c][t0*V + col]: wave w contracts the chunks w, w + 4, ... ----------------
    const float* dn = a.dh + ((long long)n * Cout * T + t0) * V;
    const long long drow = (long long)T * V;
    const bool rok = c0 + li < Cin;                                          // this lane's weight row exists
    const int row = rok ? c0 + li : 0;
    int col[FS_NP]; bool cok[FS_NP];
#pragma unroll
    for (int p = 0; p < FS_NP; ++p) {
        col[p] = p * 16 + li;
        cok[p] = col[p] < ncols;
    }
    f32x4 acc[KY][FS_NP];
#pragma unroll
    for (int k = 0; k < KY; ++k)
#pragma unroll
        for (int p = 0; p < FS_NP; ++p) acc[k][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nchunk = Cout >> 4;                                            // Cout % 16 == 0: >= 1
    if (wave < nchunk) {
        const float* wrow[K];
#pragma unroll
        for (int k = 0; k < K; ++k) wrow[k] = a.wgb + ((long long)k * Cin + row) * Cout;
        f32x4 A0[K], A1[K];
        float B0[FS_NP][4], B1[FS_NP][4];
        auto fetch = [&](int ch, f32x4(&Ao)[K], float(&Bo)[FS_NP][4]) {      // a chunk past the end loads element 0 and gives zeros
            const int base = ch * 16 + 4 * kq;
#pragma unroll
            for (int k = 0; k < K; ++k) Ao[k] = fs_load_a(wrow[k], base, rok ? Cout : 0, a.vec);
#pragma unroll
            for (int p = 0; p < FS_NP; ++p)
#pragma unroll
                for (int j = 0; j < 4; ++j) Bo[p][j] = fs_load_b(dn, (base + j) * drow + col[p], cok[p] && base + j < Cout);
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
        // ---- the residual conv: sum_c wrb[c0 + ci][c] gz[n][c][t / s][v] on the frames t % s == 0, chunks split the same way ----
        if constexpr (RES2) {
            const int grow = a.T2 * V;
            const float* wr = a.wrb + (long long)row * Cout;
            const float* gn = a.gout + (long long)n * Cout * grow;
            const float* on = a.out + (long long)n * Cout * grow;
            int goff[FS_NP]; bool gok[FS_NP];
#pragma unroll
            for (int p = 0; p < FS_NP; ++p) {
                const int tl = col[p] / V, v = col[p] - tl * V, t = t0 + tl;
                gok[p] = cok[p] & (t % s == 0);
                goff[p] = (t / s) * V + v;                                   // t < T: t / s < T2
            }
            for (int ch = wave; ch < nchunk; ch += 4) {
                const int base = ch * 16 + 4 * kq;
                const f32x4 A = fs_load_a(wr, base, rok ? Cout : 0, a.vecr);
                float G[FS_NP][4], O[FS_NP][4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int p = 0; p < FS_NP; ++p) fs_load_gz(gn, on, (base + j) * grow + goff[p], gok[p], G[p][j], O[p][j]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int p = 0; p < FS_NP; ++p) acc[K][p] = mfma16(A[j], fs_gz(G[p][j], O[p][j]), acc[K][p]);
            }
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
                    for (int k = 0; k < KY; ++k)
#pragma unroll
                        for (int r = 0; r < 4; ++r) ys[(k * FS_CT + 4 * kq + r) * FS_YP + t * VP + v] += acc[k][p][r];
                }
        }
    }
    __syncthreads();

    // ---- dx[ci][t][v] = sum_k sum_w y_k[ci][t][w] Ae[k][v][w] + res: one frame per wave and pass ---------------------------------
    const int nv = (V + 15) >> 4;                                            // 16-column pieces of v: 1 or 2
    for (int t = wave; t < tf; t += 4) {
        f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < K; ++k)
            for (int w0 = 0; w0 < VP; w0 += 4) {
                const float av = ys[(k * FS_CT + li) * FS_YP + t * VP + w0 + kq];
                const float* br = as + (k * 32 + w0 + kq) * FS_AP + li;
                o[0] = mfma16(av, br[0], o[0]);
                if (nv > 1) o[1] = mfma16(av, br[16], o[1]);
            }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int v = p * 16 + li;
            if (p < nv && v < V) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = c0 + 4 * kq + r;
                    if (c < Cin) {
                        const long long i = (((long long)n * Cin + c) * T + t0 + t) * V + v;
                        float val = o[p][r];
                        if constexpr (RES2) val += ys[(K * FS_CT + 4 * kq + r) * FS_YP + t * VP + v];
                        if (a.res_mode == 1) val += a.out[i] > 0.f ? a.gout[i] : 0.f;    // stride 1, Cin == Cout: gout has dx's layout
                        a.dx[i] = val;
                    }
                }
            }
        }
    }
}

template <int K>
static void fs_launch_gcn_bwd(const FsGcnBwdArgs& a, dim3 grid, hipStream_t st) {
    if (a.res_mode == 2) hipLaunchKernelGGL((f2s_gcn_bwd_kernel<K, true>), grid, dim3(FS_NT), 0, st, a);
    else hipLaunchKernelGGL((f2s_gcn_bwd_kernel<K, false>), grid, dim3(FS_NT), 0, st, a);
}

}  // namespace

extern "C" int tamgcn_f2s_tcn_bwd(const tamgcn_f2s_tcn_bwd_desc* d, void* stream) {
    const char* who = "tamgcn_f2s_tcn_bwd";
    TG_CHECK(d, "%s: null descriptor", who);
    TG_CHECK(d->gout && d->out && d->h && d->wtb && d->dh, "%s: null pointer", who);
    TG_CHECK(d->N >= 1 && d->T >= 1 && d->N <= 65535, "%s: bad dims N=%d T=%d", who, d->N, d->T);
    TG_CHECK(fs_geometry_ok(d->V, 1, d->Cout, d->Cout, d->KT, d->stride),
             "%s: V=%d Cout=%d KT=%d stride=%d outside 2 <= V <= 32, Cout %% 16 == 0, Cout <= 256, KT == 9, stride 1 | 2", who, d->V, d->Cout,
             d->KT, d->stride);
    TG_CHECK((long long)d->N * d->Cout * d->T * d->V < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    FsTcnBwdArgs a;
    a.N = d->N; a.C = d->Cout; a.T = d->T; a.T2 = (d->T - 1) / d->stride + 1; a.V = d->V; a.stride = d->stride; a.tf = fs_tf(d->V);
    a.vect = fs_al16(d->wtb);                                                // rows of 9 * Cout floats: a multiple of 16
    a.gout = d->gout; a.out = d->out; a.h = d->h; a.wtb = d->wtb; a.dh = d->dh;
    const dim3 grid(ceil_div(d->T, a.tf), d->Cout / FS_CT, d->N);
    if (d->stride == 1) hipLaunchKernelGGL(f2s_tcn_bwd_kernel<1>, grid, dim3(FS_NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(f2s_tcn_bwd_kernel<2>, grid, dim3(FS_NT), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("f2s_tcn_bwd_kernel<%d>", d->stride);
    TG_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int tamgcn_f2s_gcn_bwd(const tamgcn_f2s_gcn_bwd_desc* d, void* stream) {
    const char* who = "tamgcn_f2s_gcn_bwd";
    TG_CHECK(d, "%s: null descriptor", who);
    TG_CHECK(d->dh && d->Ae && d->wgb && d->dx, "%s: null pointer", who);
    TG_CHECK(d->N >= 1 && d->T >= 1 && d->N <= 65535, "%s: bad dims N=%d T=%d", who, d->N, d->T);
    TG_CHECK(d->res_mode >= 0 && d->res_mode <= 2, "%s: res_mode=%d outside 0..2", who, d->res_mode);
    TG_CHECK(fs_geometry_ok(d->V, d->K, d->Cin, d->Cout, FS_KT, d->stride),
             "%s: V=%d K=%d Cin=%d Cout=%d stride=%d outside 2 <= V <= 32, 1 <= K <= 3, 1 <= Cin <= 256, Cout %% 16 == 0, Cout <= 256, stride 1 | 2",
             who, d->V, d->K, d->Cin, d->Cout, d->stride);
    TG_CHECK(d->res_mode == 0 || (d->gout && d->out), "%s: res_mode=%d needs gout and out", who, d->res_mode);
    TG_CHECK(d->res_mode != 1 || (d->stride == 1 && d->Cin == d->Cout), "%s: the identity residual needs stride 1 and Cin == Cout", who);
    TG_CHECK(d->res_mode != 2 || d->wrb, "%s: res_mode=2 needs wrb", who);
    TG_CHECK((long long)d->N * (d->Cin > d->Cout ? d->Cin : d->Cout) * d->T * d->V < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    FsGcnBwdArgs a;
    a.N = d->N; a.Cin = d->Cin; a.Cout = d->Cout; a.T = d->T; a.T2 = (d->T - 1) / d->stride + 1; a.V = d->V; a.stride = d->stride;
    a.res_mode = d->res_mode; a.tf = fs_tf(d->V);
    a.vec = fs_al16(d->wgb);                                                 // rows of Cout floats: a multiple of 16
    a.vecr = d->res_mode == 2 && fs_al16(d->wrb);
    a.dh = d->dh; a.Ae = d->Ae; a.wgb = d->wgb; a.gout = d->gout; a.out = d->out; a.wrb = d->wrb; a.dx = d->dx;
    const dim3 grid(ceil_div(d->T, a.tf), ceil_div(d->Cin, FS_CT), d->N);
    if (d->K == 1) fs_launch_gcn_bwd<1>(a, grid, (hipStream_t)stream);
    else if (d->K == 2) fs_launch_gcn_bwd<2>(a, grid, (hipStream_t)stream);
    else fs_launch_gcn_bwd<3>(a, grid, (hipStream_t)stream);
    tamgcn_note_kernel("f2s_gcn_bwd_kernel<%d, %d>", d->K, d->res_mode == 2);
    TG_LAUNCH_CHECK(who);
    return 0;
}
