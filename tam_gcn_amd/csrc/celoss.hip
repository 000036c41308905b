// Cross-entropy with torch's options (include/tamgcn.h: tamgcn_ce_opts_*): class weights, ignore_index, label smoothing, the
// three reductions, class-index or class-probability targets.  The default-argument loss stays tamgcn_ce_fwd (stemhead.hip).
//
// ce_opts_rows_kernel   workgroups of CEO_ROWS waves, ONE WAVE PER ROW, rows strided over at most CEO_MAX_WG workgroups.  Lane j
//                       reads k = j, j + 64, ...: every pass over a row is contiguous.  Per row m = max_k l_k and e_k = expf(l_k - m)
//                       are fp32, as tamgcn_ce_fwd has them; EVERYTHING after them is fp64: s = sum_k e_k, lse = m + log(s),
//                       p_k = e_k / s, the coefficients, the weighted sums over k, the row loss, p_k * c - a_k and the division
//                       by the normaliser.  So the loss carries expf's error in s and one rounding to fp32, and g carries
//                       expf's error in e_k times its coefficient and one rounding.  Lane partials run over ascending k, then
//                       the xor butterfly 1, 2, 4, 8, 16, 32 (every lane ends with the same bits).
//                       'mean' over class indices divides by W = sum of w_y over the kept rows: every workgroup computes W itself
//                       from the labels (thread t takes rows t, t + 256, ...; LDS tree), the same bits in all of them, so g is
//                       final after this launch.  'none' stores the row losses as fp32; 'mean' / 'sum' store them as fp64 into the
//                       workspace.
// ce_opts_finish_kernel one workgroup: the fp64 row losses summed in a fixed order (thread t takes rows t, t + 256, ... in
//                       ascending order; LDS tree), divided by W ('mean' over indices; recomputed as above) or N (probabilities).
//                       A bad label's row holds NaN, which makes the reduced loss NaN.
// ce_opts_bwd_rows_kernel  dlogits[n][k] = g[n][k] * dloss[n]  ('none'; 'mean' / 'sum' are tamgcn_ce_bwd's one product).
// No floating-point atomics, no host synchronisation; the normaliser is read from the labels of the launch at hand.
#include "common.h"

namespace {

constexpr int CEO_NT = 256;                 // threads of a workgroup
constexpr int CEO_ROWS = CEO_NT / 64;       // rows (waves) per workgroup and pass
constexpr int CEO_MAX_WG = 256;             // workgroups of the row kernel: one per CU; N > CEO_ROWS * CEO_MAX_WG takes further passes

struct CeoArgs {
    const float* logits;
    const long long* labels;
    const float* probs;
    const float* weight;
    long long ignore_index;
    double eps;
    int reduction, N, K;
};

__device__ __forceinline__ float ceo_wave_max(float v) {
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double ceo_wave_sum(double v) {
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// W = sum over the rows with a label in [0, K) other than ignore_index of w_y (1 without weights); all threads get it
__device__ __forceinline__ double ceo_normaliser(const CeoArgs& a, double* red) {
    double w = 0.0;
    for (int n = threadIdx.x; n < a.N; n += CEO_NT) {
        const long long y = a.labels[n];
        if (y == a.ignore_index || y < 0 || y >= a.K) continue;
        w += a.weight ? (double)a.weight[y] : 1.0;
    }
    red[threadIdx.x] = w;
    __syncthreads();
    for (int o = CEO_NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(CEO_NT) void ce_opts_rows_kernel(CeoArgs a, float* loss, float* g, double* rowloss) {
    __shared__ double red[CEO_NT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int K = a.K;
    const bool index = a.labels != nullptr, smooth = a.eps > 0.0;
    double inv = 1.0;                                           // 1 / the divisor of g
    if (a.reduction == TAMGCN_CE_MEAN) inv = 1.0 / (index ? ceo_normaliser(a, red) : (double)a.N);
    const double ek = a.eps / (double)K, om = 1.0 - a.eps;
    double Wsum = (double)K;
    if (index && smooth && a.weight) {
        double ws = 0.0;
        for (int k = lane; k < K; k += 64) ws += (double)a.weight[k];
        Wsum = ceo_wave_sum(ws);
    }
    for (long long n = (long long)blockIdx.x * CEO_ROWS + wv; n < a.N; n += (long long)gridDim.x * CEO_ROWS) {
        const float* l = a.logits + n * K;
        float* gr = g + n * K;
        long long y = 0;
        if (index) {
            y = a.labels[n];
            const bool ignored = y == a.ignore_index;
            if (ignored || y < 0 || y >= K) {                   // ignored: loss 0; any other label outside [0, K): loss NaN; g = 0 in both
                for (int k = lane; k < K; k += 64) gr[k] = 0.f;
                if (lane == 0) {
                    const double v = ignored ? 0.0 : (double)__builtin_nanf("");
                    if (a.reduction == TAMGCN_CE_NONE) loss[n] = (float)v; else rowloss[n] = v;
                }
                continue;
            }
        }
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, l[k]);
        m = ceo_wave_max(m);
        double s = 0.0;
        for (int k = lane; k < K; k += 64) s += (double)expf(l[k] - m);
        s = ceo_wave_sum(s);
        const double lse = (double)m + log(s), is = 1.0 / s;
        double L;
        if (index) {
            const double cy = om * (a.weight ? (double)a.weight[y] : 1.0);
            const double c = smooth ? fma(ek, Wsum, cy) : cy;   // the coefficient of p_k
            double sm = 0.0;
            for (int k = lane; k < K; k += 64) {
                const float lk = l[k];
                const double p = (double)expf(lk - m) * is;
                double ak = k == y ? cy : 0.0;
                if (smooth) {                                   // eps = 0 never forms w_k * (lse - l_k): no 0 * inf
                    const double wk = a.weight ? (double)a.weight[k] : 1.0;
                    ak = fma(ek, wk, ak);
                    sm += wk * (lse - (double)lk);
                }
                gr[k] = (float)((p * c - ak) * inv);
            }
            L = cy * (lse - (double)l[y]);
            if (smooth) L += ek * ceo_wave_sum(sm);
        } else {
            const float* t = a.probs + n * K;
            double T = 0.0, acc = 0.0;
            for (int k = lane; k < K; k += 64) {
                const double wt = (a.weight ? (double)a.weight[k] : 1.0) * fma(om, (double)t[k], ek);
                T += wt;
                acc += wt * (lse - (double)l[k]);
            }
            T = ceo_wave_sum(T);
            L = ceo_wave_sum(acc);
            for (int k = lane; k < K; k += 64) {
                const double p = (double)expf(l[k] - m) * is;
                const double wt = (a.weight ? (double)a.weight[k] : 1.0) * fma(om, (double)t[k], ek);
                gr[k] = (float)((p * T - wt) * inv);
            }
        }
        if (lane == 0) {
            if (a.reduction == TAMGCN_CE_NONE) loss[n] = (float)L; else rowloss[n] = L;
        }
    }
}

__global__ __launch_bounds__(CEO_NT) void ce_opts_finish_kernel(CeoArgs a, const double* rowloss, float* loss) {
    __shared__ double red[CEO_NT];
    double W = (double)a.N;
    if (a.reduction == TAMGCN_CE_MEAN && a.labels) W = ceo_normaliser(a, red);
    __syncthreads();
    double acc = 0.0;
    for (int n = threadIdx.x; n < a.N; n += CEO_NT) acc += rowloss[n];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = CEO_NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {                                     // W = 0 (no kept row, or kept weights that sum to 0): NaN, as torch --
        const double total = red[0];                            // also where the smoothing terms alone would give x / 0
        loss[0] = a.reduction == TAMGCN_CE_MEAN ? (W == 0.0 ? __builtin_nanf("") : (float)(total / W)) : (float)total;
    }
}

__global__ __launch_bounds__(CEO_NT) void ce_opts_bwd_rows_kernel(const float* g, const float* dloss, int total, int K, float* dlogits) {
    const int e = blockIdx.x * CEO_NT + threadIdx.x;
    if (e < total) dlogits[e] = g[e] * dloss[e / K];
}

}  // namespace

// the checks of a descriptor, shared by the size query and the launch; `who` names the entry point in the message
static int ceo_check(const char* who, const tamgcn_ce_desc* d) {
    TG_CHECK(d, "%s: null descriptor", who);
    TG_CHECK(d->N >= 1 && d->K >= 1, "%s: bad dims N=%d K=%d (both must be >= 1)", who, d->N, d->K);
    TG_CHECK(d->logits, "%s: null logits", who);
    TG_CHECK((d->labels != nullptr) != (d->probs != nullptr), "%s: exactly one of labels and probs must be given, got %s", who,
             d->labels ? "both" : "neither");
    TG_CHECK(d->label_smoothing >= 0.0 && d->label_smoothing <= 1.0, "%s: label_smoothing=%g outside [0, 1]", who, d->label_smoothing);
    TG_CHECK(d->reduction == TAMGCN_CE_MEAN || d->reduction == TAMGCN_CE_SUM || d->reduction == TAMGCN_CE_NONE,
             "%s: unknown reduction=%d (0 mean, 1 sum, 2 none)", who, d->reduction);
    TG_CHECK((long long)d->N * d->K < (1LL << 31), "%s: N*K=%lld elements: the element grid would overflow (limit 2^31 - 1)", who,
             (long long)d->N * d->K);
    return 0;
}

extern "C" long long tamgcn_ce_opts_workspace_bytes(const tamgcn_ce_desc* d) {
    if (ceo_check("tamgcn_ce_opts_workspace_bytes", d) < 0) return -1;
    return d->reduction == TAMGCN_CE_NONE ? 0 : (long long)sizeof(double) * d->N;
}

extern "C" int tamgcn_ce_opts_fwd(const tamgcn_ce_desc* d, float* loss, float* g, void* workspace, void* stream) {
    if (ceo_check("tamgcn_ce_opts_fwd", d) < 0) return -1;
    TG_CHECK(loss && g, "tamgcn_ce_opts_fwd: null %s", loss ? "g" : "loss");
    TG_CHECK(workspace || d->reduction == TAMGCN_CE_NONE, "tamgcn_ce_opts_fwd: null workspace (reduction=%d needs %lld bytes)", d->reduction,
             (long long)sizeof(double) * d->N);
    CeoArgs a;
    a.logits = d->logits; a.labels = d->labels; a.probs = d->probs; a.weight = d->weight;
    a.ignore_index = d->ignore_index; a.eps = d->label_smoothing; a.reduction = d->reduction; a.N = d->N; a.K = d->K;
    const int passes = (d->N - 1) / CEO_ROWS + 1;               // workgroups that would cover every row at once
    const int wg = passes < CEO_MAX_WG ? passes : CEO_MAX_WG;
    hipLaunchKernelGGL(ce_opts_rows_kernel, dim3((unsigned)wg), dim3(CEO_NT), 0, (hipStream_t)stream, a, loss, g, (double*)workspace);
    tamgcn_note_kernel("ce_opts_rows_kernel");
    TG_LAUNCH_CHECK("tamgcn_ce_opts_fwd");
    if (d->reduction != TAMGCN_CE_NONE) {
        hipLaunchKernelGGL(ce_opts_finish_kernel, dim3(1), dim3(CEO_NT), 0, (hipStream_t)stream, a, (const double*)workspace, loss);
        tamgcn_note_kernel("ce_opts_finish_kernel");
        TG_LAUNCH_CHECK("tamgcn_ce_opts_fwd");
    }
    return 0;
}

extern "C" int tamgcn_ce_opts_bwd_rows(const float* g, const float* dloss, int N, int K, float* dlogits, void* stream) {
    TG_CHECK(g && dloss && dlogits, "tamgcn_ce_opts_bwd_rows: null %s", !g ? "g" : !dloss ? "dloss" : "dlogits");
    TG_CHECK(N >= 1 && K >= 1, "tamgcn_ce_opts_bwd_rows: bad dims N=%d K=%d (both must be >= 1)", N, K);
    TG_CHECK((long long)N * K < (1LL << 31), "tamgcn_ce_opts_bwd_rows: N*K=%lld elements: the element grid would overflow (limit 2^31 - 1)",
             (long long)N * K);
    const int total = N * K;
    hipLaunchKernelGGL(ce_opts_bwd_rows_kernel, dim3((unsigned)ceil_div(total, CEO_NT)), dim3(CEO_NT), 0, (hipStream_t)stream, g, dloss, total, K,
                       dlogits);
    tamgcn_note_kernel("ce_opts_bwd_rows_kernel");
    TG_LAUNCH_CHECK("tamgcn_ce_opts_bwd_rows");
    return 0;
}
