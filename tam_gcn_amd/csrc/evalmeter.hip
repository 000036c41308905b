// The evaluation epoch's bookkeeping on the device (reference processor/recognition_rgb.py:71-101: loss.item(), output.cpu(),
// label.cpu() and np.argmax per batch; ensemble/ensemble_ctrgcn_resnet_eval.py:217-234, :267, :421-438: per-class accuracy,
// confusion matrix, alpha sweep).  One launch per batch adds the batch to a state that stays in HBM; the host reads it once.
#include "common.h"
#include "evalbody.h"

namespace {

struct TopK { int k[TAMGCN_EVAL_MAX_TOPK]; int nk; };

// ONE workgroup of CE_NT threads, thread -> rows n = tid, tid + 256, ... (ce_fwd_kernel's mapping: the batch mean is that
// kernel's for rows [0, valid), bit for bit).  Rows n >= valid are not read.  Floating-point state is written by thread 0
// alone, integer state by atomics; a label outside [0, K) touches no class row and an index outside [0, num_samples) no
// score row.
__global__ __launch_bounds__(CE_NT) void eval_accumulate_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                const long long* __restrict__ index, int B, int K, int valid_host,
                                                                const int* __restrict__ valid_dev, TopK tk, long long base, long long num_samples,
                                                                unsigned long long* counts, double* sums, int* confusion, float* scores) {
    __shared__ double red[CE_NT];
    __shared__ int cnt[CE_NT];
    __shared__ int bad[CE_NT];
    int valid = valid_dev ? valid_dev[0] : valid_host;
    valid = valid < 0 ? 0 : (valid > B ? B : valid);
    const CeCount c = ce_count_labels(labels, valid, K, cnt, bad);
    const int kept = c.kept, nbad = c.nbad;
    double acc = 0.0;
    int hits[TAMGCN_EVAL_MAX_TOPK] = {0, 0, 0, 0};
    int badidx = 0;
    for (int n = threadIdx.x; n < valid; n += CE_NT) {
        const float* l = logits + (long long)n * K;
        if (scores) {
            const long long r = index ? index[n] : base + n;
            if (r >= 0 && r < num_samples) {
                float* o = scores + r * K;
                for (int k = 0; k < K; ++k) o[k] = l[k];
            } else {
                ++badidx;
            }
        }
        const long long y = labels[n];
        if (y < 0 || y >= K) continue;
        acc += (double)(ce_row_lse(l, K).lse - l[y]);
        // first arg max (numpy.argmax); rank of the label's score in a stable ascending sort, counted from the top
        const float sl = l[y];
        int best = 0, above = 0;
        for (int k = 0; k < K; ++k) {
            const float v = l[k];
            if (v > l[best]) best = k;
            above += (v > sl || (v == sl && k > (int)y)) ? 1 : 0;
        }
        atomicAdd(&confusion[y * K + best], 1);
#pragma unroll
        for (int i = 0; i < TAMGCN_EVAL_MAX_TOPK; ++i)
            if (i < tk.nk && above < tk.k[i]) ++hits[i];
    }
    const double total = ce_block_sum(acc, red);
    if (badidx) atomicAdd(&counts[3], (unsigned long long)badidx);
#pragma unroll
    for (int i = 0; i < TAMGCN_EVAL_MAX_TOPK; ++i)
        if (i < tk.nk && hits[i]) atomicAdd(&counts[4 + i], (unsigned long long)hits[i]);
    if (threadIdx.x == 0) {
        if (nbad) atomicAdd(&counts[2], (unsigned long long)nbad);
        if (kept > 0) {
            atomicAdd(&counts[0], 1ull);
            atomicAdd(&counts[1], (unsigned long long)kept);
            sums[0] += (double)ce_mean(total, kept, nbad);
            sums[1] += total;
        }
    }
}

struct Alphas { float a[TAMGCN_SWEEP_MAX_ALPHAS]; int n; };

// fused = 1 * a + alpha * b exactly as score_fuse_kernel builds it from weights (1, alpha) -- 0 + 1 * a, then + alpha * b, each
// product and sum rounded -- for every alpha at once; only the first arg max is kept.  One lane per sample.
__global__ __launch_bounds__(CE_NT) void score_sweep_kernel(const float* __restrict__ a, const float* __restrict__ b, Alphas al, int N, int K,
                                                            int softmax, const long long* __restrict__ labels, int* correct) {
    const int n = blockIdx.x * CE_NT + threadIdx.x;
    if (n >= N) return;
    const long long y = labels[n];
    if (y < 0 || y >= K) return;
    const float* xa = a + (long long)n * K;
    const float* xb = b + (long long)n * K;
    float mxa, inva, mxb, invb;
    fuse_softmax_stats(xa, K, softmax, mxa, inva);
    fuse_softmax_stats(xb, K, softmax, mxb, invb);
    for (int i = 0; i < al.n; ++i) {
        int best = 0;
        float fbest = 0.f;
        for (int k = 0; k < K; ++k) {
            const float f = fuse_add(fuse_add(0.f, 1.f, xa, k, softmax, mxa, inva), al.a[i], xb, k, softmax, mxb, invb);
            if (k == 0 || f > fbest) { best = k; fbest = f; }
        }
        if (best == (int)y) atomicAdd(&correct[i], 1);
    }
}

}  // namespace

extern "C" int tamgcn_eval_accumulate(const float* logits, const long long* labels, const long long* index, int B, int K,
                                      int valid, const int* valid_dev, const int* topk, int nk, long long base, long long num_samples,
                                      long long* counts, double* sums, int* confusion, float* scores, void* stream) {
    TG_CHECK(logits && labels && counts && sums && confusion, "tamgcn_eval_accumulate: null logits, labels, counts, sums or confusion");
    TG_CHECK(B > 0 && K > 0, "tamgcn_eval_accumulate: B = %d, K = %d", B, K);
    TG_CHECK(nk >= 0 && nk <= TAMGCN_EVAL_MAX_TOPK && (nk == 0 || topk), "tamgcn_eval_accumulate: nk = %d (0 .. %d entries of topk)", nk, TAMGCN_EVAL_MAX_TOPK);
    TG_CHECK((long long)K * K < (1LL << 31), "tamgcn_eval_accumulate: K = %d (the confusion matrix is indexed in 32 bits)", K);
    TG_CHECK(!scores || (num_samples > 0 && num_samples < (1LL << 40)), "tamgcn_eval_accumulate: scores with num_samples = %lld", num_samples);
    TopK tk;
    tk.nk = nk;
    for (int i = 0; i < TAMGCN_EVAL_MAX_TOPK; ++i) tk.k[i] = i < nk ? topk[i] : 0;
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(CE_NT), 0, (hipStream_t)stream, logits, labels, index, B, K, valid, valid_dev, tk,
                       base, num_samples, (unsigned long long*)counts, sums, confusion, scores);
    tamgcn_note_kernel("eval_accumulate_kernel");
    TG_LAUNCH_CHECK("tamgcn_eval_accumulate");
    return 0;
}

extern "C" int tamgcn_score_sweep(const float* a, const float* b, const float* alphas, int A, int N, int K, int softmax,
                                  const long long* labels, int* correct, void* stream) {
    TG_CHECK(a && b && alphas && labels && correct, "tamgcn_score_sweep: null argument");
    TG_CHECK(A > 0 && A <= TAMGCN_SWEEP_MAX_ALPHAS && N > 0 && K > 0, "tamgcn_score_sweep: A = %d (1 .. %d), N = %d, K = %d", A, TAMGCN_SWEEP_MAX_ALPHAS, N, K);
    Alphas al;
    al.n = A;
    for (int i = 0; i < TAMGCN_SWEEP_MAX_ALPHAS; ++i) al.a[i] = i < A ? alphas[i] : 0.f;
    hipError_t e = hipMemsetAsync(correct, 0, sizeof(int) * A, (hipStream_t)stream);
    TG_CHECK(e == hipSuccess, "tamgcn_score_sweep: memset failed");
    hipLaunchKernelGGL(score_sweep_kernel, dim3((unsigned)ceil_div(N, CE_NT)), dim3(CE_NT), 0, (hipStream_t)stream, a, b, al, N, K, softmax, labels, correct);
    tamgcn_note_kernel("score_sweep_kernel");
    TG_LAUNCH_CHECK("tamgcn_score_sweep");
    return 0;
}
