// Input-gradient joint saliency (include/tamgcn.h "saliency"; tam_gcn_amd/saliency.py): two small streaming kernels behind the
// f2s backward chain.
//
//   tamgcn_saliency_joints      sal[n][v] = sum over (m, c, t) of |c1[(m V + v) C + c] * dx0[n M + m][c][t][v]|: the eval-mode data_bn
//                               is an affine per (person, joint, channel), so the gradient with respect to the raw input is the
//                               first block's dx scaled by its c1; optionally that gradient itself, dxin (N, C, T, V, M).
//                               One wave per (n, v): lane l adds the elements l, l + 64, ... of the flat (m, c, t) index in that
//                               order, then the 64 partial sums meet in a fixed butterfly.  Two launches are bit-equal.
//   tamgcn_saliency_accumulate  the body-part bookkeeping of a saliency pass over a dataset, on the device: ONE workgroup walks the
//                               batch in order (the per-class cap makes the rule sequential), no host synchronisation.
#include "common.h"

namespace {

__global__ __launch_bounds__(64) void saliency_joints_kernel(const float* __restrict__ dx0, const float* __restrict__ c1, int C, int T, int V, int M,
                                                              float* __restrict__ sal, float* __restrict__ dxin) {
    const int v = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    const int L = M * C * T;
    float s = 0.f;
    for (int i = lane; i < L; i += 64) {
        const int t = i % T, c = (i / T) % C, m = i / (T * C);
        const float g = c1[(m * V + v) * C + c] * dx0[((((long long)n * M + m) * C + c) * T + t) * V + v];
        s += fabsf(g);
        if (dxin) dxin[((((long long)n * C + c) * T + t) * V + v) * M + m] = g;
    }
    s = wave_sum64(s);
    if (lane == 0) sal[(long long)n * V + v] = s;
}

constexpr int SA_MAXN = 4096;                // samples of one call: their counted flags live in LDS
constexpr int SA_NT = 256;                   // parts at most: one thread per part

__global__ __launch_bounds__(SA_NT) void saliency_accumulate_kernel(const float* __restrict__ sal, const long long* __restrict__ labels, int N, int V,
                                                                    const int* __restrict__ part_off, const int* __restrict__ part_joints, int P,
                                                                    int num_class, int per_class, int* __restrict__ count,
                                                                    double* __restrict__ sum) {
    __shared__ unsigned char counted[SA_MAXN];
    const int tid = threadIdx.x;
    if (tid == 0) {                                                          // batch order: a class takes samples until it holds per_class
        for (int i = 0; i < N; ++i) {
            const long long k = labels[i];
            bool ok = k >= 0 && k < num_class;
            if (ok) {
                const int have = count[k];
                ok = have < per_class;
                if (ok) count[k] = have + 1;
            }
            counted[i] = ok;
        }
    }
    __syncthreads();
    if (tid < P) {                                                           // sum[class][part] belongs to this thread alone
        const int j0 = part_off[tid], j1 = part_off[tid + 1];
        for (int i = 0; i < N; ++i) {
            if (!counted[i]) continue;
            double acc = 0.0;
            int nj = 0;
            for (int j = j0; j < j1; ++j) {
                const int v = part_joints[j];
                if (v >= 0 && v < V) {
                    acc += (double)sal[(long long)i * V + v];
                    ++nj;
                }
            }
            if (nj) sum[labels[i] * P + tid] += acc / (double)nj;
        }
    }
}

}  // namespace

extern "C" int tamgcn_saliency_joints(const float* dx0, const float* coef, int N, int C, int T, int V, int M, float* sal, float* dxin,
                                      void* stream) {
    const char* who = "tamgcn_saliency_joints";
    TG_CHECK(dx0 && coef && sal, "%s: null pointer", who);
    TG_CHECK(N >= 1 && C >= 1 && T >= 1 && V >= 1 && M >= 1 && N <= 65535, "%s: bad dims N=%d C=%d T=%d V=%d M=%d", who, N, C, T, V, M);
    TG_CHECK((long long)N * M * C * T * V < (1ll << 31), "%s: tensor of 2^31 elements or more", who);
    hipLaunchKernelGGL(saliency_joints_kernel, dim3(V, N), dim3(64), 0, (hipStream_t)stream, dx0, coef, C, T, V, M, sal, dxin);
    tamgcn_note_kernel("saliency_joints_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int tamgcn_saliency_accumulate(const float* sal, const long long* labels, int N, int V, const int* part_off, const int* part_joints,
                                          int P, int num_class, int per_class, int* count, double* sum, void* stream) {
    const char* who = "tamgcn_saliency_accumulate";
    TG_CHECK(sal && labels && part_off && part_joints && count && sum, "%s: null pointer", who);
    TG_CHECK(N >= 1 && N <= SA_MAXN && V >= 1 && P >= 1 && P <= SA_NT && num_class >= 1 && per_class >= 0,
             "%s: bad dims N=%d (1..%d) V=%d P=%d (1..%d) num_class=%d per_class=%d", who, N, SA_MAXN, V, P, SA_NT, num_class, per_class);
    hipLaunchKernelGGL(saliency_accumulate_kernel, dim3(1), dim3(SA_NT), 0, (hipStream_t)stream, sal, labels, N, V, part_off, part_joints, P,
                       num_class, per_class, count, sum);
    tamgcn_note_kernel("saliency_accumulate_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}
