// Fused optimiser update over flat fp32 buffers (ParamArena / FlatGradBucket): SGD (torch.optim.SGD) and Adam
// (torch.optim.Adam, coupled L2 weight decay, no amsgrad), one streaming pass.
//
// Capture safety.  The learning rate and the step count live in device memory: a HIP graph that holds the update reads
// the CURRENT learning rate and advances its own step count on every replay, so the host may change the rate between
// replays and SGD's first-step rule (buf = d) and Adam's bias corrections stay right after any number of replays.
//
// Two launches per call: a one-thread prologue advances *step and writes this step's scalars (in double where they
// come from powers of the betas) to scal[2]; the streaming kernel reads them.  Ordinary C++ stores only.
// The streaming kernel is the flat shape of elementwise.hip: 256-thread workgroups, one 16-byte vector per lane per
// iteration, a grid of at most 2048 workgroups striding over the rest; the n % 4 tail is scalar.
#include "common.h"
#include <math.h>

namespace {

constexpr int OPT_THREADS = 256;
constexpr long long OPT_MAX_BLOCKS = 2048;      // 256 CUs x 8 resident workgroups; the rest by grid stride

// scal[0]: SGD lr | Adam lr / (1 - b1^t);  scal[1]: SGD 1 on the first step else 0 | Adam sqrt(1 - b2^t)
__global__ void optim_prologue_kernel(int mode, const float* __restrict__ lr, int* __restrict__ step,
                                      float* __restrict__ scal, double beta1, double beta2) {
    if (threadIdx.x != 0) return;
    const int t = *step + 1;
    *step = t;
    const float l = *lr;
    if (mode == 0) {
        scal[0] = l;
        scal[1] = t == 1 ? 1.f : 0.f;
    } else {
        const double bc1 = 1.0 - pow(beta1, (double)t);
        const double bc2 = 1.0 - pow(beta2, (double)t);
        scal[0] = (float)((double)l / bc1);
        scal[1] = (float)sqrt(bc2);
    }
}

struct OptArgs {
    float m, one_m_damp, wd;          // SGD
    float b1, one_m_b1, b2, one_m_b2, eps;   // Adam
    int nesterov;
};

// one element; torch.optim.SGD (foreach=False) operation for operation
template <bool MOM>
__device__ __forceinline__ void sgd1(float& p, float g, float& buf, const OptArgs& a, float lr, bool first) {
    float d = a.wd != 0.f ? g + a.wd * p : g;
    if (MOM) {
        buf = first ? d : a.m * buf + a.one_m_damp * d;
        d = a.nesterov ? d + a.m * buf : buf;
    }
    p = p - lr * d;
}

// one element; torch.optim.Adam (coupled weight decay, amsgrad off)
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const OptArgs& a, float step_size, float bc2s) {
    if (a.wd != 0.f) g = g + a.wd * p;
    m = a.b1 * m + a.one_m_b1 * g;
    v = a.b2 * v + a.one_m_b2 * (g * g);
    const float denom = sqrtf(v) / bc2s + a.eps;
    p = p - step_size * (m / denom);
}

template <int MODE, bool MOM>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(long long n, float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ s0, float* __restrict__ s1,
                                                                   const float* __restrict__ scal, OptArgs a) {
    const float c0 = scal[0], c1 = scal[1];
    const bool first = c1 != 0.f;
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * OPT_THREADS;
    const long long i0 = (long long)blockIdx.x * OPT_THREADS + threadIdx.x;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(s0);
    f32x4* v4 = reinterpret_cast<f32x4*>(s1);
    for (long long i = i0; i < n4; i += stride) {
        f32x4 pv = p4[i];
        const f32x4 gv = g4[i];
        if (MODE == 0) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (MOM && !first) bv = m4[i];            // the first step overwrites the buffer without reading it
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pv[k], bk = bv[k];
                sgd1<MOM>(pk, gv[k], bk, a, c0, first);
                pv[k] = pk; bv[k] = bk;
            }
            if (MOM) m4[i] = bv;
        } else {
            f32x4 mv = m4[i], vv = v4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pv[k], mk = mv[k], vk = vv[k];
                adam1(pk, gv[k], mk, vk, a, c0, c1);
                pv[k] = pk; mv[k] = mk; vv[k] = vk;
            }
            m4[i] = mv;
            v4[i] = vv;
        }
        p4[i] = pv;
    }
    // tail: n % 4 elements, one per thread of the first workgroup
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        float pk = p[i];
        if (MODE == 0) {
            float bk = MOM && !first ? s0[i] : 0.f;
            sgd1<MOM>(pk, g[i], bk, a, c0, first);
            if (MOM) s0[i] = bk;
        } else {
            float mk = s0[i], vk = s1[i];
            adam1(pk, g[i], mk, vk, a, c0, c1);
            s0[i] = mk;
            s1[i] = vk;
        }
        p[i] = pk;
    }
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" int tamgcn_optim_step(const tamgcn_optim_desc* d, void* stream) {
    TG_CHECK(d, "tamgcn_optim_step: NULL descriptor");
    TG_CHECK(d->mode == 0 || d->mode == 1, "tamgcn_optim_step: mode %d is neither 0 (SGD) nor 1 (Adam)", d->mode);
    TG_CHECK(d->n > 0, "tamgcn_optim_step: n = %lld", d->n);
    TG_CHECK(d->p && d->g && d->lr && d->step && d->scal, "tamgcn_optim_step: NULL p, g, lr, step or scal");
    const bool mom = d->mode == 0 && d->momentum != 0.f;
    TG_CHECK(!(d->mode == 1 || mom) || d->s0, "tamgcn_optim_step: NULL s0 (momentum buffer / exp_avg)");
    TG_CHECK(d->mode == 0 || d->s1, "tamgcn_optim_step: NULL s1 (exp_avg_sq)");
    TG_CHECK(aligned16(d->p) && aligned16(d->g) && aligned16(d->s0) && aligned16(d->s1),
             "tamgcn_optim_step: p, g, s0, s1 must be 16-byte aligned");
    TG_CHECK(d->weight_decay >= 0.f, "tamgcn_optim_step: weight_decay %g < 0", (double)d->weight_decay);
    if (d->mode == 0) {
        TG_CHECK(d->momentum >= 0.f, "tamgcn_optim_step: momentum %g < 0", (double)d->momentum);
        TG_CHECK(!d->nesterov || (d->momentum > 0.f && d->dampening == 0.f),
                 "tamgcn_optim_step: Nesterov momentum needs momentum > 0 and zero dampening");
    } else {
        TG_CHECK(d->beta1 >= 0.0 && d->beta1 < 1.0 && d->beta2 >= 0.0 && d->beta2 < 1.0,
                 "tamgcn_optim_step: betas (%g, %g) outside [0, 1)", d->beta1, d->beta2);
        TG_CHECK(d->eps >= 0.f, "tamgcn_optim_step: eps %g < 0", (double)d->eps);
    }
    OptArgs a;
    a.m = d->momentum;
    a.one_m_damp = 1.f - d->dampening;
    a.wd = d->weight_decay;
    a.b1 = (float)d->beta1;
    a.one_m_b1 = (float)(1.0 - d->beta1);
    a.b2 = (float)d->beta2;
    a.one_m_b2 = (float)(1.0 - d->beta2);
    a.eps = d->eps;
    a.nesterov = d->nesterov ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_prologue_kernel, dim3(1), dim3(1), 0, s, d->mode, d->lr, d->step, d->scal, d->beta1, d->beta2);
    TG_LAUNCH_CHECK("tamgcn_optim_step (prologue)");
    const long long n4 = d->n >> 2;
    long long blocks = (n4 + OPT_THREADS - 1) / OPT_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > OPT_MAX_BLOCKS) blocks = OPT_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks), block(OPT_THREADS);
    if (d->mode == 1) {
        hipLaunchKernelGGL((optim_update_kernel<1, true>), grid, block, 0, s, d->n, d->p, d->g, d->s0, d->s1, d->scal, a);
        tamgcn_note_kernel("optim_update_kernel<1, true>");
    } else if (mom) {
        hipLaunchKernelGGL((optim_update_kernel<0, true>), grid, block, 0, s, d->n, d->p, d->g, d->s0, d->s1, d->scal, a);
        tamgcn_note_kernel("optim_update_kernel<0, true>");
    } else {
        hipLaunchKernelGGL((optim_update_kernel<0, false>), grid, block, 0, s, d->n, d->p, d->g, d->s0, d->s1, d->scal, a);
        tamgcn_note_kernel("optim_update_kernel<0, false>");
    }
    TG_LAUNCH_CHECK("tamgcn_optim_step");
    return 0;
}
