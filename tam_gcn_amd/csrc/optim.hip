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
//
// tamgcn_optim_step_guarded is the same update behind a gradient guard, three launches: grad_sumsq_kernel leaves one fp64
// partial of sum g^2 per workgroup (thread -> 64-lane wave by shuffles -> waves through LDS, one ordinary store);
// optim_guard_prologue_kernel, one workgroup, adds the partials in a fixed order, writes the norm, the clipping
// coefficient min(1, max_norm / (norm + 1e-6)) and the finite flag to stat[3], and then does the plain prologue's work
// unless the step is skipped; optim_update_guarded_kernel multiplies every gradient element by the coefficient (its own
// rounding, never contracted into the weight-decay FMA: coef == 1 gives the plain kernel's bits) or returns before its
// first store.  No floating-point atomics: the sum does not depend on the order in which workgroups arrive.
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

// g * coef as torch.nn.utils.clip_grad_norm_ applies it: a product rounded on its own.  Contraction is switched off so
// that it never fuses with the weight-decay term that follows (g * 1.0f must stay g).
__device__ __forceinline__ float clip1(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;
}

template <int MODE, bool MOM, bool GUARD>
__device__ __forceinline__ void optim_update_body(long long n, float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ s0, float* __restrict__ s1,
                                                  const float* __restrict__ scal, const OptArgs& a, float coef) {
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
        f32x4 gv = g4[i];
        if (GUARD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) gv[k] = clip1(gv[k], coef);
        }
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
        const float gk = GUARD ? clip1(g[i], coef) : g[i];
        if (MODE == 0) {
            float bk = MOM && !first ? s0[i] : 0.f;
            sgd1<MOM>(pk, gk, bk, a, c0, first);
            if (MOM) s0[i] = bk;
        } else {
            float mk = s0[i], vk = s1[i];
            adam1(pk, gk, mk, vk, a, c0, c1);
            s0[i] = mk;
            s1[i] = vk;
        }
        p[i] = pk;
    }
}

template <int MODE, bool MOM>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(long long n, float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ s0, float* __restrict__ s1,
                                                                   const float* __restrict__ scal, OptArgs a) {
    optim_update_body<MODE, MOM, false>(n, p, g, s0, s1, scal, a, 1.f);
}

// stat: [norm, coef, finite] of optim_guard_prologue_kernel.  A skipped step returns before the first store.
template <int MODE, bool MOM>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_guarded_kernel(long long n, float* __restrict__ p, const float* __restrict__ g,
                                                                           float* __restrict__ s0, float* __restrict__ s1,
                                                                           const float* __restrict__ scal, OptArgs a,
                                                                           const float* __restrict__ stat, int skip_nonfinite) {
    if (skip_nonfinite && stat[2] == 0.f) return;
    optim_update_body<MODE, MOM, true>(n, p, g, s0, s1, scal, a, stat[1]);
}

// Sum over the workgroup in a fixed shape: lanes of each 64-wide wave by shuffles (32, 16, ..., 1), then the waves in
// order through LDS.  The total is valid in thread 0.
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double wsum[OPT_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < OPT_THREADS / 64; ++w) t += wsum[w];
    }
    return t;
}

// partial[blockIdx.x] = sum of (double)g[i]^2 over this workgroup's grid-stride share (the n % 4 tail goes to workgroup 0)
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(long long n, const float* __restrict__ g, double* __restrict__ partial) {
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * OPT_THREADS;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
        const f32x4 gv = g4[i];
        const double d0 = gv[0], d1 = gv[1], d2 = gv[2], d3 = gv[3];
        a0 += d0 * d0;
        a1 += d1 * d1;
        a2 += d2 * d2;
        a3 += d3 * d3;
    }
    double acc = (a0 + a1) + (a2 + a3);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const double d = g[(n4 << 2) + threadIdx.x];
        acc += d * d;
    }
    const double t = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// One workgroup: thread t adds partial[t], partial[t + 256], ... in that order, block_sum adds the threads.  Thread 0
// then writes stat and, unless the step is skipped, does what optim_prologue_kernel does.
__global__ __launch_bounds__(OPT_THREADS) void optim_guard_prologue_kernel(int mode, const float* __restrict__ lr, int* __restrict__ step,
                                                                           float* __restrict__ scal, double beta1, double beta2,
                                                                           const double* __restrict__ partial, int n_partial,
                                                                           float max_norm, int skip_nonfinite,
                                                                           float* __restrict__ stat, int* __restrict__ skipped) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += OPT_THREADS) acc += partial[i];
    const double sum = block_sum(acc);
    if (threadIdx.x != 0) return;
    const bool finite = isfinite(sum);
    const float norm = (float)sqrt(sum);
    float coef = 1.f;
    if (max_norm > 0.f) {
        const float c = max_norm / (norm + 1e-6f);
        coef = c > 1.f ? 1.f : c;                    // a NaN norm gives a NaN coefficient, as torch.clamp(max=1) does
    }
    stat[0] = norm;
    stat[1] = coef;
    stat[2] = finite ? 1.f : 0.f;
    if (skip_nonfinite && !finite) {
        *skipped = *skipped + 1;
        return;
    }
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

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

// the argument checks and the launch arguments that tamgcn_optim_step and tamgcn_optim_step_guarded share
static int optim_check(const tamgcn_optim_desc* d, const char* fn, OptArgs& a, bool& mom) {
    TG_CHECK(d, "%s: NULL descriptor", fn);
    TG_CHECK(d->mode == 0 || d->mode == 1, "%s: mode %d is neither 0 (SGD) nor 1 (Adam)", fn, d->mode);
    TG_CHECK(d->n > 0, "%s: n = %lld", fn, d->n);
    TG_CHECK(d->p && d->g && d->lr && d->step && d->scal, "%s: NULL p, g, lr, step or scal", fn);
    mom = d->mode == 0 && d->momentum != 0.f;
    TG_CHECK(!(d->mode == 1 || mom) || d->s0, "%s: NULL s0 (momentum buffer / exp_avg)", fn);
    TG_CHECK(d->mode == 0 || d->s1, "%s: NULL s1 (exp_avg_sq)", fn);
    TG_CHECK(aligned16(d->p) && aligned16(d->g) && aligned16(d->s0) && aligned16(d->s1),
             "%s: p, g, s0, s1 must be 16-byte aligned", fn);
    TG_CHECK(d->weight_decay >= 0.f, "%s: weight_decay %g < 0", fn, (double)d->weight_decay);
    if (d->mode == 0) {
        TG_CHECK(d->momentum >= 0.f, "%s: momentum %g < 0", fn, (double)d->momentum);
        TG_CHECK(!d->nesterov || (d->momentum > 0.f && d->dampening == 0.f),
                 "%s: Nesterov momentum needs momentum > 0 and zero dampening", fn);
    } else {
        TG_CHECK(d->beta1 >= 0.0 && d->beta1 < 1.0 && d->beta2 >= 0.0 && d->beta2 < 1.0,
                 "%s: betas (%g, %g) outside [0, 1)", fn, d->beta1, d->beta2);
        TG_CHECK(d->eps >= 0.f, "%s: eps %g < 0", fn, (double)d->eps);
    }
    a.m = d->momentum;
    a.one_m_damp = 1.f - d->dampening;
    a.wd = d->weight_decay;
    a.b1 = (float)d->beta1;
    a.one_m_b1 = (float)(1.0 - d->beta1);
    a.b2 = (float)d->beta2;
    a.one_m_b2 = (float)(1.0 - d->beta2);
    a.eps = d->eps;
    a.nesterov = d->nesterov ? 1 : 0;
    return 0;
}

static unsigned optim_grid(long long n) {
    long long blocks = ((n >> 2) + OPT_THREADS - 1) / OPT_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > OPT_MAX_BLOCKS) blocks = OPT_MAX_BLOCKS;
    return (unsigned)blocks;
}

extern "C" int tamgcn_optim_step(const tamgcn_optim_desc* d, void* stream) {
    OptArgs a;
    bool mom;
    if (int rc = optim_check(d, "tamgcn_optim_step", a, mom)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_prologue_kernel, dim3(1), dim3(1), 0, s, d->mode, d->lr, d->step, d->scal, d->beta1, d->beta2);
    TG_LAUNCH_CHECK("tamgcn_optim_step (prologue)");
    const dim3 grid(optim_grid(d->n)), block(OPT_THREADS);
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

extern "C" int tamgcn_optim_step_guarded(const tamgcn_optim_desc* d, const tamgcn_grad_guard* g, void* stream) {
    const char* fn = "tamgcn_optim_step_guarded";
    OptArgs a;
    bool mom;
    if (int rc = optim_check(d, fn, a, mom)) return rc;
    TG_CHECK(g, "%s: NULL guard descriptor", fn);
    TG_CHECK(g->partial && g->stat, "%s: NULL partial or stat", fn);
    TG_CHECK(!g->skip_nonfinite || g->skipped, "%s: skip_nonfinite needs the skipped counter (NULL)", fn);
    TG_CHECK(((uintptr_t)g->partial & 7u) == 0, "%s: partial must be 8-byte aligned", fn);
    TG_CHECK(g->max_norm == g->max_norm, "%s: max_norm is NaN", fn);
    const unsigned blocks = optim_grid(d->n);
    TG_CHECK(g->n_partial >= (int)blocks, "%s: n_partial %d < the %u workgroups of the reduction", fn, g->n_partial, blocks);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks), block(OPT_THREADS);
    const int skip = g->skip_nonfinite ? 1 : 0;
    hipLaunchKernelGGL(grad_sumsq_kernel, grid, block, 0, s, d->n, d->g, g->partial);
    TG_LAUNCH_CHECK("tamgcn_optim_step_guarded (norm)");
    hipLaunchKernelGGL(optim_guard_prologue_kernel, dim3(1), block, 0, s, d->mode, d->lr, d->step, d->scal, d->beta1, d->beta2,
                       (const double*)g->partial, (int)blocks, g->max_norm, skip, g->stat, g->skipped);
    TG_LAUNCH_CHECK("tamgcn_optim_step_guarded (prologue)");
    if (d->mode == 1) {
        hipLaunchKernelGGL((optim_update_guarded_kernel<1, true>), grid, block, 0, s, d->n, d->p, d->g, d->s0, d->s1, d->scal, a,
                           (const float*)g->stat, skip);
        tamgcn_note_kernel("optim_update_guarded_kernel<1, true>");
    } else if (mom) {
        hipLaunchKernelGGL((optim_update_guarded_kernel<0, true>), grid, block, 0, s, d->n, d->p, d->g, d->s0, d->s1, d->scal, a,
                           (const float*)g->stat, skip);
        tamgcn_note_kernel("optim_update_guarded_kernel<0, true>");
    } else {
        hipLaunchKernelGGL((optim_update_guarded_kernel<0, false>), grid, block, 0, s, d->n, d->p, d->g, d->s0, d->s1, d->scal, a,
                           (const float*)g->stat, skip);
        tamgcn_note_kernel("optim_update_guarded_kernel<0, false>");
    }
    TG_LAUNCH_CHECK("tamgcn_optim_step_guarded");
    return 0;
}
