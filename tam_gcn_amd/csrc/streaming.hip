// Live and sliding-window inference (tam_gcn_amd/streaming.py): a ring of skeleton frames in HBM that is pushed to without the
// host, the model's input windows built straight from the ring through either feeder's val-path arithmetic (feeder_common.h:
// the bodies feeder.hip and clipfeeder.hip run), and what a sliding-window user does with the scores: softmax, per-frame
// voting, an exponential moving average.  include/tamgcn.h has the contract.
//
// Frames are numbered absolutely from 0 (the first frame ever pushed); frame f lives in slot f % cap of a ring that is
// logically (P, cap, R): (1, cap, V 3) fp64 for the N-UCLA transform, (C, cap, V M) fp32 for the clip feeder's layout.  A
// sequence that is resident as a whole is a ring of cap = its length that never wraps.  No floating-point atomics anywhere:
// every sum has one order, so two calls give the same bits and a graph replay gives the eager call's.
#include "common.h"
#include "feeder_common.h"

namespace {

constexpr int STREAM_MAX_TS = 64;        // the N-UCLA window's time_steps (the feeder's draw kernel has the same limit)
constexpr int STREAM_MAX_K = 4096;       // classes: one softmax row as fp64 in LDS

// Python's f % cap for cap > 0: slot of frame f (f >= 0 wherever a valid window reads)
__device__ __forceinline__ long long slot_of(long long f, int cap) { return clip_of(f, cap); }

// ---- the ring --------------------------------------------------------------------------------------------------------
// One thread per unit U (16 bytes where the rows and addresses allow it, else one element) of the (P, n, R) frames; frame i
// of the push goes to slot (count + i) % cap of every plane.  count is read here and moved by ring_advance_kernel behind
// this launch on the same stream, so a graph that holds both pushes to new slots on every replay.
template <class U>
__global__ __launch_bounds__(256) void ring_push_kernel(const U* __restrict__ frames, int n, int units, long long total, U* __restrict__ ring,
                                                        int cap, const long long* __restrict__ state) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int u = (int)(e % units);
    const long long row = e / units;                   // (p, i)
    const int i = (int)(row % n);
    const long long p = row / n;
    const long long slot = slot_of(state[0] + i, cap);
    ring[(p * cap + slot) * units + u] = frames[e];
}

__global__ void ring_advance_kernel(long long* __restrict__ state, int n) {
    state[0] = state[0] + n;
    state[1] = state[1] + 1;
}

// Window j of B ends (B - 1 - j) hop frames before the newest frame; (0, 0) where it would start before frame 0 or before
// count - cap (already overwritten).
__global__ __launch_bounds__(64) void ring_plan_kernel(const long long* __restrict__ state, int cap, int B, int L, int hop,
                                                       long long* __restrict__ plan) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= B) return;
    const long long count = state[0];
    const long long start = count - (long long)(B - 1 - j) * hop - L;
    const bool valid = start >= 0 && start >= count - cap;
    plan[2 * j] = valid ? start : 0;
    plan[2 * j + 1] = valid ? L : 0;
}

// a plan row the window builders accept: anything else is an invalid window (zeros)
__device__ __forceinline__ bool window_ok(long long start, long long L, int cap) { return start >= 0 && L >= 1 && L <= cap; }

// ---- windows -----------------------------------------------------------------------------------------------------------
// One workgroup per window: feeder_transform_kernel's body on the window's L frames with the identity view and the val
// path's frame indices.
__global__ __launch_bounds__(256) void window_nucla_kernel(const double* __restrict__ ring, int cap, const long long* __restrict__ plan,
                                                           const int* __restrict__ parent, int V, int TS, int center_joint, int mode,
                                                           float* __restrict__ out) {
    const int b = blockIdx.x;
    const long long start = plan[2 * b], L = plan[2 * b + 1];
    float* o = out + (long long)b * 3 * TS * V;
    if (!window_ok(start, L, cap)) {                   // uniform over the workgroup
        for (int e = threadIdx.x; e < 3 * TS * V; e += 256) o[e] = 0.f;
        return;
    }
    const double I[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
    const long long s0 = slot_of(start, cap);
    auto point = [&](long long e) {
        const long long fr = e / V;
        long long s = s0 + fr;                         // fr < L <= cap: one conditional subtraction is the modulo
        if (s >= cap) s -= cap;
        return ring + (s * V + (e - fr * V)) * 3;
    };
    feeder_transform_body(point, [&](int t) { return val_frame(t, L, TS); }, L, V, TS, mode, center_joint, I, parent, o);
}

template <int VEC>
__device__ __forceinline__ void load_span(const float* __restrict__ p, float* v) {
    if constexpr (VEC == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q[j];
    } else {
        v[0] = p[0];
    }
}

// One thread per VEC consecutive positions of an output row of W VM floats; blockIdx.x = ((window, channel), tile of 256 VEC
// positions).  clip_resize_kernel's taps and blend on the crop (start, L), the two source frames fetched at their ring slots.
// VEC = 4 only where V M is a multiple of four and both arrays are 16-byte aligned: a span then lies inside one frame.
template <int VEC>
__global__ __launch_bounds__(256) void window_clip_kernel(const float* __restrict__ ring, int cap, const long long* __restrict__ plan, int C, int W,
                                                          int VM, int tiles, float* __restrict__ out) {
#pragma clang fp contract(off)
    const unsigned blk = blockIdx.x;
    const int tile = (int)(blk % (unsigned)tiles), bc = (int)(blk / (unsigned)tiles);
    const int c = bc % C, b = bc / C;
    const int rowlen = W * VM;
    const int i = (tile * 256 + (int)threadIdx.x) * VEC;
    if (i >= rowlen) return;
    float* o = out + (long long)bc * rowlen + i;
    const long long start = plan[2 * b], Ll = plan[2 * b + 1];
    float y[VEC];
    if (!window_ok(start, Ll, cap)) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) y[j] = 0.f;
    } else {
        const int L = (int)Ll;
        const float scale = (float)L / (float)W;
        const int t = i / VM, vm = i - t * VM;
        const ResizeTaps tp = resize_taps(t, L, scale);
        const long long s0 = slot_of(start, cap);
        long long a0 = s0 + tp.i0, a1 = s0 + tp.i1;    // i0, i1 < L <= cap
        if (a0 >= cap) a0 -= cap;
        if (a1 >= cap) a1 -= cap;
        const float* src = ring + (long long)c * cap * VM + vm;
        float x0[VEC], x1[VEC];
        load_span<VEC>(src + a0 * VM, x0);
        load_span<VEC>(src + a1 * VM, x1);
#pragma unroll
        for (int j = 0; j < VEC; ++j) y[j] = tp.l0 * x0[j] + tp.l1 * x1[j];
    }
    if constexpr (VEC == 4) {
        const f32x4 q = {y[0], y[1], y[2], y[3]};
        *reinterpret_cast<f32x4*>(o) = q;
    } else {
        o[0] = y[0];
    }
}

// ---- scores --------------------------------------------------------------------------------------------------------------
// One workgroup per window: softmax of the row in fp64 (max shift; the exponentials wait in LDS and one thread adds them class
// ascending), rounded once to fp32.
__global__ __launch_bounds__(256) void window_softmax_kernel(const float* __restrict__ logits, int K, float* __restrict__ probs) {
    __shared__ double ex[STREAM_MAX_K];
    __shared__ double red[256 / 64];
    __shared__ double total;
    const int j = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (long long)j * K;
    double m = -INFINITY;
    for (int k = tid; k < K; k += 256) m = fmax(m, (double)x[k]);
    for (int off = 1; off < 64; off <<= 1) m = fmax(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    for (int k = tid; k < K; k += 256) ex[k] = exp((double)x[k] - m);
    __syncthreads();
    if (tid == 0) {
        double s = 0.;
        for (int k = 0; k < K; ++k) s += ex[k];
        total = s;
    }
    __syncthreads();
    const double s = total;
    for (int k = tid; k < K; k += 256) probs[(long long)j * K + k] = (float)(ex[k] / s);
}

// first arg max over the workgroup: every thread brings the best (value, index) of its own indices, ascending
template <class T>
__device__ __forceinline__ int block_first_argmax(T val, int idx, T* sval, int* sidx) {
    const int tid = threadIdx.x;
    sval[tid] = val; sidx[tid] = idx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            const T v = sval[tid + off];
            const int i = sidx[tid + off];
            if (i >= 0 && (sidx[tid] < 0 || v > sval[tid] || (v == sval[tid] && i < sidx[tid]))) { sval[tid] = v; sidx[tid] = i; }
        }
        __syncthreads();
    }
    return sidx[0];
}

// One workgroup per frame f: the mean over the valid windows that cover f, j ascending, of their fp32 probabilities, summed in
// fp64 and rounded once; the label is the first arg max of the rounded scores.  No window: zeros and -1.
__global__ __launch_bounds__(256) void window_vote_kernel(const float* __restrict__ probs, const long long* __restrict__ plan, int B, int K,
                                                          float* __restrict__ frame_scores, long long* __restrict__ frame_label) {
    __shared__ float sval[256];
    __shared__ int sidx[256];
    const long long f = blockIdx.x;
    const int tid = threadIdx.x;
    int cover = 0;
    for (int j = 0; j < B; ++j) {
        const long long s = plan[2 * j], L = plan[2 * j + 1];
        cover += (L >= 1 && s <= f && f < s + L) ? 1 : 0;
    }
    float best = 0.f;
    int arg = -1;
    for (int k = tid; k < K; k += 256) {
        double acc = 0.;
        for (int j = 0; j < B; ++j) {
            const long long s = plan[2 * j], L = plan[2 * j + 1];
            if (L >= 1 && s <= f && f < s + L) acc += (double)probs[(long long)j * K + k];
        }
        const float r = cover ? (float)(acc / (double)cover) : 0.f;
        frame_scores[f * K + k] = r;
        if (arg < 0 || r > best) { best = r; arg = k; }
    }
    const int lab = block_first_argmax(best, arg, sval, sidx);
    if (tid == 0) frame_label[f] = cover ? lab : -1;
}

// One workgroup.  A valid window moves the average (the first one sets it) and counts in *seen; an invalid one moves nothing.
__global__ __launch_bounds__(256) void score_ema_kernel(const float* __restrict__ probs, const long long* __restrict__ plan_row, int K, double beta,
                                                        double* __restrict__ ema, long long* __restrict__ seen, float* __restrict__ out,
                                                        long long* __restrict__ label, float* __restrict__ conf) {
    __shared__ double sval[256];
    __shared__ int sidx[256];
    const int tid = threadIdx.x;
    const bool valid = plan_row[1] >= 1;
    const long long seen0 = seen[0];
    double best = 0.;
    int arg = -1;
    for (int k = tid; k < K; k += 256) {
        double e = ema[k];
        if (valid) {
            const double p = (double)probs[k];
            e = seen0 == 0 ? p : beta * e + (1.0 - beta) * p;
            ema[k] = e;
        }
        out[k] = (float)e;
        if (arg < 0 || e > best) { best = e; arg = k; }
    }
    const int lab = block_first_argmax(best, arg, sval, sidx);     // its barriers stand between every read of *seen and the write
    if (tid == 0) {
        const long long now = seen0 + (valid ? 1 : 0);
        seen[0] = now;
        label[0] = now > 0 ? lab : -1;
        conf[0] = now > 0 ? (float)sval[0] : 0.f;                  // out[label]: the reduction carries the value with the index
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int tamgcn_ring_push(const void* frames, int n, int P, int R, int elem, void* ring, int cap, long long* state, void* stream) {
    TG_CHECK(frames && ring && state, "tamgcn_ring_push: null pointer");
    TG_CHECK(elem == 4 || elem == 8, "tamgcn_ring_push: elem %d (4: fp32 clip layout, 8: fp64 N-UCLA layout)", elem);
    TG_CHECK(P > 0 && R > 0 && cap > 0, "tamgcn_ring_push: bad dims P=%d R=%d cap=%d", P, R, cap);
    TG_CHECK(n >= 1 && n <= cap, "tamgcn_ring_push: n = %d frames outside 1..cap = %d", n, cap);
    TG_CHECK((long long)R * elem <= (1LL << 30), "tamgcn_ring_push: a frame row of %lld bytes is too large", (long long)R * elem);
    const long long rowbytes = (long long)R * elem;
    const bool vec = rowbytes % 16 == 0 && aligned16(frames) && aligned16(ring);
    const int units = (int)(vec ? rowbytes / 16 : R);
    const long long total = (long long)P * n * units;
    TG_CHECK((long long)P * cap * units < (1LL << 40) && total < (1LL << 31) * 256, "tamgcn_ring_push: ring too large (P=%d cap=%d R=%d)", P, cap, R);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (vec) hipLaunchKernelGGL(ring_push_kernel<uint4>, grid, block, 0, (hipStream_t)stream, (const uint4*)frames, n, units, total, (uint4*)ring, cap, state);
    else if (elem == 8) hipLaunchKernelGGL(ring_push_kernel<unsigned long long>, grid, block, 0, (hipStream_t)stream, (const unsigned long long*)frames, n, units, total, (unsigned long long*)ring, cap, state);
    else hipLaunchKernelGGL(ring_push_kernel<unsigned>, grid, block, 0, (hipStream_t)stream, (const unsigned*)frames, n, units, total, (unsigned*)ring, cap, state);
    tamgcn_note_kernel("ring_push_kernel<%d>", vec ? 16 : elem);
    TG_LAUNCH_CHECK("tamgcn_ring_push");
    hipLaunchKernelGGL(ring_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, n);
    TG_LAUNCH_CHECK("tamgcn_ring_push (advance)");
    return 0;
}

extern "C" int tamgcn_ring_plan(const long long* state, int cap, int B, int L, int hop, long long* plan, void* stream) {
    TG_CHECK(state && plan, "tamgcn_ring_plan: null pointer");
    TG_CHECK(cap > 0 && B > 0 && hop >= 1, "tamgcn_ring_plan: bad dims cap=%d B=%d hop=%d", cap, B, hop);
    TG_CHECK(L >= 1 && L <= cap, "tamgcn_ring_plan: window L = %d outside 1..cap = %d", L, cap);
    hipLaunchKernelGGL(ring_plan_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, state, cap, B, L, hop, plan);
    tamgcn_note_kernel("ring_plan_kernel");
    TG_LAUNCH_CHECK("tamgcn_ring_plan");
    return 0;
}

extern "C" int tamgcn_window_nucla(const double* ring, int cap, const long long* plan, int B, const int* parent, int V, int time_steps,
                                   int center_joint, int mode, float* out, void* stream) {
    TG_CHECK(ring && plan && parent && out, "tamgcn_window_nucla: null pointer");
    TG_CHECK(cap > 0 && B > 0 && V > 0, "tamgcn_window_nucla: bad dims cap=%d B=%d V=%d", cap, B, V);
    TG_CHECK(time_steps > 0 && time_steps <= STREAM_MAX_TS, "tamgcn_window_nucla: time_steps %d outside 1..%d", time_steps, STREAM_MAX_TS);
    TG_CHECK((long long)cap * V <= (1LL << 30) && V <= (1 << 20), "tamgcn_window_nucla: a ring of cap V = %lld positions is too large", (long long)cap * V);
    TG_CHECK(center_joint >= 0 && center_joint < V, "tamgcn_window_nucla: centre joint %d outside 0..%d", center_joint, V - 1);
    TG_CHECK(mode >= 0 && mode <= 3, "tamgcn_window_nucla: mode %d (0 joint, 1 bone, 2 motion, 3 bone-motion)", mode);
    hipLaunchKernelGGL(window_nucla_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, ring, cap, plan, parent, V, time_steps, center_joint,
                       mode, out);
    tamgcn_note_kernel("window_nucla_kernel");
    TG_LAUNCH_CHECK("tamgcn_window_nucla");
    return 0;
}

extern "C" int tamgcn_window_clip(const float* ring, int cap, const long long* plan, int B, int C, int V, int M, int W, float* out, void* stream) {
    TG_CHECK(ring && plan && out, "tamgcn_window_clip: null pointer");
    TG_CHECK(cap > 0 && B > 0 && C > 0 && V > 0 && M > 0 && W > 0, "tamgcn_window_clip: bad dims cap=%d B=%d C=%d V=%d M=%d W=%d", cap, B, C, V, M, W);
    TG_CHECK((long long)cap * V * M <= (1LL << 30) && (long long)W * V * M <= (1LL << 30),
             "tamgcn_window_clip: a channel plane above 2^30 elements (cap=%d W=%d V=%d M=%d)", cap, W, V, M);
    const int VM = V * M, rowlen = W * VM;
    const bool vec = VM % 4 == 0 && aligned16(ring) && aligned16(out);
    const int tiles = ceil_div(rowlen, 256 * (vec ? 4 : 1));
    const long long blocks = (long long)B * C * tiles;
    TG_CHECK(blocks < (1LL << 31), "tamgcn_window_clip: %lld workgroups", blocks);
    const dim3 grid((unsigned)blocks), block(256);
    if (vec) hipLaunchKernelGGL(window_clip_kernel<4>, grid, block, 0, (hipStream_t)stream, ring, cap, plan, C, W, VM, tiles, out);
    else hipLaunchKernelGGL(window_clip_kernel<1>, grid, block, 0, (hipStream_t)stream, ring, cap, plan, C, W, VM, tiles, out);
    tamgcn_note_kernel("window_clip_kernel<%d>", vec ? 4 : 1);
    TG_LAUNCH_CHECK("tamgcn_window_clip");
    return 0;
}

extern "C" int tamgcn_window_vote(const float* logits, const long long* plan, int B, int K, int n_frames, float* probs, float* frame_scores,
                                  long long* frame_label, void* stream) {
    TG_CHECK(logits && plan && probs, "tamgcn_window_vote: null pointer");
    TG_CHECK(B > 0 && K > 0 && K <= STREAM_MAX_K, "tamgcn_window_vote: bad dims B=%d K=%d (K at most %d)", B, K, STREAM_MAX_K);
    TG_CHECK((frame_scores == nullptr) == (frame_label == nullptr), "tamgcn_window_vote: frame_scores and frame_label go together");
    TG_CHECK(!frame_scores || n_frames > 0, "tamgcn_window_vote: n_frames = %d with frame outputs", n_frames);
    hipLaunchKernelGGL(window_softmax_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, K, probs);
    tamgcn_note_kernel("window_softmax_kernel");
    TG_LAUNCH_CHECK("tamgcn_window_vote");
    if (frame_scores) {
        hipLaunchKernelGGL(window_vote_kernel, dim3((unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, (const float*)probs, plan, B, K, frame_scores,
                           frame_label);
        tamgcn_note_kernel("window_vote_kernel");
        TG_LAUNCH_CHECK("tamgcn_window_vote (frames)");
    }
    return 0;
}

extern "C" int tamgcn_score_ema(const float* probs, const long long* plan_row, int K, double beta, double* ema, long long* seen, float* out,
                                long long* label, float* conf, void* stream) {
    TG_CHECK(probs && plan_row && ema && seen && out && label && conf, "tamgcn_score_ema: null pointer");
    TG_CHECK(K > 0 && K <= STREAM_MAX_K, "tamgcn_score_ema: K = %d outside 1..%d", K, STREAM_MAX_K);
    TG_CHECK(beta >= 0.0 && beta < 1.0, "tamgcn_score_ema: beta = %g outside [0, 1)", beta);   // NaN fails too
    hipLaunchKernelGGL(score_ema_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, probs, plan_row, K, beta, ema, seen, out, label, conf);
    tamgcn_note_kernel("score_ema_kernel");
    TG_LAUNCH_CHECK("tamgcn_score_ema");
    return 0;
}
