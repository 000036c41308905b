// Live and sliding-window inference (tam_gcn_amd/streaming.py): a bank of S rings of skeleton frames in HBM, one ring per feed,
// that is pushed to without the host, the model's input windows built straight from the rings through either feeder's val-path
// arithmetic (feeder_common.h: the bodies feeder.hip and clipfeeder.hip run), and what a sliding-window user does with the
// scores: softmax, per-frame voting, an exponential moving average per feed, a debounced decision log.  One ring is a bank of
// S = 1 without counts or restarts: the single-ring entry points forward to the bank's.  include/tamgcn.h has the contract.
//
// Frames are numbered absolutely from 0 (the first frame a feed was ever pushed); frame f lives in slot f % cap of a ring that is
// logically (P, cap, R): (1, cap, V 3) fp64 for the N-UCLA transform, (C, cap, V M) fp32 for the clip feeder's layout; feed s is
// at s * (P cap R).  A sequence that is resident as a whole is a ring of cap = its length that never wraps.  No floating-point
// atomics anywhere: every sum has one order, so two calls give the same bits and a graph replay gives the eager call's.
#include "common.h"
#include "feeder_common.h"

namespace {

constexpr int STREAM_MAX_TS = 64;        // the N-UCLA window's time_steps (the feeder's draw kernel has the same limit)
constexpr int STREAM_MAX_K = 4096;       // classes: one softmax row as fp64 in LDS
constexpr int BANK_MAX_FEEDS = 1024;     // bank_decide_kernel: one workgroup, four feeds per thread

// Python's f % cap for cap > 0: slot of frame f (f >= 0 wherever a valid window reads)
__device__ __forceinline__ long long slot_of(long long f, int cap) { return clip_of(f, cap); }

// ---- the rings -------------------------------------------------------------------------------------------------------
// what feed s takes of a tick's n frames, and whether it is forgotten first (counts, restart: int32 [S] or null)
__device__ __forceinline__ int bank_take(const int* __restrict__ counts, int s, int n) { return counts ? min(max(counts[s], 0), n) : n; }
__device__ __forceinline__ bool bank_fresh(const int* __restrict__ restart, int s) { return restart && restart[s] != 0; }

// blockIdx.y = feed; one thread per unit U (16 bytes where the rows and addresses allow it, else one element) of the feed's
// (P, n, R) frames; frame i of the push goes to slot (count + i) % cap of every plane.  A restarted feed's count reads as 0; a
// unit of a frame beyond the feed's take stores nothing (and is not loaded).  count is read here and moved by
// bank_advance_kernel behind this launch on the same stream, so a graph that holds both pushes to new slots on every replay.
template <class U>
__global__ __launch_bounds__(256) void bank_push_kernel(const U* __restrict__ frames, int n, int units, long long total, U* __restrict__ ring,
                                                        int cap, long long ring_units, const long long* __restrict__ state,
                                                        const int* __restrict__ counts, const int* __restrict__ restart) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int s = blockIdx.y;
    const int u = (int)(e % units);
    const long long row = e / units;                   // (p, i)
    const int i = (int)(row % n);
    const long long p = row / n;
    const long long slot = slot_of((bank_fresh(restart, s) ? 0 : state[2 * s]) + i, cap);
    if (i < bank_take(counts, s, n)) ring[s * ring_units + (p * cap + slot) * units + u] = frames[s * total + e];
}

// one thread per feed: the restart first, then the clamped count.  A feed that takes nothing and is not restarted keeps its state.
__global__ __launch_bounds__(256) void bank_advance_kernel(long long* __restrict__ state, int S, int n, const int* __restrict__ counts,
                                                           const int* __restrict__ restart) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const bool fresh = bank_fresh(restart, s);
    const int take = bank_take(counts, s, n);
    if (!fresh && take == 0) return;
    state[2 * s] = (fresh ? 0 : state[2 * s]) + take;
    state[2 * s + 1] = (fresh ? 0 : state[2 * s + 1]) + (take > 0 ? 1 : 0);
}

// Window w of S B is window j = w % B of feed w / B: it ends (B - 1 - j) hop frames before the feed's newest frame; (0, 0) where
// it would start before frame 0 or before count - cap (already overwritten), and for a feed that takes no frame this tick.
__global__ __launch_bounds__(64) void bank_plan_kernel(const long long* __restrict__ state, const int* __restrict__ counts, int S, int cap, int B,
                                                       int L, int hop, long long* __restrict__ plan) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= S * B) return;
    const int s = w / B, j = w - s * B;
    const long long count = state[2 * s];
    const long long start = count - (long long)(B - 1 - j) * hop - L;
    const bool valid = !(counts && counts[s] <= 0) && start >= 0 && start >= count - cap;
    plan[2 * w] = valid ? start : 0;
    plan[2 * w + 1] = valid ? L : 0;
}

// a plan row the window builders accept: anything else is an invalid window (zeros)
__device__ __forceinline__ bool window_ok(long long start, long long L, int cap) { return start >= 0 && L >= 1 && L <= cap; }

// ---- windows -----------------------------------------------------------------------------------------------------------
// One workgroup per window, window b of S B on the ring of feed b / B: feeder_transform_kernel's body on the window's L frames
// with the identity view and the val path's frame indices.
__global__ __launch_bounds__(256) void bank_window_nucla_kernel(const double* __restrict__ bank, int cap, const long long* __restrict__ plan, int B,
                                                                const int* __restrict__ parent, int V, int TS, int center_joint, int mode,
                                                                float* __restrict__ out) {
    const int b = blockIdx.x;
    const double* ring = bank + (long long)(blockIdx.x / (unsigned)B) * cap * V * 3;
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
// positions); window b of S B reads the ring of feed b / B, (C, cap, VM) floats apart.  clip_resize_kernel's taps and blend on
// the crop (start, L), the two source frames fetched at their ring slots.  VEC = 4 only where V M is a multiple of four and both
// arrays are 16-byte aligned: a span then lies inside one frame.
template <int VEC>
__global__ __launch_bounds__(256) void bank_window_clip_kernel(const float* __restrict__ ring, int cap, const long long* __restrict__ plan, int B,
                                                               int C, int W, int VM, int tiles, float* __restrict__ out) {
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
        const float* src = ring + (long long)((b / B) * C + c) * cap * VM + vm;
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

// One workgroup per feed: the feed's B windows (probs and plan rows s B + j) update its average oldest first, every thread its
// own classes k = tid, tid + 256, ... in every window, so the windows need no barrier between them.  A valid window moves the
// average (the feed's first one ever sets it) and counts in seen[s]; an invalid one moves nothing.  A restarted feed's average
// reads as zeros and its seen as 0, and both are stored either way.  out = the rounded average after the last window, label its
// first arg max (taken once), conf = out[label]; -1 and 0 before the feed's first valid window.  advanced (may be null): 1 where
// seen moved.
__global__ __launch_bounds__(256) void bank_ema_kernel(const float* __restrict__ probs, const long long* __restrict__ plan,
                                                       const int* __restrict__ restart, int B, int K, double beta, double* __restrict__ ema,
                                                       long long* __restrict__ seen, float* __restrict__ out, long long* __restrict__ label,
                                                       float* __restrict__ conf, int* __restrict__ advanced) {
    __shared__ double sval[256];
    __shared__ int sidx[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool fresh0 = bank_fresh(restart, s);
    const long long seen0 = fresh0 ? 0 : seen[s];
    double* avg = ema + (long long)s * K;
    float* o = out + (long long)s * K;
    long long now = seen0;
    double best = 0.;
    int arg = -1;                                      // the thread's first largest class of the last window
    for (int j = 0; j < B; ++j) {
        const long long w = (long long)s * B + j;
        const bool valid = plan[2 * w + 1] >= 1, fresh = fresh0 && j == 0;
        arg = -1;
        for (int k = tid; k < K; k += 256) {
            double e = fresh ? 0. : avg[k];
            if (valid) {
                const double p = (double)probs[w * K + k];
                e = now == 0 ? p : beta * e + (1.0 - beta) * p;
            }
            if (valid || fresh) avg[k] = e;
            o[k] = (float)e;
            if (arg < 0 || e > best) { best = e; arg = k; }
        }
        now += valid ? 1 : 0;
    }
    const int lab = block_first_argmax(best, arg, sval, sidx);     // its barriers stand between every read of seen[s] and the write
    if (tid == 0) {
        seen[s] = now;
        label[s] = now > 0 ? lab : -1;
        conf[s] = now > 0 ? (float)sval[0] : 0.f;      // out[label]: the reduction carries the value with the index
        if (advanced) advanced[s] = now > seen0 ? 1 : 0;
    }
}

// One workgroup of 256 threads, thread t owning feeds 4 t .. 4 t + 3 (S <= 1024): the debounce update of every feed, then an
// exclusive scan of "this feed has an event" over the feeds in ascending order gives every event its row, so the log has one
// order and no atomics.  deb int64 (S, 3) = (stable, cand, run); count int64 [2] = (written, dropped).
__global__ __launch_bounds__(256) void bank_decide_kernel(const long long* __restrict__ label, const float* __restrict__ conf,
                                                          const int* __restrict__ advanced, const int* __restrict__ restart,
                                                          const long long* __restrict__ state, int S, float threshold, long long hold,
                                                          long long* __restrict__ deb, long long* __restrict__ rows, float* __restrict__ rconf,
                                                          long long* __restrict__ count, long long capacity) {
    __shared__ int wave_sum[256 / 64];
    const int tid = threadIdx.x;
    int ev[4];
    int mine = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = 4 * tid + q;
        ev[q] = 0;
        if (s >= S) continue;
        const bool fresh = bank_fresh(restart, s);
        long long stable = fresh ? -1 : deb[3 * s], cand = fresh ? -1 : deb[3 * s + 1], run = fresh ? 0 : deb[3 * s + 2];
        if (advanced[s]) {
            const long long lab = label[s];
            if (conf[s] >= threshold) {
                if (lab == cand) run += 1;
                else { cand = lab; run = 1; }
            } else {
                cand = -1;
                run = 0;
            }
            if (run >= hold && cand != stable) { stable = cand; ev[q] = 1; }
        }
        deb[3 * s] = stable; deb[3 * s + 1] = cand; deb[3 * s + 2] = run;
        mine += ev[q];
    }
    int incl = mine;                                   // inclusive scan over the wave, then over the four waves
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if ((tid & 63) >= off) incl += v;
    }
    if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < (tid >> 6)) before += wave_sum[w];
        total += wave_sum[w];
    }
    const long long written = count[0];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = 4 * tid + q;
        if (!ev[q]) continue;
        const long long at = written + before;
        ++before;
        if (at >= capacity) continue;                  // a full log drops the event, it never overwrites
        rows[3 * at] = s; rows[3 * at + 1] = state[2 * s] - 1; rows[3 * at + 2] = label[s];
        rconf[at] = conf[s];
    }
    __syncthreads();                                   // every read of count[0] is behind us
    if (tid == 0) {
        const long long room = capacity > written ? capacity - written : 0;
        const long long kept = total < room ? total : room;
        count[0] = written + kept;
        count[1] = count[1] + (total - kept);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- one host body per operation: `who` is the entry point that was called; one ring is S = 1 with null counts and restart ------
#define TG_FEEDS(who, S) TG_CHECK((S) >= 1 && (S) <= BANK_MAX_FEEDS, "%s: S = %d feeds outside 1..%d", who, S, BANK_MAX_FEEDS)

int push(const char* who, const void* frames, int S, int n, int P, int R, int elem, void* ring, int cap, long long* state, const int* counts,
         const int* restart, hipStream_t stream) {
    TG_CHECK(frames && ring && state, "%s: null pointer", who);
    TG_FEEDS(who, S);
    TG_CHECK(elem == 4 || elem == 8, "%s: elem %d (4: fp32 clip layout, 8: fp64 N-UCLA layout)", who, elem);
    TG_CHECK(P > 0 && R > 0 && cap > 0, "%s: bad dims P=%d R=%d cap=%d", who, P, R, cap);
    TG_CHECK(n >= 1 && n <= cap, "%s: n = %d frames outside 1..cap = %d", who, n, cap);
    TG_CHECK((long long)R * elem <= (1LL << 30), "%s: a frame row of %lld bytes is too large", who, (long long)R * elem);
    const long long rowbytes = (long long)R * elem;
    const bool vec = rowbytes % 16 == 0 && aligned16(frames) && aligned16(ring);       // the feed strides P n rowbytes and P cap rowbytes
    const int units = (int)(vec ? rowbytes / 16 : R);                                  // are multiples of 16 with the rows
    const long long total = (long long)P * n * units, ring_units = (long long)P * cap * units;
    TG_CHECK(ring_units * S < (1LL << 40) && total < (1LL << 31) * 256, "%s: bank too large (S=%d P=%d cap=%d R=%d)", who, S, P, cap, R);
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)S), block(256);
    if (vec) hipLaunchKernelGGL(bank_push_kernel<uint4>, grid, block, 0, stream, (const uint4*)frames, n, units, total, (uint4*)ring, cap, ring_units, state, counts, restart);
    else if (elem == 8) hipLaunchKernelGGL(bank_push_kernel<unsigned long long>, grid, block, 0, stream, (const unsigned long long*)frames, n, units, total, (unsigned long long*)ring, cap, ring_units, state, counts, restart);
    else hipLaunchKernelGGL(bank_push_kernel<unsigned>, grid, block, 0, stream, (const unsigned*)frames, n, units, total, (unsigned*)ring, cap, ring_units, state, counts, restart);
    tamgcn_note_kernel("bank_push_kernel<%d>", vec ? 16 : elem);
    TG_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(bank_advance_kernel, dim3((unsigned)ceil_div(S, 256)), dim3(256), 0, stream, state, S, n, counts, restart);
    TG_LAUNCH_CHECK(who);
    return 0;
}

int plan_windows(const char* who, const long long* state, const int* counts, int S, int cap, int B, int L, int hop, long long* plan,
                 hipStream_t stream) {
    TG_CHECK(state && plan, "%s: null pointer", who);
    TG_FEEDS(who, S);
    TG_CHECK(cap > 0 && B > 0 && hop >= 1, "%s: bad dims cap=%d B=%d hop=%d", who, cap, B, hop);
    TG_CHECK(L >= 1 && L <= cap, "%s: window L = %d outside 1..cap = %d", who, L, cap);
    TG_CHECK((long long)S * B < (1LL << 30), "%s: S B = %lld windows", who, (long long)S * B);
    hipLaunchKernelGGL(bank_plan_kernel, dim3((unsigned)ceil_div(S * B, 64)), dim3(64), 0, stream, state, counts, S, cap, B, L, hop, plan);
    tamgcn_note_kernel("bank_plan_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int window_nucla(const char* who, const double* ring, int S, int cap, const long long* plan, int B, const int* parent, int V, int time_steps,
                 int center_joint, int mode, float* out, hipStream_t stream) {
    TG_CHECK(ring && plan && parent && out, "%s: null pointer", who);
    TG_FEEDS(who, S);
    TG_CHECK(cap > 0 && B > 0 && V > 0, "%s: bad dims cap=%d B=%d V=%d", who, cap, B, V);
    TG_CHECK(time_steps > 0 && time_steps <= STREAM_MAX_TS, "%s: time_steps %d outside 1..%d", who, time_steps, STREAM_MAX_TS);
    TG_CHECK((long long)cap * V <= (1LL << 30) && V <= (1 << 20), "%s: a ring of cap V = %lld positions is too large", who, (long long)cap * V);
    TG_CHECK(center_joint >= 0 && center_joint < V, "%s: centre joint %d outside 0..%d", who, center_joint, V - 1);
    TG_CHECK(mode >= 0 && mode <= 3, "%s: mode %d (0 joint, 1 bone, 2 motion, 3 bone-motion)", who, mode);
    TG_CHECK((long long)S * B < (1LL << 30), "%s: S B = %lld windows", who, (long long)S * B);
    hipLaunchKernelGGL(bank_window_nucla_kernel, dim3((unsigned)(S * B)), dim3(256), 0, stream, ring, cap, plan, B, parent, V, time_steps, center_joint,
                       mode, out);
    tamgcn_note_kernel("bank_window_nucla_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

int window_clip(const char* who, const float* ring, int S, int cap, const long long* plan, int B, int C, int V, int M, int W, float* out,
                hipStream_t stream) {
    TG_CHECK(ring && plan && out, "%s: null pointer", who);
    TG_FEEDS(who, S);
    TG_CHECK(cap > 0 && B > 0 && C > 0 && V > 0 && M > 0 && W > 0, "%s: bad dims cap=%d B=%d C=%d V=%d M=%d W=%d", who, cap, B, C, V, M, W);
    TG_CHECK((long long)cap * V * M <= (1LL << 30) && (long long)W * V * M <= (1LL << 30),
             "%s: a channel plane above 2^30 elements (cap=%d W=%d V=%d M=%d)", who, cap, W, V, M);
    TG_CHECK((long long)S * B < (1LL << 30) && (long long)S * C < (1LL << 30), "%s: S B = %lld windows, S C = %lld planes", who, (long long)S * B,
             (long long)S * C);
    const int VM = V * M, rowlen = W * VM;
    const bool vec = VM % 4 == 0 && aligned16(ring) && aligned16(out);      // the feed stride C cap VM is a multiple of four with VM
    const int tiles = ceil_div(rowlen, 256 * (vec ? 4 : 1));
    const long long blocks = (long long)S * B * C * tiles;
    TG_CHECK(blocks < (1LL << 31), "%s: %lld workgroups", who, blocks);
    const dim3 grid((unsigned)blocks), block(256);
    if (vec) hipLaunchKernelGGL(bank_window_clip_kernel<4>, grid, block, 0, stream, ring, cap, plan, B, C, W, VM, tiles, out);
    else hipLaunchKernelGGL(bank_window_clip_kernel<1>, grid, block, 0, stream, ring, cap, plan, B, C, W, VM, tiles, out);
    tamgcn_note_kernel("bank_window_clip_kernel<%d>", vec ? 4 : 1);
    TG_LAUNCH_CHECK(who);
    return 0;
}

// advanced may be null (tamgcn_score_ema has no such output)
int score_ema(const char* who, const float* probs, const long long* plan, const int* restart, int S, int B, int K, double beta, double* ema,
              long long* seen, float* out, long long* label, float* conf, int* advanced, hipStream_t stream) {
    TG_CHECK(probs && plan && ema && seen && out && label && conf, "%s: null pointer", who);
    TG_FEEDS(who, S);
    TG_CHECK(B > 0 && (long long)S * B < (1LL << 30), "%s: B = %d windows per feed", who, B);
    TG_CHECK(K > 0 && K <= STREAM_MAX_K, "%s: K = %d outside 1..%d", who, K, STREAM_MAX_K);
    TG_CHECK(beta >= 0.0 && beta < 1.0, "%s: beta = %g outside [0, 1)", who, beta);   // NaN fails too
    hipLaunchKernelGGL(bank_ema_kernel, dim3((unsigned)S), dim3(256), 0, stream, probs, plan, restart, B, K, beta, ema, seen, out, label, conf,
                       advanced);
    tamgcn_note_kernel("bank_ema_kernel");
    TG_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

// ---- one ring: the bank's bodies at S = 1, every frame taken, no restart ---------------------------------------------------------
extern "C" int tamgcn_ring_push(const void* frames, int n, int P, int R, int elem, void* ring, int cap, long long* state, void* stream) {
    return push("tamgcn_ring_push", frames, 1, n, P, R, elem, ring, cap, state, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int tamgcn_ring_plan(const long long* state, int cap, int B, int L, int hop, long long* plan, void* stream) {
    return plan_windows("tamgcn_ring_plan", state, nullptr, 1, cap, B, L, hop, plan, (hipStream_t)stream);
}

extern "C" int tamgcn_window_nucla(const double* ring, int cap, const long long* plan, int B, const int* parent, int V, int time_steps,
                                   int center_joint, int mode, float* out, void* stream) {
    return window_nucla("tamgcn_window_nucla", ring, 1, cap, plan, B, parent, V, time_steps, center_joint, mode, out, (hipStream_t)stream);
}

extern "C" int tamgcn_window_clip(const float* ring, int cap, const long long* plan, int B, int C, int V, int M, int W, float* out, void* stream) {
    return window_clip("tamgcn_window_clip", ring, 1, cap, plan, B, C, V, M, W, out, (hipStream_t)stream);
}

extern "C" int tamgcn_score_ema(const float* probs, const long long* plan_row, int K, double beta, double* ema, long long* seen, float* out,
                                long long* label, float* conf, void* stream) {
    return score_ema("tamgcn_score_ema", probs, plan_row, nullptr, 1, 1, K, beta, ema, seen, out, label, conf, nullptr, (hipStream_t)stream);
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

// ---- the bank ------------------------------------------------------------------------------------------------------------------
extern "C" int tamgcn_bank_push(const void* frames, int S, int n, int P, int R, int elem, void* ring, int cap, long long* state, const int* counts,
                                const int* restart, void* stream) {
    return push("tamgcn_bank_push", frames, S, n, P, R, elem, ring, cap, state, counts, restart, (hipStream_t)stream);
}

extern "C" int tamgcn_bank_plan(const long long* state, const int* counts, int S, int cap, int B, int L, int hop, long long* plan, void* stream) {
    return plan_windows("tamgcn_bank_plan", state, counts, S, cap, B, L, hop, plan, (hipStream_t)stream);
}

extern "C" int tamgcn_bank_window_nucla(const double* ring, int S, int cap, const long long* plan, int B, const int* parent, int V, int time_steps,
                                        int center_joint, int mode, float* out, void* stream) {
    return window_nucla("tamgcn_bank_window_nucla", ring, S, cap, plan, B, parent, V, time_steps, center_joint, mode, out, (hipStream_t)stream);
}

extern "C" int tamgcn_bank_window_clip(const float* ring, int S, int cap, const long long* plan, int B, int C, int V, int M, int W, float* out,
                                       void* stream) {
    return window_clip("tamgcn_bank_window_clip", ring, S, cap, plan, B, C, V, M, W, out, (hipStream_t)stream);
}

extern "C" int tamgcn_bank_ema(const float* probs, const long long* plan, const int* restart, int S, int B, int K, double beta, double* ema,
                               long long* seen, float* out, long long* label, float* conf, int* advanced, void* stream) {
    TG_CHECK(advanced, "tamgcn_bank_ema: null pointer");
    return score_ema("tamgcn_bank_ema", probs, plan, restart, S, B, K, beta, ema, seen, out, label, conf, advanced, (hipStream_t)stream);
}

extern "C" int tamgcn_bank_decide(const long long* label, const float* conf, const int* advanced, const int* restart, const long long* state, int S,
                                  float threshold, int hold, long long* deb, long long* log_rows, float* log_conf, long long* log_count,
                                  int log_capacity, void* stream) {
    TG_CHECK(label && conf && advanced && state && deb && log_rows && log_conf && log_count, "tamgcn_bank_decide: null pointer");
    TG_CHECK(S >= 1 && S <= BANK_MAX_FEEDS, "tamgcn_bank_decide: S = %d feeds outside 1..%d", S, BANK_MAX_FEEDS);
    TG_CHECK(threshold == threshold, "tamgcn_bank_decide: threshold is NaN");
    TG_CHECK(hold >= 1, "tamgcn_bank_decide: hold = %d below 1", hold);
    TG_CHECK(log_capacity >= 1, "tamgcn_bank_decide: log_capacity = %d below 1", log_capacity);
    hipLaunchKernelGGL(bank_decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, label, conf, advanced, restart, state, S, threshold,
                       (long long)hold, deb, log_rows, log_conf, log_count, (long long)log_capacity);
    tamgcn_note_kernel("bank_decide_kernel");
    TG_LAUNCH_CHECK("tamgcn_bank_decide");
    return 0;
}
