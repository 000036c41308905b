// Input-side kernels of the skeleton path: what the reference does per sample on the host in
// feeder/feeder_nucla_gcn.py:85-130 (centre, view transform, min-max to [-1, 1], resample to `time_steps` frames,
// bone / motion streams), as one workgroup per clip on the GPU, and the 4-stream derivation of BASELINE.json
// configs[2] from a joint batch that is already resident in HBM.
#include "common.h"
#include "feeder_common.h"

namespace {

// out = stream(x) over (N, C, T, V, M), V*M innermost.  mode 1: bone (x[v] - x[parent[v]]), 2: motion
// (x[t+1] - x[t], last frame 0), 3: motion of bone.
__global__ __launch_bounds__(256) void stream_derive_kernel(const float* __restrict__ x, const int* __restrict__ parent, int T, int V, int M,
                                                            int mode, long long total, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int VM = V * M;
    const int vm = (int)(e % VM);
    const long long row = e / VM;                     // (n, c, t)
    const int t = (int)(row % T);
    const int v = vm / M, m = vm - v * M;
    const int pv = parent[v] * M + m;
    const float* xr = x + row * VM;
    float cur = xr[vm];
    if (mode == 1) { out[e] = cur - xr[pv]; return; }
    if (t == T - 1) { out[e] = 0.f; return; }
    const float* xn = xr + VM;                        // frame t + 1
    if (mode == 2) { out[e] = xn[vm] - cur; return; }
    out[e] = (xn[vm] - xn[pv]) - (cur - xr[pv]);
}

struct FeederArgs {
    const double* raw;          // concatenated clips, (sum L, V, 3)
    const long long* offs;      // [N + 1] frame offsets
    const double* rot;          // [N][9] row-major view matrix Ry.Rx.S (points are row vectors: p' = p . R)
    const int* idx;             // [N][TS] source frame of every output frame
    const int* parent;          // [V] bone parent (0-based), used by the bone streams
    int N, V, TS, mode, center_joint;
    float* out;                 // (N, 3, TS, V, 1)
    const long long* clip_ids;  // INDEXED only: [N] clip of every slot, taken modulo n_clips; offs is then the split's [n_clips + 1]
    long long n_clips;
};

// One workgroup per clip, the body of feeder_common.h (shared with the ring's window builder, streaming.hip).
// INDEXED: slot n reads clip clip_ids[n] % n_clips of the resident split instead of clip n of a gathered copy; the
// arithmetic is this one body either way.
template <bool INDEXED>
__global__ __launch_bounds__(256) void feeder_transform_kernel(const FeederArgs a) {
    const int n = blockIdx.x, V = a.V, TS = a.TS;
    const long long c = INDEXED ? clip_of(a.clip_ids[n], a.n_clips) : n;
    const long long f0 = a.offs[c], L = a.offs[c + 1] - f0;
    const double* clip = a.raw + f0 * V * 3;
    const int* idx = a.idx + (long long)n * TS;
    feeder_transform_body([&](long long e) { return clip + e * 3; }, [&](int t) { return idx[t]; }, L, V, TS, a.mode, a.center_joint,
                          a.rot + (long long)n * 9, a.parent, a.out + (long long)n * 3 * TS * V);
}

// ---- the train path's draws on the device (Feeder.batch_device) ----------------------------------------------------
// (clip_of, val_frame and Philox4x32-10: feeder_common.h)
// o = a . b, 3 x 3 row-major, each entry summed left to right
__device__ __forceinline__ void mat3(const double* a, const double* b, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = a[i * 3 + 0] * b[0 + j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}

constexpr int DRAW_MAX_TS = 64;         // one lane per output frame

struct DrawArgs {
    const long long* offs;      // [n_clips + 1] frame offsets of the resident split
    const long long* clip_ids;  // [B], taken modulo n_clips
    const long long* labels;    // [n_clips] or null
    const long long* state;     // [2] = (seed, call counter), read here, advanced by feeder_advance_kernel
    const double* cossin;       // [121][2] = (cos, sin) of -60 .. 60 degrees as the host's libm gives them (train only)
    long long n_clips;
    int B, TS, train;
    double* view;               // [B][3] = (agx, agy, s)
    double* rot;                // [B][9]
    int* idx;                   // [B][TS]
    long long* labels_out;      // [B] or null
};

// One wave per batch slot.  The stream of draws is defined in INTEGRATION.md ("Training loop") and restated in numpy by
// tests/feeder_draws.py: block 0 of slot b gives the view, blocks 1 .. ceil(TS / 4) one word per output frame; Floyd's
// algorithm turns the words into TS distinct positions among the n = 100 L slots of `list(arange(L)) * 100` (reference
// feeder/feeder_nucla_gcn.py:112), position p holding frame p % L; the frames are sorted by ranking.
__global__ __launch_bounds__(64) void feeder_draw_kernel(const DrawArgs a) {
    __shared__ unsigned u[DRAW_MAX_TS];
    __shared__ int fr[DRAW_MAX_TS];
    const int b = blockIdx.x, lane = threadIdx.x, TS = a.TS;
    const long long clip = clip_of(a.clip_ids[b], a.n_clips);
    long long L = a.offs[clip + 1] - a.offs[clip];
    if (L < 1) L = 1;                                    // Feeder.load_data() refuses such a split; never divide by it
    if (lane == 0 && a.labels_out) a.labels_out[b] = a.labels[clip];
    int* idx = a.idx + (long long)b * TS;
    double* view = a.view + (long long)b * 3;
    double* rot = a.rot + (long long)b * 9;
    if (!a.train) {                                      // np.linspace(0, L - 1, TS).astype(int), reference :116
        if (lane < TS) idx[lane] = val_frame(lane, L, TS);
        if (lane < 9) rot[lane] = (lane % 4 == 0) ? 1.0 : 0.0;
        if (lane < 3) view[lane] = lane == 2 ? 1.0 : 0.0;
        return;
    }
    const unsigned long long seed = (unsigned long long)a.state[0], call = (unsigned long long)a.state[1];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), cl = (unsigned)call, ch = (unsigned)(call >> 32);
    if (lane < (TS + 3) / 4) {
        unsigned w[4];
        philox4x32_10(cl, ch, (unsigned)b, (unsigned)lane + 1u, k0, k1, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) u[4 * lane + q] = w[q];
    }
    if (lane == 0) {
        unsigned w[4];
        philox4x32_10(cl, ch, (unsigned)b, 0u, k0, k1, w);
        const int agx = -60 + (int)__umulhi(w[0], 121u), agy = -60 + (int)__umulhi(w[1], 121u);
        // 53 random bits: every step exact in fp64 but the last addition
        const double s = 0.5 + ((double)(w[2] >> 5) * 67108864.0 + (double)(w[3] >> 6)) * 0x1p-53;
        view[0] = (double)agx; view[1] = (double)agy; view[2] = s;
        const double cx = a.cossin[2 * (agx + 60)], sx = a.cossin[2 * (agx + 60) + 1];
        const double cy = a.cossin[2 * (agy + 60)], sy = a.cossin[2 * (agy + 60) + 1];
        const double Rx[9] = {1., 0., 0., 0., cx, sx, 0., -sx, cx};          // reference :75-83
        const double Ry[9] = {cy, 0., -sy, 0., 1., 0., sy, 0., cy};
        const double Ss[9] = {s, 0., 0., 0., s, 0., 0., 0., s};
        double t[9], R[9];
        mat3(Rx, Ss, t);
        mat3(Ry, t, R);                                                       // np.dot(Ry, np.dot(Rx, Ss))
#pragma unroll
        for (int e = 0; e < 9; ++e) rot[e] = R[e];
    }
    __syncthreads();
    const unsigned long long n = 100ull * (unsigned long long)L;           // >= 100 > DRAW_MAX_TS
    long long mine = -1;                                                    // lane i keeps the position step i took
    for (int i = 0; i < TS; ++i) {
        const unsigned long long J = n - (unsigned long long)TS + (unsigned long long)i;
        const long long t = (long long)(((unsigned long long)u[i] * (J + 1)) >> 32);      // uniform in [0, J]
        const bool taken = __ballot(mine == t) != 0;
        if (lane == i) mine = taken ? (long long)J : t;
    }
    const int f = lane < TS ? (int)(mine % L) : 0;
    fr[lane] = f;
    __syncthreads();
    if (lane < TS) {
        int rank = 0;
        for (int j = 0; j < TS; ++j) {
            const int g = fr[j];
            rank += (g < f || (g == f && j < lane)) ? 1 : 0;
        }
        idx[rank] = f;
    }
}

// the call counter moves on the device, after the draw of this call has read it (same stream): a graph that holds both
// launches draws a new batch on every replay
__global__ void feeder_advance_kernel(long long* __restrict__ state) { state[1] = state[1] + 1; }

}  // namespace

extern "C" int tamgcn_stream_derive(const float* x, int N, int C, int T, int V, int M, const int* parent, int mode, float* out, void* stream) {
    TG_CHECK(x && parent && out, "tamgcn_stream_derive: null pointer");
    TG_CHECK(N > 0 && C > 0 && T > 0 && V > 0 && M > 0, "tamgcn_stream_derive: bad dims N=%d C=%d T=%d V=%d M=%d", N, C, T, V, M);
    TG_CHECK(mode >= 1 && mode <= 3, "tamgcn_stream_derive: mode %d (1 bone, 2 motion, 3 bone-motion)", mode);
    const long long total = (long long)N * C * T * V * M;
    TG_CHECK(total < (1LL << 31) * 256, "tamgcn_stream_derive: tensor too large");
    hipLaunchKernelGGL(stream_derive_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, parent, T, V, M, mode, total, out);
    tamgcn_note_kernel("stream_derive_kernel");
    TG_LAUNCH_CHECK("tamgcn_stream_derive");
    return 0;
}

extern "C" int tamgcn_feeder_transform(const double* raw, const long long* offsets, const double* rot, const int* idx, const int* parent,
                                       int N, int V, int time_steps, int center_joint, int mode, float* out, void* stream) {
    TG_CHECK(raw && offsets && rot && idx && parent && out, "tamgcn_feeder_transform: null pointer");
    TG_CHECK(N > 0 && V > 0 && time_steps > 0, "tamgcn_feeder_transform: bad dims N=%d V=%d time_steps=%d", N, V, time_steps);
    TG_CHECK(center_joint >= 0 && center_joint < V, "tamgcn_feeder_transform: centre joint %d outside 0..%d", center_joint, V - 1);
    TG_CHECK(mode >= 0 && mode <= 3, "tamgcn_feeder_transform: mode %d (0 joint, 1 bone, 2 motion, 3 bone-motion)", mode);
    FeederArgs a;
    a.raw = raw; a.offs = offsets; a.rot = rot; a.idx = idx; a.parent = parent;
    a.N = N; a.V = V; a.TS = time_steps; a.mode = mode; a.center_joint = center_joint; a.out = out;
    a.clip_ids = nullptr; a.n_clips = 0;
    hipLaunchKernelGGL(feeder_transform_kernel<false>, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("feeder_transform_kernel");
    TG_LAUNCH_CHECK("tamgcn_feeder_transform");
    return 0;
}

extern "C" int tamgcn_feeder_draw(const long long* offsets, long long n_clips, const long long* clip_ids, int B, const long long* labels,
                                  long long* state, const double* cossin, int time_steps, int train, double* view, double* rot, int* idx,
                                  long long* labels_out, void* stream) {
    TG_CHECK(offsets && clip_ids && state && view && rot && idx, "tamgcn_feeder_draw: null pointer");
    TG_CHECK(B > 0 && n_clips > 0, "tamgcn_feeder_draw: bad dims B=%d n_clips=%lld", B, n_clips);
    TG_CHECK(time_steps > 0 && time_steps <= DRAW_MAX_TS, "tamgcn_feeder_draw: time_steps %d outside 1..%d", time_steps, DRAW_MAX_TS);
    TG_CHECK(train == 0 || train == 1, "tamgcn_feeder_draw: train %d (0 val, 1 train)", train);
    TG_CHECK(!train || cossin, "tamgcn_feeder_draw: the train path needs the cos/sin table");
    TG_CHECK((labels == nullptr) == (labels_out == nullptr), "tamgcn_feeder_draw: labels and labels_out go together");
    DrawArgs a;
    a.offs = offsets; a.clip_ids = clip_ids; a.labels = labels; a.state = state; a.cossin = cossin; a.n_clips = n_clips;
    a.B = B; a.TS = time_steps; a.train = train; a.view = view; a.rot = rot; a.idx = idx; a.labels_out = labels_out;
    hipLaunchKernelGGL(feeder_draw_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("feeder_draw_kernel");
    TG_LAUNCH_CHECK("tamgcn_feeder_draw");
    if (train) {                                        // the val path consumes nothing of the stream
        hipLaunchKernelGGL(feeder_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
        TG_LAUNCH_CHECK("tamgcn_feeder_draw (advance)");
    }
    return 0;
}

extern "C" int tamgcn_feeder_transform_indexed(const double* raw, const long long* offsets, long long n_clips, const long long* clip_ids,
                                               const double* rot, const int* idx, const int* parent, int B, int V, int time_steps,
                                               int center_joint, int mode, float* out, void* stream) {
    TG_CHECK(raw && offsets && clip_ids && rot && idx && parent && out, "tamgcn_feeder_transform_indexed: null pointer");
    TG_CHECK(B > 0 && n_clips > 0 && V > 0 && time_steps > 0, "tamgcn_feeder_transform_indexed: bad dims B=%d n_clips=%lld V=%d time_steps=%d",
             B, n_clips, V, time_steps);
    TG_CHECK(center_joint >= 0 && center_joint < V, "tamgcn_feeder_transform_indexed: centre joint %d outside 0..%d", center_joint, V - 1);
    TG_CHECK(mode >= 0 && mode <= 3, "tamgcn_feeder_transform_indexed: mode %d (0 joint, 1 bone, 2 motion, 3 bone-motion)", mode);
    FeederArgs a;
    a.raw = raw; a.offs = offsets; a.rot = rot; a.idx = idx; a.parent = parent;
    a.N = B; a.V = V; a.TS = time_steps; a.mode = mode; a.center_joint = center_joint; a.out = out;
    a.clip_ids = clip_ids; a.n_clips = n_clips;
    hipLaunchKernelGGL(feeder_transform_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("feeder_transform_kernel<indexed>");
    TG_LAUNCH_CHECK("tamgcn_feeder_transform_indexed");
    return 0;
}
