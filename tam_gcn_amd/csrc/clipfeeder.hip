// The feeder for fixed-shape skeleton arrays (N, C, T, V, M) -- NTU, Kinetics-skeleton, COCO / OpenPose keypoints, anything the
// ST-GCN / CTR-GCN data tools write -- with the whole split resident in HBM: what the reference does per sample on the host in
// feeder/feeder_nucla_fusion.py:95-106 through feeder/tools.py (random_shift :118-130, random_choose / auto_pading :39-62, the
// centre crop, random_move :65-115).  Shift and window compose to three integers per batch slot (the "plan": output frame t is
// raw frame src0 + t for lo <= t < hi and zero elsewhere), so no intermediate clip exists; the move is a per-frame 2 x 2 map of
// the x and y planes in fp64.  A second mode, not from the reference, is the pipeline CTR-GCN was published with: a crop (start, L)
// of the valid frames resized linearly in time to the window, then one 3-D rotation per clip (clip_crop_draw_kernel,
// clip_resize_kernel).  include/tamgcn.h has the contract and the definition of the draw stream.
#include "common.h"
#include "feeder_common.h"

namespace {

constexpr int CLIP_MAX_NODE = 16;       // move_time <= 8: np.arange gives 8 or 9 nodes, W is appended

// ---- (begin, end) of every resident clip: first valid frame, last valid frame + 1; a frame is valid iff any of its C V M
// elements != 0 (NaN counts, -0.0 does not: numpy's and IEEE's !=).  One workgroup per clip; the smallest and the largest
// in-plane position (t VM + vm) of a non-zero element give the two frames, so the loop divides nothing.
template <int VEC>
__global__ __launch_bounds__(256) void clip_extent_kernel(const float* __restrict__ raw, int C, int T, int VM, int* __restrict__ extent) {
    __shared__ int smin[4], smax[4];
    const int tid = threadIdx.x;
    const int plane = T * VM;
    const float* p = raw + (long long)blockIdx.x * C * plane;
    int emin = plane, emax = -1;
    for (int c = 0; c < C; ++c, p += plane) {
        for (int e = tid * VEC; e < plane; e += 256 * VEC) {
            if constexpr (VEC == 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(p + e);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (v[j] != 0.f) { emin = min(emin, e + j); emax = max(emax, e + j); }
            } else {
                if (p[e] != 0.f) { emin = min(emin, e); emax = max(emax, e); }
            }
        }
    }
    for (int off = 1; off < 64; off <<= 1) {
        emin = min(emin, __shfl_xor(emin, off));
        emax = max(emax, __shfl_xor(emax, off));
    }
    if ((tid & 63) == 0) { smin[tid >> 6] = emin; smax[tid >> 6] = emax; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { emin = min(emin, smin[w]); emax = max(emax, smax[w]); }
        extent[2 * (long long)blockIdx.x + 0] = emax < 0 ? 0 : emin / VM;
        extent[2 * (long long)blockIdx.x + 1] = emax < 0 ? T : emax / VM + 1;
    }
}

// ---- the draws of one batch: one thread per slot -------------------------------------------------------------------------
struct ClipDrawArgs {
    const int* extent;          // [n_clips][2]
    const long long* clip_ids;  // [B], taken modulo n_clips
    const long long* labels;    // [n_clips] or null
    const long long* state;     // [2] = (seed, call counter), read here, advanced by clip_advance_kernel
    const double* angle;        // candidate tables [nA], [nS], [nT] (with keys; null otherwise)
    const double* scale;
    const double* trans;
    long long n_clips;
    int B, T, W, num_node, nA, nS, nT, flags;
    int* plan;                  // [B][3] = (src0, lo, hi)
    int* draws;                 // [B][2] = (bias, d)
    int* move_idx;              // [B][num_node][4] or null (no move)
    double* keys;               // [B][num_node][4] = (angle in degrees, scale, t_x, t_y) or null
    long long* labels_out;      // [B] or null
};

__global__ __launch_bounds__(64) void clip_draw_kernel(const ClipDrawArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const long long clip = clip_of(a.clip_ids[b], a.n_clips);
    if (a.labels_out) a.labels_out[b] = a.labels[clip];
    const bool shift = a.flags & 1, choose = a.flags & 2, move = a.flags & 4;
    const int T = a.T, W = a.W;
    const unsigned long long seed = (unsigned long long)a.state[0], call = (unsigned long long)a.state[1];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), cl = (unsigned)call, ch = (unsigned)(call >> 32);
    int begin = 0, size = T;
    if (shift) {
        begin = a.extent[2 * clip];
        size = min(max(a.extent[2 * clip + 1] - begin, 0), T);        // tamgcn_clip_extent gives 1 .. T; never a range of <= 0
    }
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (shift || choose) philox4x32_10(cl, ch, (unsigned)b, 0u, k0, k1, w);
    const int bias = shift ? (int)__umulhi(w[0], (unsigned)(T - size + 1)) : 0;
    int d = 0;
    if (choose) {
        if (T > W) d = (int)__umulhi(w[1], (unsigned)(T - W + 1));
        else if (T < W) d = -(int)__umulhi(w[1], (unsigned)(W - T + 1));
    } else if (T > W) {
        d = (T - W) / 2;
    }
    a.plan[3 * b + 0] = d - bias + begin;
    a.plan[3 * b + 1] = max(0, bias - d);
    a.plan[3 * b + 2] = min(W, bias + size - d);
    a.draws[2 * b + 0] = bias;
    a.draws[2 * b + 1] = d;
    if (!move) return;
    for (int i = 0; i < a.num_node; ++i) {
        philox4x32_10(cl, ch, (unsigned)b, 1u + (unsigned)i, k0, k1, w);
        const int ia = (int)__umulhi(w[0], (unsigned)a.nA), is = (int)__umulhi(w[1], (unsigned)a.nS);
        const int ix = (int)__umulhi(w[2], (unsigned)a.nT), iy = (int)__umulhi(w[3], (unsigned)a.nT);
        const long long o = ((long long)b * a.num_node + i) * 4;
        a.move_idx[o + 0] = ia; a.move_idx[o + 1] = is; a.move_idx[o + 2] = ix; a.move_idx[o + 3] = iy;
        if (a.keys) { a.keys[o + 0] = a.angle[ia]; a.keys[o + 1] = a.scale[is]; a.keys[o + 2] = a.trans[ix]; a.keys[o + 3] = a.trans[iy]; }
    }
}

// the call counter moves on the device, after the draw of this call has read it (same stream): a graph that holds both
// launches draws a new batch on every replay
__global__ void clip_advance_kernel(long long* __restrict__ state) { state[1] = state[1] + 1; }

// ---- the gather -------------------------------------------------------------------------------------------------------------
struct ClipXfArgs {
    const float* raw;           // (n_clips, C, T, V, M)
    const long long* clip_ids;  // [B], taken modulo n_clips
    const int* plan;            // [B][3]
    const int* node;            // [num_node] (move only)
    const double* keys;         // [B][num_node][4] (move only)
    long long n_clips;
    int B, C, T, W, VM, num_node, tiles, G;
    float* out;                 // (B, C, W, V, M)
};

// element k of np.linspace(start, stop, n), as numpy computes it: k * ((stop - start) / (n - 1)) + start, the last element
// stop itself, n = 1 -> start.  No contraction: the product rounds before the sum, as it does on the host.
__device__ __forceinline__ double linspace_at(double start, double stop, int k, int n) {
#pragma clang fp contract(off)
    if (n == 1) return start;
    if (k == n - 1) return stop;
    const double step = (stop - start) / (double)(n - 1);
    return (double)k * step + start;
}

struct MoveRow { double cs, ss, tx, ty; };     // cos a . s, sin a . s, translations of one frame

__device__ __forceinline__ MoveRow move_row(const ClipXfArgs& a, int b, int t) {
#pragma clang fp contract(off)
    int i = 0;
    while (i < a.num_node - 2 && !(a.node[i] <= t && t < a.node[i + 1])) ++i;      // segments are disjoint and cover 0 .. W - 1
    const int n = a.node[i + 1] - a.node[i], k = t - a.node[i];
    const double* k0 = a.keys + ((long long)b * a.num_node + i) * 4;
    const double ang = linspace_at(k0[0], k0[4], k, n) * 3.141592653589793 / 180.0;  // reference tools.py:95-96: (.. * np.pi) / 180
    const double sc = linspace_at(k0[1], k0[5], k, n);
    MoveRow r;
    double sn, cn;
    sincos(ang, &sn, &cn);
    r.cs = cn * sc; r.ss = sn * sc;
    r.tx = linspace_at(k0[2], k0[6], k, n);
    r.ty = linspace_at(k0[3], k0[7], k, n);
    return r;
}

// VEC consecutive elements of one (slot, channel) row of the output: positions i .. i + VEC - 1 of its W VM floats.  `off` is the
// element offset of position 0's source in raw (it may lie before the clip when src0 < 0: only positions inside
// [ilo, ihi) are dereferenced, and the caller has clamped those to the clip's own frames).
template <int VEC>
__device__ __forceinline__ void load_span(const float* __restrict__ raw, long long off, int i, int ilo, int ihi, float* v) {
    if (i >= ilo && i + VEC <= ihi) {
        const float* p = raw + off + i;
        if (VEC == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = q[j];
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = p[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = (i + j >= ilo && i + j < ihi) ? raw[off + i + j] : 0.f;
    }
}

template <int VEC>
__device__ __forceinline__ void store_span(float* __restrict__ p, const float* v) {
    if constexpr (VEC == 4) {
        f32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p) = q;          // row length and i are multiples of 4, the output is 16-byte aligned
    } else {
        p[0] = v[0];
    }
}

// One thread per VEC output elements of a row; blockIdx.x = ((slot, group), tile of 256 VEC elements).  Without the move a group
// is a channel.  With it group 0 is the x and y planes together -- read, mapped in fp64 and written by the same thread -- and
// group g >= 1 is channel g + 1, copied.  Every frame of the window is moved, the zero frames of the plan included (the
// reference translates its padding to (t_x, t_y)).  A tile spans 256 VEC / VM + 1 frames at the most: their parameters (one
// fp64 sincos each, the kernel's only long arithmetic) are computed once, by the first lanes of wave 0, into LDS; a tile of
// more than CLIP_LDS_ROWS frames (VM < 16 with 16-byte accesses) computes them per thread instead -- the same function.
constexpr int CLIP_LDS_ROWS = 64;

template <int VEC, bool MOVE>
__global__ __launch_bounds__(256) void clip_transform_kernel(const ClipXfArgs a) {
    __shared__ MoveRow rows[MOVE ? CLIP_LDS_ROWS : 1];
    const unsigned blk = blockIdx.x;
    const int tile = (int)(blk % (unsigned)a.tiles), sg = (int)(blk / (unsigned)a.tiles);
    const int g = sg % a.G, b = sg / a.G;
    const int rowlen = a.W * a.VM;
    const int i = (tile * 256 + (int)threadIdx.x) * VEC;
    int t0 = 0;
    bool staged = false;
    if (MOVE && g == 0) {                           // g is the same for the whole workgroup: so is the barrier
        const int e0 = tile * 256 * VEC, e1 = min(e0 + 256 * VEC, rowlen) - 1;
        t0 = e0 / a.VM;
        const int nfr = e1 / a.VM - t0 + 1;
        staged = nfr <= CLIP_LDS_ROWS;
        if (staged) {
            if ((int)threadIdx.x < nfr) rows[threadIdx.x] = move_row(a, b, t0 + (int)threadIdx.x);
            __syncthreads();
        }
    }
    if (i >= rowlen) return;
    const long long clip = clip_of(a.clip_ids[b], a.n_clips);
    const long long src0 = a.plan[3 * b];
    // whatever the plan holds, a copied frame lies inside the window and inside the clip
    const long long lo = max(max((long long)a.plan[3 * b + 1], 0ll), -src0);
    const long long hi = min(min((long long)a.plan[3 * b + 2], (long long)a.W), (long long)a.T - src0);
    const int ilo = hi > lo ? (int)(lo * a.VM) : 0, ihi = hi > lo ? (int)(hi * a.VM) : 0;      // hi <= W: below 2^30
    const int c = MOVE ? (g == 0 ? 0 : g + 1) : g;
    const long long off = ((clip * a.C + c) * (long long)a.T + src0) * a.VM;
    float* o = a.out + ((long long)b * a.C + c) * rowlen + i;
    float x[VEC];
    load_span<VEC>(a.raw, off, i, ilo, ihi, x);
    if (!MOVE || g != 0) { store_span<VEC>(o, x); return; }
    float y[VEC];
    load_span<VEC>(a.raw, off + (long long)a.T * a.VM, i, ilo, ihi, y);
    int t_of = -1;
    MoveRow r;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
#pragma clang fp contract(off)
        const int t = (i + j) / a.VM;
        if (t != t_of) { r = staged ? rows[t - t0] : move_row(a, b, t); t_of = t; }
        const double xd = (double)x[j], yd = (double)y[j];
        x[j] = (float)(r.cs * xd + (-r.ss) * yd + r.tx);
        y[j] = (float)(r.ss * xd + r.cs * yd + r.ty);
    }
    store_span<VEC>(o, x);
    store_span<VEC>(o + rowlen, y);
}

// ---- crop-and-resize mode: the draws --------------------------------------------------------------------------------------------
// The pipeline CTR-GCN was published with: a share p of the clip's valid frames, cropped at the centre (one p) or at a drawn
// place (p drawn on [p0, p1)), resized linearly to W frames, then one rotation per clip.  include/tamgcn.h has the definition.
struct ClipCropArgs {
    const int* extent;          // [n_clips][2]
    const long long* clip_ids;  // [B], taken modulo n_clips
    const long long* labels;    // [n_clips] or null
    const long long* state;     // [2] = (seed, call counter)
    long long n_clips;
    int B, flags, min_crop;
    double p0, p1, theta;
    int* crop;                  // [B][2] = (start, L)
    double* drawn;              // [B][4] = (p, a_x, a_y, a_z)
    float* rot;                 // [B][9] (flag 2 only)
    long long* labels_out;      // [B] or null
};

// o = a . b, 3 x 3 row-major, every entry summed over k = 0, 1, 2 left to right
__device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* o) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
}

__global__ __launch_bounds__(64) void clip_crop_draw_kernel(const ClipCropArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const long long clip = clip_of(a.clip_ids[b], a.n_clips);
    if (a.labels_out) a.labels_out[b] = a.labels[clip];
    const unsigned long long seed = (unsigned long long)a.state[0], call = (unsigned long long)a.state[1];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), cl = (unsigned)call, ch = (unsigned)(call >> 32);
    const int begin = a.extent[2 * clip];
    const int valid = max(a.extent[2 * clip + 1] - begin, 1);          // tamgcn_clip_extent gives >= 1
    unsigned w[4];
    double p = a.p0;
    int bias, L;
    if (a.flags & 1) {
        philox4x32_10(cl, ch, (unsigned)b, 0u, k0, k1, w);
        const double u = (double)w[0] * 0x1p-32;
        p = a.p0 + u * (a.p1 - a.p0);
        L = min(max((int)floor((double)valid * p), a.min_crop), valid);
        bias = (int)__umulhi(w[1], (unsigned)(valid - L + 1));
    } else {
        bias = min((int)((1.0 - p) * (double)valid / 2.0), (valid - 1) / 2);
        L = valid - 2 * bias;
    }
    a.crop[2 * b + 0] = begin + bias;
    a.crop[2 * b + 1] = L;
    double ang[3] = {0.0, 0.0, 0.0};
    if (a.flags & 2) {
        philox4x32_10(cl, ch, (unsigned)b, 1u, k0, k1, w);
        double s[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ang[k] = a.theta * (2.0 * ((double)w[k] * 0x1p-32) - 1.0);
            sincos(ang[k], &s[k], &c[k]);
        }
        const double rx[9] = {1.0, 0.0, 0.0, 0.0, c[0], s[0], 0.0, -s[0], c[0]};
        const double ry[9] = {c[1], 0.0, -s[1], 0.0, 1.0, 0.0, s[1], 0.0, c[1]};
        const double rz[9] = {c[2], s[2], 0.0, -s[2], c[2], 0.0, 0.0, 0.0, 1.0};
        double zy[9], r[9];
        mat3_mul(rz, ry, zy);
        mat3_mul(zy, rx, r);
#pragma unroll
        for (int k = 0; k < 9; ++k) a.rot[9 * (long long)b + k] = (float)r[k];
    }
    a.drawn[4 * (long long)b + 0] = p;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.drawn[4 * (long long)b + 1 + k] = ang[k];
}

// ---- crop-and-resize mode: the gather -------------------------------------------------------------------------------------------
struct ClipRsArgs {
    const float* raw;           // (n_clips, C, T, V, M)
    const long long* clip_ids;  // [B], taken modulo n_clips
    const int* crop;            // [B][2] = (start, L)
    const float* rot;           // [B][9] or null
    long long n_clips;
    int B, C, T, W, VM, tiles, G;
    float* out;                 // (B, C, W, V, M)
};

// The two source frames of output frame t and their weights: F.interpolate(mode='bilinear', align_corners=False) on the time
// axis, in fp32 and without contraction.  o0, o1 are element offsets into a channel plane of the clip.
struct Tap { int o0, o1; float l0, l1; };

__device__ __forceinline__ Tap resize_tap(int t, int start, int L, float scale, int VM) {
    const ResizeTaps r = resize_taps(t, L, scale);       // feeder_common.h: shared with the ring's window builder
    Tap tp;
    tp.o0 = (start + r.i0) * VM; tp.o1 = (start + r.i1) * VM; tp.l0 = r.l0; tp.l1 = r.l1;
    return tp;
}

// VEC consecutive floats at p: one 16-byte access where p allows it (a source frame starts at a multiple of V M floats, which
// for NTU's 50 is 16-byte aligned on every other frame only), dword accesses otherwise
template <int VEC>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float* v) {
    if (VEC == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = q[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = p[j];
    }
}

// One thread per VEC consecutive positions of an output row of W VM floats; blockIdx.x = ((slot, group), tile of 256 VEC
// positions).  Without the rotation a group is a channel; with it there is one group, and a thread reads, blends, maps and
// writes the three channels of its positions.  Positions inside one output frame share their two source frames, so the span is
// two VEC-wide loads per channel; a span that crosses into the next frame (VM % VEC != 0) goes position by position.  start and
// L are clamped into the clip: whatever crop holds, every frame read is one of the clip's own T.
template <int VEC, bool ROT>
__global__ __launch_bounds__(256) void clip_resize_kernel(const ClipRsArgs a) {
#pragma clang fp contract(off)
    constexpr int NC = ROT ? 3 : 1;
    const unsigned blk = blockIdx.x;
    const int tile = (int)(blk % (unsigned)a.tiles), sg = (int)(blk / (unsigned)a.tiles);
    const int g = sg % a.G, b = sg / a.G;
    const int rowlen = a.W * a.VM;
    const int i = (tile * 256 + (int)threadIdx.x) * VEC;
    if (i >= rowlen) return;
    const long long clip = clip_of(a.clip_ids[b], a.n_clips);
    const int L = min(max(a.crop[2 * b + 1], 1), a.T);
    const int start = min(max(a.crop[2 * b], 0), a.T - L);
    const float scale = (float)L / (float)a.W;
    const int plane = a.T * a.VM;
    const int c0 = ROT ? 0 : g;
    const float* src = a.raw + (clip * a.C + c0) * (long long)plane;
    float* o = a.out + ((long long)b * a.C + c0) * rowlen + i;
    float y[NC][VEC];
    const int t = i / a.VM, vm = i - t * a.VM;
    if (VEC == 1 || vm + VEC <= a.VM) {
        const Tap tp = resize_tap(t, start, L, scale, a.VM);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float x0[VEC], x1[VEC];
            load_vec<VEC>(src + (long long)c * plane + tp.o0 + vm, x0);
            load_vec<VEC>(src + (long long)c * plane + tp.o1 + vm, x1);
#pragma unroll
            for (int j = 0; j < VEC; ++j) y[c][j] = tp.l0 * x0[j] + tp.l1 * x1[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int tj = (i + j) / a.VM, vj = i + j - tj * a.VM;
            const Tap tp = resize_tap(tj, start, L, scale, a.VM);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float* q = src + (long long)c * plane + vj;
                y[c][j] = tp.l0 * q[tp.o0] + tp.l1 * q[tp.o1];
            }
        }
    }
    if constexpr (ROT) {
        float r[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = a.rot[9 * (long long)b + k];
        float z[3][VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) z[c][j] = r[3 * c] * y[0][j] + r[3 * c + 1] * y[1][j] + r[3 * c + 2] * y[2][j];
#pragma unroll
        for (int c = 0; c < 3; ++c) store_span<VEC>(o + (long long)c * rowlen, z[c]);
    } else {
        store_span<VEC>(o, y[0]);
    }
}

}  // namespace

extern "C" int tamgcn_clip_extent(const float* raw, long long n_clips, int C, int T, int V, int M, int* extent, void* stream) {
    TG_CHECK(raw && extent, "tamgcn_clip_extent: null pointer");
    TG_CHECK(n_clips > 0 && n_clips < (1LL << 31) && C > 0 && T > 0 && V > 0 && M > 0, "tamgcn_clip_extent: bad dims n_clips=%lld C=%d T=%d V=%d M=%d",
             n_clips, C, T, V, M);
    TG_CHECK((long long)T * V * M <= (1LL << 30), "tamgcn_clip_extent: a channel plane of T V M = %lld elements is too large", (long long)T * V * M);
    const bool vec = ((long long)T * V * M) % 4 == 0 && (reinterpret_cast<uintptr_t>(raw) & 15) == 0;
    if (vec) hipLaunchKernelGGL(clip_extent_kernel<4>, dim3((unsigned)n_clips), dim3(256), 0, (hipStream_t)stream, raw, C, T, V * M, extent);
    else hipLaunchKernelGGL(clip_extent_kernel<1>, dim3((unsigned)n_clips), dim3(256), 0, (hipStream_t)stream, raw, C, T, V * M, extent);
    tamgcn_note_kernel(vec ? "clip_extent_kernel<4>" : "clip_extent_kernel<1>");
    TG_LAUNCH_CHECK("tamgcn_clip_extent");
    return 0;
}

extern "C" int tamgcn_clip_draw(const int* extent, long long n_clips, const long long* clip_ids, int B, const long long* labels, long long* state,
                                int flags, int T, int W, int num_node, int nA, int nS, int nT, const double* angle, const double* scale,
                                const double* trans, int* plan, int* draws, int* move_idx, double* keys, long long* labels_out, void* stream) {
    TG_CHECK(extent && clip_ids && state && plan && draws, "tamgcn_clip_draw: null pointer");
    TG_CHECK(B > 0 && n_clips > 0 && T > 0 && W > 0, "tamgcn_clip_draw: bad dims B=%d n_clips=%lld T=%d W=%d", B, n_clips, T, W);
    TG_CHECK(T <= (1 << 30) && W <= (1 << 30), "tamgcn_clip_draw: T=%d or W=%d above 2^30", T, W);
    TG_CHECK(flags >= 0 && flags <= 7, "tamgcn_clip_draw: flags %d (1 shift | 2 choose | 4 move)", flags);
    TG_CHECK((labels == nullptr) == (labels_out == nullptr), "tamgcn_clip_draw: labels and labels_out go together");
    if (flags & 4) {
        TG_CHECK(move_idx, "tamgcn_clip_draw: the move needs move_idx");
        TG_CHECK(num_node >= 2 && num_node <= CLIP_MAX_NODE, "tamgcn_clip_draw: num_node %d outside 2..%d", num_node, CLIP_MAX_NODE);
        TG_CHECK(nA > 0 && nS > 0 && nT > 0, "tamgcn_clip_draw: empty candidate list (nA=%d nS=%d nT=%d)", nA, nS, nT);
        TG_CHECK(!keys || (angle && scale && trans), "tamgcn_clip_draw: keys need the three candidate tables");
    }
    ClipDrawArgs a;
    a.extent = extent; a.clip_ids = clip_ids; a.labels = labels; a.state = state; a.angle = angle; a.scale = scale; a.trans = trans;
    a.n_clips = n_clips; a.B = B; a.T = T; a.W = W; a.num_node = num_node; a.nA = nA; a.nS = nS; a.nT = nT; a.flags = flags;
    a.plan = plan; a.draws = draws; a.move_idx = move_idx; a.keys = keys; a.labels_out = labels_out;
    hipLaunchKernelGGL(clip_draw_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("clip_draw_kernel");
    TG_LAUNCH_CHECK("tamgcn_clip_draw");
    if (flags) {                                        // no random flag: nothing of the stream is consumed
        hipLaunchKernelGGL(clip_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
        TG_LAUNCH_CHECK("tamgcn_clip_draw (advance)");
    }
    return 0;
}

extern "C" int tamgcn_clip_transform(const float* raw, long long n_clips, const long long* clip_ids, const int* plan, const int* node,
                                     const double* keys, int num_node, int B, int C, int T, int W, int V, int M, float* out, void* stream) {
    TG_CHECK(raw && clip_ids && plan && out, "tamgcn_clip_transform: null pointer");
    TG_CHECK(B > 0 && n_clips > 0 && C > 0 && T > 0 && W > 0 && V > 0 && M > 0, "tamgcn_clip_transform: bad dims B=%d n_clips=%lld C=%d T=%d W=%d V=%d M=%d",
             B, n_clips, C, T, W, V, M);
    TG_CHECK((long long)T * V * M <= (1LL << 30) && (long long)W * V * M <= (1LL << 30), "tamgcn_clip_transform: a channel plane above 2^30 elements (T=%d W=%d V=%d M=%d)",
             T, W, V, M);
    TG_CHECK((node == nullptr) == (keys == nullptr), "tamgcn_clip_transform: node and keys go together");
    const bool move = keys != nullptr;
    if (move) {
        TG_CHECK(C >= 2, "tamgcn_clip_transform: the move maps channels 0 and 1, C=%d", C);
        TG_CHECK(num_node >= 2 && num_node <= CLIP_MAX_NODE, "tamgcn_clip_transform: num_node %d outside 2..%d", num_node, CLIP_MAX_NODE);
    }
    const int rowlen = W * V * M;
    const bool vec = rowlen % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    ClipXfArgs a;
    a.raw = raw; a.clip_ids = clip_ids; a.plan = plan; a.node = node; a.keys = keys; a.n_clips = n_clips;
    a.B = B; a.C = C; a.T = T; a.W = W; a.VM = V * M; a.num_node = num_node; a.out = out;
    a.tiles = ceil_div(rowlen, 256 * (vec ? 4 : 1));
    a.G = move ? C - 1 : C;
    const long long blocks = (long long)B * a.G * a.tiles;
    TG_CHECK(blocks < (1LL << 31), "tamgcn_clip_transform: %lld workgroups", blocks);
    const dim3 grid((unsigned)blocks), block(256);
    if (vec && move) hipLaunchKernelGGL((clip_transform_kernel<4, true>), grid, block, 0, (hipStream_t)stream, a);
    else if (vec) hipLaunchKernelGGL((clip_transform_kernel<4, false>), grid, block, 0, (hipStream_t)stream, a);
    else if (move) hipLaunchKernelGGL((clip_transform_kernel<1, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((clip_transform_kernel<1, false>), grid, block, 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("clip_transform_kernel<%d, %s>", vec ? 4 : 1, move ? "move" : "copy");
    TG_LAUNCH_CHECK("tamgcn_clip_transform");
    return 0;
}

extern "C" int tamgcn_clip_crop_draw(const int* extent, long long n_clips, const long long* clip_ids, int B, const long long* labels,
                                     long long* state, int flags, double p0, double p1, int min_crop, double theta, int* crop,
                                     double* drawn, float* rot, long long* labels_out, void* stream) {
    TG_CHECK(extent && clip_ids && state && crop && drawn, "tamgcn_clip_crop_draw: null pointer");
    TG_CHECK(B > 0 && n_clips > 0, "tamgcn_clip_crop_draw: bad dims B=%d n_clips=%lld", B, n_clips);
    TG_CHECK(flags >= 0 && flags <= 3, "tamgcn_clip_crop_draw: flags %d (1 random crop | 2 rotation)", flags);
    TG_CHECK(p0 > 0.0 && p0 <= p1 && p1 <= 1.0, "tamgcn_clip_crop_draw: p0=%g p1=%g outside 0 < p0 <= p1 <= 1", p0, p1);   // NaN fails too
    TG_CHECK(min_crop >= 1, "tamgcn_clip_crop_draw: min_crop %d below 1", min_crop);
    TG_CHECK(theta >= 0.0 && theta <= 1.79e308, "tamgcn_clip_crop_draw: theta=%g must be finite and >= 0", theta);
    TG_CHECK(!(flags & 2) || rot, "tamgcn_clip_crop_draw: the rotation needs rot");
    TG_CHECK((labels == nullptr) == (labels_out == nullptr), "tamgcn_clip_crop_draw: labels and labels_out go together");
    ClipCropArgs a;
    a.extent = extent; a.clip_ids = clip_ids; a.labels = labels; a.state = state; a.n_clips = n_clips; a.B = B; a.flags = flags;
    a.min_crop = min_crop; a.p0 = p0; a.p1 = p1; a.theta = theta; a.crop = crop; a.drawn = drawn; a.rot = rot; a.labels_out = labels_out;
    hipLaunchKernelGGL(clip_crop_draw_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("clip_crop_draw_kernel");
    TG_LAUNCH_CHECK("tamgcn_clip_crop_draw");
    if (flags) {                                        // nothing random: nothing of the stream is consumed
        hipLaunchKernelGGL(clip_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
        TG_LAUNCH_CHECK("tamgcn_clip_crop_draw (advance)");
    }
    return 0;
}

extern "C" int tamgcn_clip_resize(const float* raw, long long n_clips, const long long* clip_ids, const int* crop, const float* rot, int B,
                                  int C, int T, int W, int V, int M, float* out, void* stream) {
    TG_CHECK(raw && clip_ids && crop && out, "tamgcn_clip_resize: null pointer");
    TG_CHECK(B > 0 && n_clips > 0 && C > 0 && T > 0 && W > 0 && V > 0 && M > 0, "tamgcn_clip_resize: bad dims B=%d n_clips=%lld C=%d T=%d W=%d V=%d M=%d",
             B, n_clips, C, T, W, V, M);
    TG_CHECK((long long)T * V * M <= (1LL << 30) && (long long)W * V * M <= (1LL << 30), "tamgcn_clip_resize: a channel plane above 2^30 elements (T=%d W=%d V=%d M=%d)",
             T, W, V, M);
    TG_CHECK(!rot || C == 3, "tamgcn_clip_resize: the rotation maps three channels, C=%d", C);
    const int rowlen = W * V * M;
    const bool vec = rowlen % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    ClipRsArgs a;
    a.raw = raw; a.clip_ids = clip_ids; a.crop = crop; a.rot = rot; a.n_clips = n_clips;
    a.B = B; a.C = C; a.T = T; a.W = W; a.VM = V * M; a.out = out;
    a.tiles = ceil_div(rowlen, 256 * (vec ? 4 : 1));
    a.G = rot ? 1 : C;
    const long long blocks = (long long)B * a.G * a.tiles;
    TG_CHECK(blocks < (1LL << 31), "tamgcn_clip_resize: %lld workgroups", blocks);
    const dim3 grid((unsigned)blocks), block(256);
    if (vec && rot) hipLaunchKernelGGL((clip_resize_kernel<4, true>), grid, block, 0, (hipStream_t)stream, a);
    else if (vec) hipLaunchKernelGGL((clip_resize_kernel<4, false>), grid, block, 0, (hipStream_t)stream, a);
    else if (rot) hipLaunchKernelGGL((clip_resize_kernel<1, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((clip_resize_kernel<1, false>), grid, block, 0, (hipStream_t)stream, a);
    tamgcn_note_kernel("clip_resize_kernel<%d, %s>", vec ? 4 : 1, rot ? "rot" : "plain");
    TG_LAUNCH_CHECK("tamgcn_clip_resize");
    return 0;
}
