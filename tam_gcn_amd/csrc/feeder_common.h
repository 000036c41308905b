// What the two device-side feeders (feeder.hip: ragged N-UCLA clips; clipfeeder.hip: fixed-shape (N, C, T, V, M) arrays)
// share: the clip a batch slot reads and the counter-based generator of their draw streams.  And what they share with the
// window builders of streaming.hip, which read their frames from a ring instead of a clip: the N-UCLA transform's one body
// (feeder_transform_body) and the time-resize's taps (resize_taps).
#pragma once
#include "common.h"

// Python's i % n for n > 0 (the sign of the divisor): what Feeder.batch() does with the indices it is given
__device__ __forceinline__ long long clip_of(long long i, long long n) {
    const long long r = i % n;
    return r < 0 ? r + n : r;
}

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four 32-bit words.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* w) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// ---- the N-UCLA transform (reference feeder/feeder_nucla_gcn.py:85-130) ---------------------------------------------
__device__ __forceinline__ void rot_point(const double* p, const double* c, const double* R, double* o) {
    const double x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
    // numpy's row-vector-times-matrix order: o_j = x R[0][j] + y R[1][j] + z R[2][j], left to right
    o[0] = x * R[0] + y * R[3] + z * R[6];
    o[1] = x * R[1] + y * R[4] + z * R[7];
    o[2] = x * R[2] + y * R[5] + z * R[8];
}

// np.linspace(0, L - 1, TS).astype(int)[t], reference :116 (the val path's source frame of output frame t)
__device__ __forceinline__ int val_frame(int t, long long L, int TS) {
    const double step = (double)(L - 1) / (double)(TS > 1 ? TS - 1 : 1);
    return (t == TS - 1 && TS > 1) ? (int)(L - 1) : (int)((double)t * step);
}

// One workgroup of 256 threads per clip of L frames.  Pass 1: per-coordinate min / max over every (frame, joint) of the
// transformed clip; pass 2: the TS x V output positions (gathered frames), normalised to [-1, 1] and written as the requested
// stream into out, the slot's (3, TS, V).  point(e) is the address of the three coordinates of position e = frame * V + joint
// of the clip -- consecutive in a clip of feeder.hip, slot by slot in a ring of streaming.hip -- and src_frame(t) the clip's
// frame that output frame t shows; R the row-major view matrix (points are row vectors: p' = p . R).
template <class Point, class SrcFrame>
__device__ __forceinline__ void feeder_transform_body(Point point, SrcFrame src_frame, long long L, int V, int TS, int mode, int center_joint,
                                                      const double* R, const int* __restrict__ parent, float* __restrict__ out) {
    __shared__ double smin[3][256 / 64], smax[3][256 / 64];
    __shared__ double lo[3], hi[3];
    const int tid = threadIdx.x;
    const double* c0 = point(center_joint);                                                                               // frame 0
    const double cen[3] = {c0[0], c0[1], c0[2]};
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (long long e = tid; e < L * V; e += 256) {
        double o[3];
        rot_point(point(e), cen, R, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = fmin(mn[k], o[k]); mx[k] = fmax(mx[k], o[k]); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 1; off < 64; off <<= 1) {
            mn[k] = fmin(mn[k], __shfl_xor(mn[k], off));
            mx[k] = fmax(mx[k], __shfl_xor(mx[k], off));
        }
        if ((tid & 63) == 0) { smin[k][tid >> 6] = mn[k]; smax[k][tid >> 6] = mx[k]; }
    }
    __syncthreads();
    if (tid < 3) {
        double l = smin[tid][0], h = smax[tid][0];
        for (int w = 1; w < 4; ++w) { l = fmin(l, smin[tid][w]); h = fmax(h, smax[tid][w]); }
        lo[tid] = l; hi[tid] = h;
    }
    __syncthreads();
    auto joint = [&](int t, int v, double* o) {        // normalised joint coordinates of output frame t
        const long long fr = src_frame(t);
        double p[3];
        rot_point(point(fr * V + v), cen, R, p);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (p[k] - lo[k]) / (hi[k] - lo[k] + 1e-6) * 2 - 1;
    };
    auto bone = [&](int t, int v, double* o) {
        double c[3], p[3];
        joint(t, v, c); joint(t, parent[v], p);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = c[k] - p[k];
    };
    for (int e = tid; e < TS * V; e += 256) {
        const int t = e / V, v = e - t * V;
        double o[3] = {0., 0., 0.};
        if (mode == 0) joint(t, v, o);
        else if (mode == 1) bone(t, v, o);
        else if (t < TS - 1) {
            double c[3], nx[3];
            if (mode == 2) { joint(t, v, c); joint(t + 1, v, nx); }
            else { bone(t, v, c); bone(t + 1, v, nx); }
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = nx[k] - c[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) out[((long long)k * TS + t) * V + v] = (float)o[k];
    }
}

// ---- the linear time-resize (clipfeeder.hip's crop-and-resize mode) ---------------------------------------------------
// The two source frames i0, i1 of the crop's L that output frame t of W blends, and their weights: F.interpolate(mode='bilinear',
// align_corners=False) on the time axis, in fp32 and without contraction; scale = (float)L / (float)W.  The blend is
// l0 * x[i0] + l1 * x[i1], again without contraction.
struct ResizeTaps { int i0, i1; float l0, l1; };

__device__ __forceinline__ ResizeTaps resize_taps(int t, int L, float scale) {
#pragma clang fp contract(off)
    const float src = fmaxf(scale * ((float)t + 0.5f) - 0.5f, 0.f);
    ResizeTaps r;
    r.i0 = min((int)src, L - 1); r.i1 = min(r.i0 + 1, L - 1);
    r.l1 = src - (float)r.i0; r.l0 = 1.f - r.l1;
    return r;
}
