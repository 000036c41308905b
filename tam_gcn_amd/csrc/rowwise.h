// What the row-streaming kernels share (elementwise.hip: the CTR-GCN / ST-GCN epilogues; dropout.hip: the block tail with a
// device-drawn mask): the row geometry of a launch, the row sums, the ReLU sign bits and the float4 view of a fused prologue.
// Everything has internal linkage; the lane rule itself (row_geo) stays in elementwise.hip, other sources ask tamgcn_row_tpr.
#pragma once
#include "common.h"

// lanes per row of a row-wise launch over (N, C, L) (elementwise.hip, row_geo)
int tamgcn_row_tpr(int N, int C, int L, int vec_capable);

namespace {

constexpr int EW_THREADS = 256;

// row geometry of a launch: lanes per row (power of two, 16..256) -> rows per workgroup.  Round 4: long rows get the WHOLE workgroup
// (the four waves walk one row together: 5.0-5.6 against 4.8-5.4 TB/s at HBM-streaming sizes, tools/probes/ew_layout_probe.hip;
// in the product the N-UCLA rows of 320 steps gained nothing); their row sums then meet in LDS.
struct RowGeo { int tpr, rows; };               // rows = N * C
__device__ __forceinline__ bool row_coords(const RowGeo& g, int C, int& c, int& n, int& li) {
    const int rpb = EW_THREADS / g.tpr;
    const int row = blockIdx.x * rpb + threadIdx.x / g.tpr;
    li = threadIdx.x & (g.tpr - 1);
    const bool ok = row < g.rows;
    const int r = ok ? row : 0;                    // idle lanes shadow row 0 (loads only) and take part in the shuffles
    n = r / C; c = r - n * C;
    return ok;
}
// sum over the lanes of a row (every thread of the workgroup calls it; fixed order: lanes by xor-shuffle, then the row's waves in turn)
__device__ __forceinline__ float row_sum(float v, const RowGeo& g) {
    const int w = g.tpr < 64 ? g.tpr : 64;
    for (int o = 1; o < w; o <<= 1) v += __shfl_xor(v, o);
    if (g.tpr > 64) {                               // wave-uniform (kernel argument): the row spans tpr / 64 waves
        __shared__ float red[EW_THREADS / 64];
        const int wave = threadIdx.x >> 6, wpr = g.tpr >> 6, first = wave & ~(wpr - 1);
        __syncthreads();                            // a previous call's reads of red
        if ((threadIdx.x & 63) == 0) red[wave] = v;
        __syncthreads();
        float t = red[first];
        for (int k = 1; k < wpr; ++k) t += red[first + k];
        v = t;
    }
    return v;
}
__device__ __forceinline__ void row_store_sums(const float* vals, int nst, float* part, int C, int N, int c, int n,
                                               const RowGeo& g, int li, bool ok) {
    for (int s = 0; s < nst; ++s) {
        const float v = row_sum(vals[s], g);
        if (li == 0 && ok) part[((long long)s * C + c) * N + n] = v;
    }
}

// ---- ReLU sign bits --------------------------------------------------------
// One bit per element, set iff the stored activation is > 0.f (the test its backward applies; -0.0, +0.0 and NaN give 0), so
// that the backward reads 1/16 of a tensor pass instead of the activation.  Layout: every (n, c) row of L floats has
// sign_row_bytes(L) = ceil(L / 4) bytes; byte i holds elements 4i .. 4i+3 in bits 0 .. 3 -- the byte of the float4 a lane
// holds anyway.  The last byte of a row with L % 4 != 0 is assembled from the scalar tail's lanes (sign_tail_store).
__device__ __forceinline__ unsigned sign4(const float4& v) {
    return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
}
// the scalar tail: lanes 0 .. (L % 4) - 1 of the row hold one element each (tb = their bit, shifted to its place; 0 elsewhere).
// Every thread of the workgroup calls it; lanes 0 .. 3 of a row are neighbours in one wave (tpr >= 16).
__device__ __forceinline__ void sign_tail_store(unsigned tb, unsigned char* brow, int L, int li) {
    tb |= __shfl_xor(tb, 1);
    tb |= __shfl_xor(tb, 2);
    if (li == 0 && (L & 3)) brow[L >> 2] = (unsigned char)tb;
}
__device__ __forceinline__ float4 sign_mask4(float4 d, unsigned q) {
    if (!(q & 1u)) d.x = 0.f;
    if (!(q & 2u)) d.y = 0.f;
    if (!(q & 4u)) d.z = 0.f;
    if (!(q & 8u)) d.w = 0.f;
    return d;
}

// float4 view of the fused prologue for one channel row (coefficients are per channel)
struct RowSrc {
    const float* x1; const float* x2; float c1, c2, c0; int act;
};
__device__ __forceinline__ RowSrc row_src(const SrcDev& s, long long base, int ch) {
    RowSrc r;
    r.x1 = s.x1 + base; r.x2 = s.x2 ? s.x2 + base : nullptr;
    r.c1 = s.coef ? s.coef[ch] : 1.f;
    r.c2 = (s.coef && s.x2) ? s.coef[s.ctot + ch] : 0.f;
    r.c0 = s.coef ? s.coef[2 * s.ctot + ch] : 0.f;
    r.act = s.act;
    return r;
}
__device__ __forceinline__ float row_val(const RowSrc& r, int i) {
    float v = fmaf(r.c1, r.x1[i], fmaf(r.c2, r.x2 ? r.x2[i] : 0.f, r.c0));
    return r.act == 1 ? fmaxf(v, 0.f) : v;
}
__device__ __forceinline__ float4 row_val4(const RowSrc& r, int i4) {
    float4 a = reinterpret_cast<const float4*>(r.x1)[i4];
    float4 b = r.x2 ? reinterpret_cast<const float4*>(r.x2)[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o;
    o.x = fmaf(r.c1, a.x, fmaf(r.c2, b.x, r.c0)); o.y = fmaf(r.c1, a.y, fmaf(r.c2, b.y, r.c0));
    o.z = fmaf(r.c1, a.z, fmaf(r.c2, b.z, r.c0)); o.w = fmaf(r.c1, a.w, fmaf(r.c2, b.w, r.c0));
    if (r.act == 1) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    return o;
}
// Every row-wise kernel below walks a row as L / 4 groups of four floats plus a scalar tail of L % 4 elements.  Rows are 16-byte
// aligned only if L % 4 == 0; gfx950 takes dword-aligned 16-byte accesses at full rate (tools/probes/unaligned_probe.hip), and the
// scalar loops NTU's T = 150 / 75 layers (L = 3750 / 1875) used to take ran at under half the streaming rate.

}  // namespace
