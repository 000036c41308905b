// Dropout inside the residual tail of an st_gcn block (reference models/stgcn.py:77-99) and of the model heads: the mask is a
// counter-based draw made, applied and remembered in the tail's single pass (include/tamgcn.h, tamgcn_drop_add_act_fwd).
// Row mapping, sign bits and row sums are the ones of elementwise.hip (rowwise.h); Philox4x32-10 is the feeders' (feeder_common.h).
#include "common.h"
#include "rowwise.h"
#include "feeder_common.h"

namespace {

// out = act(keep * a * scale + res) in add_act_fwd_kernel's single pass and row mapping.  The mask is a counter-based draw
// (include/tamgcn.h, tamgcn_drop_add_act_fwd): one Philox4x32-10 call per group of four floats, word e decides element
// 4g + e, kept iff word >= thr.  A byte of `bits` holds the sign bits of `out` in its low nibble (as sign4 writes them;
// zero without the ReLU) and the keep bits in its high nibble, so the backward draws nothing.
__device__ __forceinline__ unsigned keep4(const unsigned* w, unsigned thr) {
    return (w[0] >= thr ? 1u : 0u) | (w[1] >= thr ? 2u : 0u) | (w[2] >= thr ? 4u : 0u) | (w[3] >= thr ? 8u : 0u);
}
__global__ __launch_bounds__(EW_THREADS) void drop_add_act_fwd_kernel(RowGeo geo, SrcDev a, SrcDev res, int has_res, int relu, int C, int L,
                                                                      const long long* __restrict__ state, unsigned site, unsigned thr,
                                                                      float scale, float* out, unsigned char* bits) {
#pragma clang fp contract(off)             // a * scale is rounded before the residual is added
    int c, n, li;
    const bool rowok = row_coords(geo, C, c, n, li);
    if (!rowok) L = 0;                     // idle lanes only take part in the shuffles
    const RowSrc ra = row_src(a, ((long long)n * a.ctot + a.coff + c) * L, a.coff + c);
    RowSrc rr = ra;
    if (has_res) rr = row_src(res, ((long long)n * res.ctot + res.coff + c) * L, res.coff + c);
    const unsigned row = (unsigned)(n * C + c);
    float* op = out + (long long)row * L;
    unsigned char* brow = bits ? bits + (long long)row * ((L + 3) >> 2) : nullptr;
    const unsigned long long seed = (unsigned long long)state[0], call = (unsigned long long)state[1];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), cl = (unsigned)call, ch = (unsigned)(call >> 32);
    const unsigned sbase = site << 20;
    unsigned tb = 0;
    {                                      // groups of four floats (rows need only be 4-byte aligned: V = 25), then the row's tail
        for (int i = li; i < (L >> 2); i += geo.tpr) {
            unsigned w[4];
            philox4x32_10(cl, ch, row, sbase | (unsigned)i, k0, k1, w);
            const unsigned k = keep4(w, thr);
            float4 v = row_val4(ra, i);
            v.x = (k & 1u) ? v.x * scale : 0.f; v.y = (k & 2u) ? v.y * scale : 0.f;
            v.z = (k & 4u) ? v.z * scale : 0.f; v.w = (k & 8u) ? v.w * scale : 0.f;
            if (has_res) { float4 r = row_val4(rr, i); v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            reinterpret_cast<float4*>(op)[i] = v;
            if (brow) brow[i] = (unsigned char)((relu ? sign4(v) : 0u) | (k << 4));
        }
    }
    {
        for (int i = (L & ~3) + li; i < L; i += geo.tpr) {      // lanes 0 .. (L % 4) - 1: the same group, one word each
            unsigned w[4];
            philox4x32_10(cl, ch, row, sbase | (unsigned)(i >> 2), k0, k1, w);
            const bool keep = w[i & 3] >= thr;
            float v = keep ? row_val(ra, i) * scale : 0.f;
            if (has_res) v += row_val(rr, i);
            v = relu ? fmaxf(v, 0.f) : v;
            op[i] = v;
            if (relu && v > 0.f) tb |= 1u << (i & 3);
            if (keep) tb |= 16u << (i & 3);
        }
    }
    if (bits) sign_tail_store(tb, brow, L, li);     // uniform over the launch: every lane of the wave reaches the shuffles
}

// d = dout under the sign nibble; dza = d * scale under the keep nibble (into bn2); dzr = d (into the residual branch).
// part as add_act_bwd: [0..1] = (sum dza, sum dza (a_pre - mu_a)), [2..3] = (sum d, sum d (r_pre - mu_r)) if r_pre is given.
__global__ __launch_bounds__(EW_THREADS) void drop_add_act_bwd_kernel(RowGeo geo, const float* dout, const unsigned char* bits, int relu, float scale,
                                                                      const float* a_pre, const float* a_save, const float* r_pre,
                                                                      const float* r_save, int C, int L, int N, float* dza, float* dzr, float* part) {
#pragma clang fp contract(off)             // dza = fl32(d * scale) also where it enters the sums
    int c, n, li;
    const bool rowok = row_coords(geo, C, c, n, li);
    if (!rowok) L = 0;                     // idle lanes only take part in the shuffles
    const long long b = ((long long)n * C + c) * L;
    const unsigned char* brow = bits + ((long long)n * C + c) * ((L + 3) >> 2);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    const float mua = a_pre ? a_save[c] : 0.f, mur = r_pre ? r_save[c] : 0.f;
    {                                      // groups of four floats (rows need only be 4-byte aligned: V = 25), then the row's tail
        for (int i = li; i < (L >> 2); i += geo.tpr) {
            float4 d = reinterpret_cast<const float4*>(dout + b)[i];
            const unsigned q = brow[i];
            if (relu) d = sign_mask4(d, q);
            const float4 za = sign_mask4(make_float4(d.x * scale, d.y * scale, d.z * scale, d.w * scale), q >> 4);
            reinterpret_cast<float4*>(dza + b)[i] = za;
            if (dzr) reinterpret_cast<float4*>(dzr + b)[i] = d;
            s[0] += (za.x + za.y) + (za.z + za.w);
            if (a_pre) {
                float4 p = reinterpret_cast<const float4*>(a_pre + b)[i];
                s[1] = fmaf(za.x, p.x - mua, fmaf(za.y, p.y - mua, fmaf(za.z, p.z - mua, fmaf(za.w, p.w - mua, s[1]))));
            }
            if (r_pre) {
                float4 p = reinterpret_cast<const float4*>(r_pre + b)[i];
                s[2] += (d.x + d.y) + (d.z + d.w);
                s[3] = fmaf(d.x, p.x - mur, fmaf(d.y, p.y - mur, fmaf(d.z, p.z - mur, fmaf(d.w, p.w - mur, s[3]))));
            }
        }
    }
    {
        for (int i = (L & ~3) + li; i < L; i += geo.tpr) {
            float d = dout[b + i];
            const unsigned q = brow[i >> 2] >> (i & 3);
            if (relu && !(q & 1u)) d = 0.f;
            const float za = (q & 16u) ? d * scale : 0.f;
            dza[b + i] = za;
            if (dzr) dzr[b + i] = d;
            s[0] += za;
            if (a_pre) s[1] = fmaf(za, a_pre[b + i] - mua, s[1]);
            if (r_pre) { s[2] += d; s[3] = fmaf(d, r_pre[b + i] - mur, s[3]); }
        }
    }
    if (part) row_store_sums(s, r_pre ? 4 : 2, part, C, N, c, n, geo, li, rowok);      // uniform over the launch
}

// the call counter moves on the device, after the forward of this call has read it (same stream): a graph that holds the
// forward and this launch draws a new mask on every replay
__global__ void dropout_advance_kernel(long long* __restrict__ state) { state[1] = state[1] + 1; }

bool grid_ok(int N, int C) { return N > 0 && C > 0 && (long long)N * C < (1LL << 31); }
RowGeo drop_geo(int N, int C, int L) { RowGeo g; g.tpr = tamgcn_row_tpr(N, C, L, 1); g.rows = N * C; return g; }
dim3 row_grid(const RowGeo& g) { return dim3((unsigned)ceil_div(g.rows, EW_THREADS / g.tpr)); }

}  // namespace

// L <= 2^22 and site < 4096: the group index and the site id share one 32-bit counter word (site << 20 | g, g < L / 4 <= 2^20)
extern "C" int tamgcn_drop_add_act_fwd(const tamgcn_src* a, const tamgcn_src* res, int relu, int N, int C, int T, int V,
                                       const long long* state, int site, unsigned thr, float scale, float* out, unsigned char* bits, void* stream) {
    TG_CHECK(a && a->x1 && out && state && grid_ok(N, C) && T > 0 && V > 0, "tamgcn_drop_add_act_fwd: bad args");
    TG_CHECK((long long)T * V <= (1LL << 22), "tamgcn_drop_add_act_fwd: rows of more than 2^22 elements are not served (T * V = %lld)", (long long)T * V);
    TG_CHECK(site >= 0 && site < 4096, "tamgcn_drop_add_act_fwd: site %d outside 0 .. 4095", site);
    TG_CHECK(scale >= 1.f && scale <= 3.4e38f, "tamgcn_drop_add_act_fwd: scale %g is not 1 / (1 - p) of a p in (0, 1)", (double)scale);
    const RowGeo geo = drop_geo(N, C, T * V);
    hipLaunchKernelGGL(drop_add_act_fwd_kernel, row_grid(geo), dim3(EW_THREADS), 0, (hipStream_t)stream,
                       geo, make_src(*a), res ? make_src(*res) : null_src(), res ? 1 : 0, relu ? 1 : 0, C, T * V, state, (unsigned)site, thr, scale, out, bits);
    tamgcn_note_kernel("drop_add_act_fwd_kernel");
    TG_LAUNCH_CHECK("tamgcn_drop_add_act_fwd");
    return 0;
}

extern "C" int tamgcn_drop_add_act_bwd(const float* dout, const unsigned char* bits, int relu, float scale, const float* a_pre, const float* a_save,
                                       const float* r_pre, const float* r_save, int N, int C, int T, int V, float* dza, float* dzr, float* part,
                                       void* stream) {
    TG_CHECK(dout && bits && dza && grid_ok(N, C) && T > 0 && V > 0 && (!a_pre || a_save) && (!r_pre || (r_save && dzr)) &&
             (part || (!a_pre && !r_pre)) && (!part || a_pre), "tamgcn_drop_add_act_bwd: bad args");
    TG_CHECK((long long)T * V <= (1LL << 22), "tamgcn_drop_add_act_bwd: rows of more than 2^22 elements are not served (T * V = %lld)", (long long)T * V);
    TG_CHECK(scale >= 1.f && scale <= 3.4e38f, "tamgcn_drop_add_act_bwd: scale %g is not 1 / (1 - p) of a p in (0, 1)", (double)scale);
    const RowGeo geo = drop_geo(N, C, T * V);
    hipLaunchKernelGGL(drop_add_act_bwd_kernel, row_grid(geo), dim3(EW_THREADS), 0, (hipStream_t)stream,
                       geo, dout, bits, relu ? 1 : 0, scale, a_pre, a_save, r_pre, r_save, C, T * V, N, dza, dzr, part);
    tamgcn_note_kernel("drop_add_act_bwd_kernel");
    TG_LAUNCH_CHECK("tamgcn_drop_add_act_bwd");
    return 0;
}

extern "C" int tamgcn_dropout_advance(long long* state, void* stream) {
    TG_CHECK(state, "tamgcn_dropout_advance: no state");
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    tamgcn_note_kernel("dropout_advance_kernel");
    TG_LAUNCH_CHECK("tamgcn_dropout_advance");
    return 0;
}
