// The three streaming kernels of CTRGC, once: the bodies behind ctrgc_tiled.hip's ctrgc_agg_fwd / ctrgc_agg_bwd /
// ctrgc_de_acc_mfma kernels (the joint count a template argument: 20, 25, 32, 64) and vgen.hip's vgen_agg_fwd / vgen_agg_bwd /
// vgen_de_acc kernels (the joint count a kernel argument, 2..32).  tests/test_gpu_vgen_routes.py holds the two families to the
// same bits at V = 20, 25 and 32.
//
// How the text is shared.  This header has the constants, the LDS formulas and the two geometry policies.  The bodies are
// FRAGMENTS -- ctrgc_stream_agg_fwd.h, ctrgc_stream_agg_bwd.h, ctrgc_stream_de_acc.h and the prologue they share,
// ctrgc_stream_prologue4.h -- that each __global__ function pastes into itself with #include, after `using G = <policy>;
// const G g...;`, with its own arguments and the joint count V (a template argument there, a kernel argument here) in scope.
// Pasted, not called: as __forceinline__ function templates the same text gave other device code than the kernels it replaced
// (other registers in 6 of the 24 templated kernels; the parent's own text moved into such a function gave exactly that code,
// so it was the function form, not the policy).  Pasted, all 24 templated kernels are instruction for instruction what they were
// (profiles/ctrgc_stream_merge_resources.txt).
//
//   stream_agg_fwd   y[n,c,t,u]     = sum_s sum_v x3_s[n,c,t,v] E_s[n,c,u,v]   + moment partials   E_c stationary in LDS,
//   stream_agg_bwd   dx3_s[n,c,t,v] = sum_u dy[n,c,t,u] E_s[n,c,u,v]           + db3 partials      (transposed for bwd)
//   stream_de_acc    dE_s[n,c,u,v]  = sum_t dy[n,c,t,u] x3_s[n,c,t,v]
//
// Common to all: workgroup = (n, c), 256 threads; the streamed operand in chunks of STREAM_BT = 32 frames, the next chunk's
// 16-byte pieces fetched into registers under the MFMAs (v_mfma_f32_16x16x4_f32) of this one; V joints in HBM, VP = V rounded
// up to a multiple of 16 in LDS, the pads zero, so the contraction over joints runs (V + 3) / 4 steps and nothing of a pad
// reaches global memory.  Rows of V floats need no alignment (16-byte accesses from dword-aligned addresses run at full rate on
// gfx950, tools/probes/unaligned_probe.hip); a chunk's last piece may reach <= 12 bytes past it, into the next (n, c) row or
// into the slack the ops' allocator keeps behind every tensor: every float past the chunk's valid run is replaced by zero
// before it reaches LDS (cut4, ctrgc_stream_prologue4.h).  dy comes with its producer's prologue act(c1 x1 + c2 x2 + c0).
//
// LDS images.  A-type operands (rows = MFMA row index i, contraction along the row) use pitch PE = VP + 2 (16 rows x 2 k hit
// 32 distinct banks with ds_read_b32); B-type operands of [k][j] form (the dE accumulation) use pitch VP + 16 == 16 (mod 32).
//
// Waves.  Aggregation: a chunk is 2 frame tiles x NUT joint tiles; wave -> (frame tile wave >> 1, joint tiles of half
// wave & 1).  dE accumulation: NUT x NUT output tiles per subset; wave -> (u tile, NUT / (4 / UW) v tiles), every subset.
// NUT = 1 (VP = 16, the run-time policy only): a chunk is two output tiles, so waves 0 and 1 carry the aggregation's MFMAs
// (all four still stream the operands, and these kernels are HBM-bound); in the dE accumulation wave s owns subset s.
//
// The GEOMETRY POLICY G owns what differs between the two families and nothing else (TlGeo<V> / VgGeo<VP>):
//
//   constexpr in both   VP PE NUT, VMAX (bound of V: sizes the prefetch registers), AL (V % 4 == 0 known: rows of the dE
//                       accumulation's images take aligned 16-byte stores), PADS (the images have pad columns to zero), FULL
//                       (VP == V known: the store guards fold away), FILL_WITH_E (stage_E zeroes the chunk image with E's in
//                       one run and one barrier; else the kernel zeroes it under PADS and stage_E only E's)
//   divV(f, r, c)       flat index -> (row, column) of a [rows][V] run: a constant division / tg_rcp_div
//   k4()                contraction steps over the joints: a constant (the loop unrolls) / (V + 3) / 4
//   subset_of(e, CH4)   e / CH4 / two compares
//   scatter4(...)       four consecutive floats -> LDS image: float2 pairs when V % 4 == 0 is known, else element-wise with
//                       constant divisions / a wrapping element-wise scatter
//   stage_E<ST, TR>()   E_c of every subset -> LDS: one flat register-staged run (16-byte loads when AL) / one subset at a time
// and three members that keep, for each family, the form its kernels were compiled with (either form under the other policy
// costs it registers or instructions, see the resources file):
//   idle0(e, n)         the prefetch index of a lane past the chunk's n pieces (it fetches nothing): clamped to 0, so that the
//                       constant divisions see a small dividend / left as it is
//   in_clip(f, valid, t0, T)
//                       does the piece at float f of the chunk at t0 start inside the clip: t0 + f / V < T / f < valid, the
//                       chunk's floats inside the clip -- the same predicate for pieces of the chunk
//   cut4(t, f, valid)   a piece that starts inside the clip may run past its end: those floats belong to the next row (or the
//                       slack) and must not enter a sum: zero from flat index `valid` on.  One test of the whole piece around
//                       three selects / four selects (under the run-time policy the first form compiles to a branch per piece)
// What the run-time policy pays for its members is in profiles/vgen_bench.txt and DESIGN.md section 3b-2.
#pragma once
#include "common.h"

namespace {

constexpr int STREAM_BT = 32;            // frames per chunk

// dynamic LDS of the aggregation kernels ([ST][VP][PE] E + [ST or 1][BT][PE] chunk) and of the dE accumulation ([ST + 1][BT][VP + 16])
constexpr size_t stream_agg_lds(int VP, int ST, bool bwd) { return sizeof(float) * (size_t)((ST * VP + (bwd ? 1 : ST) * STREAM_BT) * (VP + 2)); }
constexpr size_t stream_de_lds(int VP, int ST) { return sizeof(float) * (size_t)((ST + 1) * STREAM_BT * (VP + 16)); }

// ---------------------------------------------------------------------------------------------------------------
// the joint count a template argument
// ---------------------------------------------------------------------------------------------------------------
template <int V_> struct TlGeo {
    static constexpr int V = V_, VMAX = V;
    static constexpr int VP = (V + 15) & ~15;          // joints in LDS
    static constexpr int PE = VP + 2;                  // A-type pitch
    static constexpr int K4 = (V + 3) / 4;             // contraction steps over joints (pads are zero)
    static constexpr int NUT = VP / 16;                // 16-wide joint tiles
    static constexpr bool AL = (V % 4) == 0, PADS = VP != V, FULL = VP == V, FILL_WITH_E = false;
    static_assert(NUT % 2 == 0 && (STREAM_BT * V) % 4 == 0, "tile geometry");

    __device__ __forceinline__ static void divV(int f, int& r, int& c) { r = f / V; c = f - r * V; }
    __device__ __forceinline__ static constexpr int k4() { return K4; }
    __device__ __forceinline__ static int subset_of(int e, int CH4) { return e / CH4; }
    __device__ __forceinline__ static int idle0(int e, int n) { return e < n ? e : 0; }
    __device__ __forceinline__ static bool in_clip(int f, int, int t0, int T) { return t0 + f / V < T; }
    __device__ __forceinline__ static void cut4(float4& t, int f, int valid) {
        if (f + 3 >= valid) { if (f + 0 >= valid) t.x = 0.f; if (f + 1 >= valid) t.y = 0.f; if (f + 2 >= valid) t.z = 0.f; t.w = 0.f; }
    }

    // float4 of a contiguous [rows][V] run starting at flat index f -> LDS image with row pitch P (rows of V real + zero pads)
    __device__ __forceinline__ static void scatter4(float* img, int P, int f, const float4& t) {
        if constexpr (AL) {
            const int r = f / V, c = f - r * V;
            float2* d = reinterpret_cast<float2*>(img + r * P + c);
            d[0] = make_float2(t.x, t.y);
            d[1] = make_float2(t.z, t.w);
        } else {
            const float vals[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int r = (f + k) / V, c = (f + k) - r * V; img[r * P + c] = vals[k]; }
        }
    }

    // E_c of every subset -> LDS, rows u (TRANSPOSE = false: Es[s][u][v]) or rows v (true: Es[s][v][u]), pitch VP + 2, pads zero;
    // FILL_WITH_E: the chunk image behind it (nchunk floats at Es + ST * VP * PE) is zeroed in the same run; else the kernel has done it
    template <int ST, bool TRANSPOSE>
    __device__ __forceinline__ static void stage_E(const float* __restrict__ Eg, int Cout, int n, int c, float* Es, int) {
        constexpr int VV = V * V;
        if constexpr (PADS) {
            for (int e = threadIdx.x; e < ST * VP * PE; e += 256) Es[e] = 0.f;
            __syncthreads();
        }
        if constexpr (AL) {
            constexpr int NV4 = ST * VV / 4, NL = (NV4 + 255) / 256;
            float4 t[NL];
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int e = threadIdx.x + i * 256, ec = e < NV4 ? e : 0, s = ec / (VV / 4), r = ec - s * (VV / 4);
                t[i] = reinterpret_cast<const float4*>(Eg + (((long long)n * ST + s) * Cout + c) * VV)[r];
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int e = threadIdx.x + i * 256, s = e / (VV / 4), r = e - s * (VV / 4);
                if (e < NV4) {
                    const int u = (r * 4) / V, v = (r * 4) - u * V;
                    if constexpr (!TRANSPOSE) {
                        float2* d = reinterpret_cast<float2*>(Es + (s * VP + u) * PE + v);
                        d[0] = make_float2(t[i].x, t[i].y);
                        d[1] = make_float2(t[i].z, t[i].w);
                    } else {
                        float* d = Es + (s * VP + v) * PE + u;
                        d[0] = t[i].x; d[PE] = t[i].y; d[2 * PE] = t[i].z; d[3 * PE] = t[i].w;
                    }
                }
            }
        } else {
            constexpr int NE = ST * VV, NL = (NE + 255) / 256;
            float t[NL];
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int e = threadIdx.x + i * 256, ec = e < NE ? e : 0, s = ec / VV, r = ec - s * VV;
                t[i] = Eg[(((long long)n * ST + s) * Cout + c) * VV + r];
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int e = threadIdx.x + i * 256, s = e / VV, r = e - s * VV;
                if (e < NE) {
                    const int u = r / V, v = r - u * V;
                    Es[TRANSPOSE ? (s * VP + v) * PE + u : (s * VP + u) * PE + v] = t[i];
                }
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------
// the joint count a kernel argument; what is a template argument is only what sizes a register array
// ---------------------------------------------------------------------------------------------------------------
template <int VP_> struct VgGeo {
    static constexpr int VP = VP_, VMAX = VP;
    static constexpr int PE = VP + 2;                  // A-type pitch (16 rows x 2 k hit 32 distinct banks)
    static constexpr int NUT = VP / 16;                // 16-wide joint tiles
    static constexpr bool AL = false, PADS = true, FULL = false, FILL_WITH_E = true;
    static_assert(VP == 16 || VP == 32, "VP is 16 or 32");
    const int V;
    const float rcpV;
    __device__ __forceinline__ explicit VgGeo(int v) : V(v), rcpV(1.f / (float)v) {}

    __device__ __forceinline__ void divV(int f, int& r, int& c) const { r = tg_rcp_div(f, rcpV); c = f - r * V; }
    __device__ __forceinline__ int k4() const { return (V + 3) / 4; }
    __device__ __forceinline__ static int subset_of(int e, int CH4) { return (e >= CH4) + (e >= 2 * CH4); }
    __device__ __forceinline__ static int idle0(int e, int) { return e; }
    __device__ __forceinline__ static bool in_clip(int f, int valid, int, int) { return f < valid; }
    __device__ __forceinline__ static void cut4(float4& t, int f, int valid) {
        if (f + 0 >= valid) t.x = 0.f;
        if (f + 1 >= valid) t.y = 0.f;
        if (f + 2 >= valid) t.z = 0.f;
        if (f + 3 >= valid) t.w = 0.f;
    }

    // four consecutive floats of a contiguous [rows][V] run starting at flat index f -> LDS image with row pitch P
    __device__ __forceinline__ void scatter4(float* img, int P, int f, const float4& t) const {
        const float vals[4] = {t.x, t.y, t.z, t.w};
        int r, c;
        divV(f, r, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            img[r * P + c] = vals[k];
            if (++c == V) { c = 0; ++r; }
        }
    }

    // E_c of every subset -> LDS, rows u (TRANSPOSE = false: Es[s][u][v]) or rows v (true: Es[s][v][u]), pitch VP + 2, pads zero;
    // FILL_WITH_E: the chunk image behind it (nchunk floats at Es + ST * VP * PE) is zeroed in the same run; else the kernel has done it
    template <int ST, bool TRANSPOSE>
    __device__ __forceinline__ void stage_E(const float* __restrict__ Eg, int Cout, int n, int c, float* Es, int nchunk) const {
        constexpr int NL = VP * VP / 256;
        const int VV = V * V;
        for (int e = threadIdx.x; e < ST * VP * PE + nchunk; e += 256) Es[e] = 0.f;     // both images in one run
        __syncthreads();
#pragma unroll
        for (int s = 0; s < ST; ++s) {
            const float* g = Eg + (((long long)n * ST + s) * Cout + c) * VV;
            float t[NL];
#pragma unroll
            for (int i = 0; i < NL; ++i) { const int e = threadIdx.x + i * 256; t[i] = g[e < VV ? e : 0]; }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int e = threadIdx.x + i * 256;
                if (e < VV) {
                    int u, v;
                    divV(e, u, v);
                    Es[TRANSPOSE ? (s * VP + v) * PE + u : (s * VP + u) * PE + v] = t[i];
                }
            }
        }
    }
};

}  // namespace
