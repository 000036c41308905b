// Shared host/device helpers of libtamgcn_xmodal.so (gfx950 / CDNA4 only): error text and check macros of its own, and the
// exact-fp32 MFMA tile step every GEMM of the head is built from.  ../common.h is included for its device helpers only
// (mfma16, wave_sum16, tg_launch_lds); nothing here defines a symbol of libtamgcn.so.
#pragma once
#include "../common.h"
#include "../../../include/tamgcn_xmodal.h"

void tamgcn_xm_set_error(const char* fmt, ...);

#define XM_CHECK(cond, ...)                         \
    do {                                            \
        if (!(cond)) {                              \
            tamgcn_xm_set_error(__VA_ARGS__);       \
            return -1;                              \
        }                                           \
    } while (0)

#define XM_LAUNCH_CHECK(name)                                                            \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) {                                                          \
            tamgcn_xm_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));   \
            return -2;                                                                   \
        }                                                                                \
    } while (0)

constexpr int XM_MAX_N = 1024;      // clips per call: the pre-activations of 16 hidden units for all of them are 64 KB of LDS

static inline bool xm_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static inline bool xm_al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

// N in 1..XM_MAX_N and every listed width a positive multiple of 4
#define XM_CHECK_N(fn, N) XM_CHECK((N) >= 1 && (N) <= XM_MAX_N, fn ": N = %d outside 1..%d", (N), XM_MAX_N)
#define XM_CHECK_W(fn, name, v) XM_CHECK((v) >= 4 && (v) % 4 == 0, fn ": " name " = %d is not a positive multiple of 4", (v))
#define XM_CHECK_P16(fn, name, p) XM_CHECK((p) != nullptr && xm_al16(p), fn ": " name " is NULL or not 16-byte aligned")

// ---------------------------------------------------------------------------
// One step of a 16 x 16 output tile on v_mfma_f32_16x16x4_f32 covers 16 contraction indices: lane (i = lane & 15, q = lane >> 4)
// holds indices k .. k + 3 with k = kb + 4 q of row i of A and of column i of B, and MFMA j takes element j of both (which four
// indices an MFMA sums is free as long as A and B agree).  An operand whose contraction index is contiguous in memory is one
// 16-byte load per lane and step; one whose contraction index is the leading dimension is four dword loads, 16 lanes wide.
// D[row = 4 q + reg][col = i].  Indices >= K contribute zeros; the caller clamps r / c into the matrix and drops those results.
// ---------------------------------------------------------------------------
__device__ __forceinline__ f32x4 xm_frag_rowk(const float* __restrict__ base, int ld, int r, int k, int K) {   // ld, K % 4 == 0
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k < K) v = *reinterpret_cast<const f32x4*>(base + (size_t)r * ld + k);
    return v;
}
__device__ __forceinline__ f32x4 xm_frag_colk(const float* __restrict__ base, int ld, int c, int k, int K) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = k + j < K ? base[(size_t)(k + j) * ld + c] : 0.f;
    return v;
}
__device__ __forceinline__ f32x4 xm_mma16(const f32x4& a, const f32x4& b, f32x4 acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = mfma16(a[j], b[j], acc);
    return acc;
}

// out (M, Nc) = A (M, K) . B for a thin A (M <= 1024 rows, K % 4 == 0, rows of A 16-byte aligned).  A workgroup owns 16 columns
// and up to 64 rows; its four waves take every fourth step of K and wave t sums the four partial tiles of row tile t in wave
// order through LDS, so the result does not depend on timing.  B is read once per 64 rows.
//   BT   B is (Nc, K): out = A B^T, B streamed with 16-byte loads;  else B is (K, Nc)
//   SIG  out = 1 / (1 + expf(-(acc + bias[col])))
template <bool BT, bool SIG>
__global__ __launch_bounds__(256) void xm_gemm_ksplit(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ bias,
                                                       int M, int Nc, int K, float* __restrict__ out) {
    __shared__ f32x4 part[4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int c0 = blockIdx.x * 16, cc = min(c0 + i, Nc - 1);
    const int rt0 = blockIdx.y * 4, nrt = min(4, (M + 15) / 16 - rt0);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = wave * 16; kb < K; kb += 64) {
        const int k = kb + 4 * q;
        const f32x4 b = BT ? xm_frag_rowk(B, K, cc, k, K) : xm_frag_colk(B, Nc, cc, k, K);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nrt) {
                const int r = min((rt0 + t) * 16 + i, M - 1);
                acc[t] = xm_mma16(xm_frag_rowk(A, K, r, k, K), b, acc[t]);
            }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) part[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave < nrt) {
        const f32x4 s = ((part[0][wave][lane] + part[1][wave][lane]) + part[2][wave][lane]) + part[3][wave][lane];
        const int col = c0 + i;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = (rt0 + wave) * 16 + 4 * q + reg;
            if (row < M && col < Nc) {
                float v = s[reg];
                if (SIG) {
                    v += bias[col];
                    v = 1.f / (1.f + expf(-v));
                }
                out[(size_t)row * Nc + col] = v;
            }
        }
    }
}
