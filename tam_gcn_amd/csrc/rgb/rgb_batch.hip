// tamgcn_rgb_draw and tamgcn_rgb_batch: one batch of the RGB modality from the resized uint8 store.
#include "rgb_common.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct RgbBatchArgs {
    const unsigned char* store;     // (n, S, S, 3)
    const long long* ids;           // [B], taken modulo n
    const float* lut;               // (3, 256)
    const int* flip;                // [B] or null
    const unsigned char* missing;   // [n] or null
    const float* row_scale;         // (B, S) or null
    const long long* labels;        // [n] or null
    long long* labels_out;          // [B] or null
    float* out;                     // (B, 3 F, S, S)
    long long n;
    int S, B, F, missing_mode;
};

// ---- the flips of one batch: one thread per slot --------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rgb_draw_kernel(const long long* __restrict__ state, int B, int* __restrict__ flip) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const unsigned long long seed = (unsigned long long)state[0], call = (unsigned long long)state[1];
    unsigned w[4];
    philox4x32_10((unsigned)call, (unsigned)(call >> 32), (unsigned)b, 0u, (unsigned)seed, (unsigned)(seed >> 32), w);
    flip[b] = w[0] < 0x80000000u ? 1 : 0;
}

// the call counter moves on the device, after the draw of this call has read it (same stream): the convention of
// clip_advance_kernel (../clipfeeder.hip)
__global__ void rgb_advance_kernel(long long* __restrict__ state) { state[1] = state[1] + 1; }

// the table in LDS: 768 floats, three per thread of a 256-thread workgroup
__device__ __forceinline__ void load_lut(float (*s_lut)[256], const float* __restrict__ lut) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s_lut[c][threadIdx.x] = lut[c * 256 + threadIdx.x];
    __syncthreads();
}

// ---- S % 4 == 0: a thread makes x = 4 q .. 4 q + 3 of row y of slot b, all three channels ------------------------------------
__global__ __launch_bounds__(256) void rgb_batch_vec_kernel(const RgbBatchArgs a) {
    __shared__ float s_lut[3][256];
    load_lut(s_lut, a.lut);
    const int Q = a.S >> 2;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)a.B * a.S * Q) return;
    const int q = (int)(t % Q);
    const long long r = t / Q;
    const int y = (int)(r % a.S), b = (int)(r / a.S);
    const long long id = clip_of(a.ids[b], a.n);
    if (a.labels_out && y == 0 && q == 0) a.labels_out[b] = a.labels[id];
    const bool gone = a.missing && a.missing[id] != 0;
    const bool fl = a.flip && a.flip[b] != 0;
    unsigned d[3] = {0u, 0u, 0u};                                               // a black image
    if (!gone) {
        const unsigned* __restrict__ p =
            reinterpret_cast<const unsigned*>(a.store + ((id * a.S + y) * a.S + 4 * (fl ? Q - 1 - q : q)) * 3);
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
    }
    // byte 3 i + c of the 12 is channel c of pixel i: pixel 0 = d0[0..2], 1 = d0[3] d1[0..1], 2 = d1[2..3] d2[0], 3 = d2[1..3]
    const unsigned px[4] = {d[0] & 0xFFFFFFu, (d[0] >> 24) | ((d[1] & 0xFFFFu) << 8), (d[1] >> 16) | ((d[2] & 0xFFu) << 16), d[2] >> 8};
    f32x4_t v[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned s = fl ? px[3 - i] : px[i];                              // the mirrored quad, reversed
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][i] = s_lut[c][(s >> (8 * c)) & 0xFFu];
    }
    if (a.row_scale) {
        const float w = a.row_scale[(long long)b * a.S + y];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] * w;
    }
    if (gone && a.missing_mode == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const long long plane = (long long)a.S * a.S;
    float* __restrict__ o = a.out + (long long)b * 3 * a.F * plane + (long long)y * a.S + 4 * q;
    for (int f = 0; f < a.F; ++f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4_t*>(o + (long long)(3 * f + c) * plane) = v[c];
    }
}

// ---- any S: a thread makes one x of row y of slot b, all three channels ------------------------------------------------------
__global__ __launch_bounds__(256) void rgb_batch_scalar_kernel(const RgbBatchArgs a) {
    __shared__ float s_lut[3][256];
    load_lut(s_lut, a.lut);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)a.B * a.S * a.S) return;
    const int x = (int)(t % a.S);
    const long long r = t / a.S;
    const int y = (int)(r % a.S), b = (int)(r / a.S);
    const long long id = clip_of(a.ids[b], a.n);
    if (a.labels_out && y == 0 && x == 0) a.labels_out[b] = a.labels[id];
    const bool gone = a.missing && a.missing[id] != 0;
    const bool fl = a.flip && a.flip[b] != 0;
    float v[3];
    const unsigned char* __restrict__ p = a.store + ((id * a.S + y) * a.S + (fl ? a.S - 1 - x : x)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = s_lut[c][gone ? 0u : (unsigned)p[c]];
    if (a.row_scale) {
        const float w = a.row_scale[(long long)b * a.S + y];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] * w;
    }
    if (gone && a.missing_mode == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = 0.f;
    }
    const long long plane = (long long)a.S * a.S;
    float* __restrict__ o = a.out + (long long)b * 3 * a.F * plane + (long long)y * a.S + x;
    for (int f = 0; f < a.F; ++f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(long long)(3 * f + c) * plane] = v[c];
    }
}

}  // namespace

extern "C" int tamgcn_rgb_draw(long long* state, int B, int* flip, void* stream) {
    RGB_CHECK(state && flip, "tamgcn_rgb_draw: state or flip is NULL");
    RGB_CHECK(rgb_al(state, 8) && rgb_al(flip, 4), "tamgcn_rgb_draw: state or flip is not aligned to its element");
    RGB_CHECK(B >= 1, "tamgcn_rgb_draw: B = %d", B);
    hipLaunchKernelGGL(rgb_draw_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, state, B, flip);
    RGB_LAUNCH_CHECK("tamgcn_rgb_draw");
    hipLaunchKernelGGL(rgb_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    RGB_LAUNCH_CHECK("tamgcn_rgb_draw (advance)");
    return 0;
}

extern "C" int tamgcn_rgb_batch(const unsigned char* store, long long n, int S, const long long* ids, int B, const float* lut, const int* flip,
                                const unsigned char* missing, int missing_mode, const float* row_scale, int F, const long long* labels,
                                long long* labels_out, float* out, void* stream) {
    RGB_CHECK(store && ids && lut && out, "tamgcn_rgb_batch: store, ids, lut or out is NULL");
    RGB_CHECK(n >= 1 && S >= 1 && B >= 1 && F >= 1, "tamgcn_rgb_batch: bad dims n = %lld, S = %d, B = %d, F = %d", n, S, B, F);
    RGB_CHECK((long long)B * S * S < (1LL << 31), "tamgcn_rgb_batch: B S S = %lld reaches 2^31: split the batch", (long long)B * S * S);
    RGB_CHECK(missing_mode == 0 || missing_mode == 1, "tamgcn_rgb_batch: missing_mode = %d (0 zeros | 1 black)", missing_mode);
    RGB_CHECK((labels == nullptr) == (labels_out == nullptr), "tamgcn_rgb_batch: labels and labels_out go together");
    RGB_CHECK(rgb_al(ids, 8) && rgb_al(lut, 4) && rgb_al(out, 4) && rgb_al(flip, 4) && rgb_al(row_scale, 4) && rgb_al(labels, 8) &&
                  rgb_al(labels_out, 8),
              "tamgcn_rgb_batch: a pointer is not aligned to its element");
    RgbBatchArgs a;
    a.store = store; a.ids = ids; a.lut = lut; a.flip = flip; a.missing = missing; a.row_scale = row_scale; a.labels = labels;
    a.labels_out = labels_out; a.out = out; a.n = n; a.S = S; a.B = B; a.F = F; a.missing_mode = missing_mode;
    const bool vec = S % 4 == 0 && rgb_al(store, 4) && rgb_al(out, 16);
    if (vec) {
        const long long threads = (long long)B * S * (S / 4);
        hipLaunchKernelGGL(rgb_batch_vec_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    } else {
        const long long threads = (long long)B * S * S;
        hipLaunchKernelGGL(rgb_batch_scalar_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    }
    RGB_LAUNCH_CHECK("tamgcn_rgb_batch");
    return 0;
}
