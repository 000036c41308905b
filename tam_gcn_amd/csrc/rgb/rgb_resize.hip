// tamgcn_rgb_resize: PIL's 8-bit bilinear resample, one axis per launch.  Runs once per split, at load.
#include "rgb_common.h"

namespace {

// in (outer, n_in, inner) -> out (outer, n_out, inner) along the middle axis; one thread per output byte, consecutive threads
// on consecutive bytes.  The horizontal pass is (n H0, W0, 3), the vertical one (n, H0, 3 Wo).
__global__ __launch_bounds__(256) void rgb_resample_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                           const int* __restrict__ coef, const int* __restrict__ bounds, int K,
                                                           long long total, int n_in, int n_out, int inner) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % inner);
    const long long t = e / inner;
    const int o = (int)(t % n_out);
    const long long r = t / n_out;
    const int first = min(max(bounds[2 * o], 0), n_in);
    const int count = min(min(max(bounds[2 * o + 1], 0), K), n_in - first);
    const int* __restrict__ c = coef + (long long)o * K;
    const unsigned char* __restrict__ p = in + (r * n_in + first) * inner + i;
    int acc = 1 << 21;
    for (int j = 0; j < count; ++j) acc += c[j] * (int)p[(long long)j * inner];
    out[e] = (unsigned char)min(max(acc >> 22, 0), 255);
}

int launch_pass(const unsigned char* in, unsigned char* out, const int* coef, const int* bounds, int K, long long outer, int n_in,
                int n_out, int inner, hipStream_t stream, const char* what) {
    const long long total = outer * n_out * inner;
    hipLaunchKernelGGL(rgb_resample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, coef, bounds, K, total,
                       n_in, n_out, inner);
    RGB_LAUNCH_CHECK(what);
    return 0;
}

}  // namespace

extern "C" int tamgcn_rgb_resize(const unsigned char* src, int n, int H0, int W0, int Ho, int Wo, const int* coef_h, const int* bounds_h,
                                 int Kh, const int* coef_v, const int* bounds_v, int Kv, unsigned char* tmp, unsigned char* dst,
                                 void* stream) {
    RGB_CHECK(src && dst, "tamgcn_rgb_resize: src or dst is NULL");
    RGB_CHECK(n >= 1 && H0 >= 1 && W0 >= 1 && Ho >= 1 && Wo >= 1, "tamgcn_rgb_resize: bad dims n = %d, H0 = %d, W0 = %d, Ho = %d, Wo = %d", n,
              H0, W0, Ho, Wo);
    const long long lim = (1LL << 31) / 3;
    RGB_CHECK((long long)n * H0 * W0 < lim && (long long)n * H0 * Wo < lim && (long long)n * Ho * Wo < lim,
              "tamgcn_rgb_resize: %d images of %d x %d -> %d x %d reach 2^31 bytes in one tensor: split the call", n, H0, W0, Ho, Wo);
    RGB_CHECK((coef_h == nullptr) == (bounds_h == nullptr), "tamgcn_rgb_resize: coef_h and bounds_h go together");
    RGB_CHECK((coef_v == nullptr) == (bounds_v == nullptr), "tamgcn_rgb_resize: coef_v and bounds_v go together");
    const bool hor = coef_h != nullptr, ver = coef_v != nullptr;
    RGB_CHECK(hor || W0 == Wo, "tamgcn_rgb_resize: the horizontal pass is skipped but W0 = %d != Wo = %d", W0, Wo);
    RGB_CHECK(ver || H0 == Ho, "tamgcn_rgb_resize: the vertical pass is skipped but H0 = %d != Ho = %d", H0, Ho);
    RGB_CHECK(!hor || (Kh >= 1 && Kh <= TAMGCN_RGB_MAX_TAPS), "tamgcn_rgb_resize: Kh = %d outside 1..%d", Kh, TAMGCN_RGB_MAX_TAPS);
    RGB_CHECK(!ver || (Kv >= 1 && Kv <= TAMGCN_RGB_MAX_TAPS), "tamgcn_rgb_resize: Kv = %d outside 1..%d", Kv, TAMGCN_RGB_MAX_TAPS);
    RGB_CHECK(!(hor && ver) || tmp, "tamgcn_rgb_resize: two passes need tmp (n, H0, Wo, 3)");
    RGB_CHECK(src != dst && (!(hor && ver) || (tmp != src && tmp != dst)), "tamgcn_rgb_resize: src, tmp and dst must not overlap");
    hipStream_t s = (hipStream_t)stream;
    if (!hor && !ver) {
        const hipError_t e = hipMemcpyAsync(dst, src, (size_t)n * H0 * W0 * 3, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) {
            tamgcn_rgb_set_error("tamgcn_rgb_resize: copy failed: %s", hipGetErrorString(e));
            return -2;
        }
        return 0;
    }
    if (hor) {
        const int rc = launch_pass(src, ver ? tmp : dst, coef_h, bounds_h, Kh, (long long)n * H0, W0, Wo, 3, s, "tamgcn_rgb_resize (horizontal)");
        if (rc) return rc;
    }
    if (ver) return launch_pass(hor ? tmp : src, dst, coef_v, bounds_v, Kv, n, H0, Ho, 3 * Wo, s, "tamgcn_rgb_resize (vertical)");
    return 0;
}
