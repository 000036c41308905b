// Partial-slab reductions.  The kernels that contract over samples and frames (weight gradients, the CTRGC bias / dA / dw4 /
// dalpha gradients) write one partial slab per split instead of using atomics; these kernels sum the slabs: fp64
// accumulation in a fixed order, so the result does not depend on scheduling.
#include "common.h"

namespace {

// out[e] = sum_s part[s][e]: 64 consecutive e per block (coalesced), the split axis spread over
// the 4 waves of the block, fp64 accumulation, fixed order => deterministic.
__global__ __launch_bounds__(256) void reduce_sum_kernel(const float* part, int nsplit, long long stride_s, long long count,
                                                         float scale, int accumulate, float* out) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * 64 + lane;
    double s = 0.0;
    if (e < count)
        for (int k = w; k < nsplit; k += 4) s += (double)part[k * stride_s + e];
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && e < count) {
        double t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        float r = (float)(t * (double)scale);
        out[e] = accumulate ? out[e] + r : r;
    }
}

}  // namespace

// first stage for many splits: group g (64 splits) is summed in place into its first slab.  Only
// the block owning (64 elements, group g) touches those slabs for those elements: race-free.
__global__ __launch_bounds__(256) void reduce_group_kernel(float* part, int nsplit, long long stride_s, long long count) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * 64 + lane;
    const int s0 = blockIdx.y * 64, s1 = min(nsplit, s0 + 64);
    double s = 0.0;
    if (e < count)
        for (int k = s0 + w; k < s1; k += 4) s += (double)part[k * stride_s + e];
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && e < count)
        part[(long long)s0 * stride_s + e] = (float)((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
}

// Many slab reductions in one launch: blockIdx.y = descriptor, blockIdx.x = 64-element group (the longest descriptor
// sets the grid, the others leave early).  A layer's backward produces ~25 partial-slab sets; reducing each with its own
// one or two 6-us launches was 1.4 ms of a 31 ms step.  Same arithmetic as reduce_sum_kernel: fp64, fixed order.
constexpr int RM_MAX = 24;
struct ReduceMulti { int n; tamgcn_reduce_desc d[RM_MAX]; };

__global__ __launch_bounds__(256) void reduce_multi_kernel(const ReduceMulti md) {
    __shared__ double red[4][64];
    const tamgcn_reduce_desc& d = md.d[blockIdx.y];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * 64 + lane;
    if ((long long)blockIdx.x * 64 >= d.count) return;          // whole workgroup: uniform
    double s = 0.0;
    if (e < d.count) {
        const float* p = d.part + e;
        int k = w;
        for (; k + 28 < d.nsplit; k += 32) {                      // eight independent loads in flight, summed as two groups of four
            float a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = p[(long long)(k + 4 * i) * d.stride_s];
            s += ((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3]);
            s += ((double)a[4] + (double)a[5]) + ((double)a[6] + (double)a[7]);
        }
        for (; k + 12 < d.nsplit; k += 16) {                      // four independent loads in flight
            float a0 = p[(long long)k * d.stride_s], a1 = p[(long long)(k + 4) * d.stride_s];
            float a2 = p[(long long)(k + 8) * d.stride_s], a3 = p[(long long)(k + 12) * d.stride_s];
            s += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
        }
        for (; k < d.nsplit; k += 4) s += (double)p[(long long)k * d.stride_s];
    }
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && e < d.count) {
        double t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        float r = (float)(t * (double)d.scale);
        d.out[e] = d.accumulate ? d.out[e] + r : r;
    }
}

extern "C" int tamgcn_reduce_multi(const tamgcn_reduce_desc* descs, int n, void* stream) {
    TG_CHECK(descs && n > 0, "tamgcn_reduce_multi: bad args");
    for (int i0 = 0; i0 < n; i0 += RM_MAX) {
        ReduceMulti md;
        md.n = n - i0 < RM_MAX ? n - i0 : RM_MAX;
        long long maxc = 0;
        for (int i = 0; i < md.n; ++i) {
            md.d[i] = descs[i0 + i];
            TG_CHECK(md.d[i].part && md.d[i].out && md.d[i].nsplit > 0 && md.d[i].count > 0, "tamgcn_reduce_multi: bad descriptor %d", i0 + i);
            if (md.d[i].count > maxc) maxc = md.d[i].count;
        }
        hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)((maxc + 63) / 64), md.n), dim3(256), 0, (hipStream_t)stream, md);
    }
    tamgcn_note_kernel("reduce_multi_kernel");
    TG_LAUNCH_CHECK("tamgcn_reduce_multi");
    return 0;
}

extern "C" int tamgcn_reduce_sum(float* part, int nsplit, long long stride_s, long long count,
                                 float scale, int accumulate, float* out, void* stream) {
    TG_CHECK(part && out && nsplit > 0 && count > 0, "tamgcn_reduce_sum: bad args");
    long long blocks = (count + 63) / 64;
    if (nsplit > 128) {                                 // two stages (clobbers `part`, which is scratch)
        int groups = (nsplit + 63) / 64;
        TG_CHECK(groups <= 65535, "tamgcn_reduce_sum: too many splits");
        hipLaunchKernelGGL(reduce_group_kernel, dim3((unsigned)blocks, groups), dim3(256), 0, (hipStream_t)stream,
                           part, nsplit, stride_s, count);
        nsplit = groups;
        stride_s *= 64;
    }
    hipLaunchKernelGGL(reduce_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       part, nsplit, stride_s, count, scale, accumulate, out);
    tamgcn_note_kernel("reduce_sum_kernel");
    TG_LAUNCH_CHECK("tamgcn_reduce_sum");
    return 0;
}
