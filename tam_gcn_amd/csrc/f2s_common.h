// The f2s family's shared constants and operand helpers (f2s.hip: the eval-mode st_gcn block forward; f2s_bwd.hip: its data
// gradient).  Moved here unchanged from f2s.hip.
#pragma once
#include "common.h"

namespace {

constexpr int FS_NT = 256;                 // four waves
constexpr int FS_CT = 16;                  // output channels per workgroup
constexpr int FS_NP = 4;                   // 16-column pieces of a tile
constexpr int FS_MAXCOLS = 16 * FS_NP;     // columns (frames x joints) of a tile
constexpr int FS_MAXTF = 8;                // frames per tile at most
constexpr int FS_YP = 92;                  // floats per (k, channel) row of y in LDS: max tf*VP = 84 (V = 9), + 8: rows 4 banks apart mod 32
constexpr int FS_AP = 48;                  // floats per row of Ae in LDS: 32 columns; 16 * odd keeps kq = 0, 1 on distinct banks
constexpr int FS_RP = FS_MAXCOLS + 4;      // floats per channel row of the tcn's reduction tile
constexpr int FS_KT = 9;

static inline int fs_tf(int V) {
    int tf = FS_MAXCOLS / V;
    return tf < 1 ? 1 : (tf > FS_MAXTF ? FS_MAXTF : tf);
}

// all-ones where ok, else zero, opaque to the compiler: a plain `ok ? v : 0` on a loaded value is turned into a branch around
// the load, with a full wait behind it, and a chunk's loads then complete one after the other instead of together
__device__ __forceinline__ float fs_keep(float v, bool ok) {
    unsigned m = ok ? 0xffffffffu : 0u;
    asm("" : "+v"(m));
    return __uint_as_float(__float_as_uint(v) & m);
}

// four weights w[base .. base + 3] of a row of `len` floats: one 16-byte load where the caller vouches for the alignment
// (vec: len % 4 == 0 and a 16-byte aligned array), else four loads; indices >= len read element 0 instead and give zero
__device__ __forceinline__ f32x4 fs_load_a(const float* __restrict__ row, int base, int len, bool vec) {
    f32x4 a;
    if (vec) {
        a = *reinterpret_cast<const f32x4*>(row + (base < len ? base : 0));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = row[base + j < len ? base + j : 0];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = fs_keep(a[j], base + j < len);
    return a;
}

// p[ok ? i : 0], zero where !ok: the load itself is unconditional (element 0 of the array is always there)
__device__ __forceinline__ float fs_load_b(const float* __restrict__ p, long long i, bool ok) {
    return fs_keep(p[ok ? i : 0], ok);
}

static inline bool fs_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int fs_geometry_ok(int V, int K, int Cin, int Cout, int KT, int stride) {
    return V >= 2 && V <= 32 && K >= 1 && K <= 3 && Cin >= 1 && Cin <= 256 && Cout >= 16 && Cout <= 256 && Cout % 16 == 0 && KT == FS_KT &&
           (stride == 1 || stride == 2);
}

}  // namespace
