// What the two device-side feeders (feeder.hip: ragged N-UCLA clips; clipfeeder.hip: fixed-shape (N, C, T, V, M) arrays)
// share: the clip a batch slot reads and the counter-based generator of their draw streams.
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
