// Device helpers shared by the token-choice kernels (sample.hip, beam.hip): the order-preserving integer image of a float and the
// Philox4x32-10 + Gumbel draw that egomi_sample_rows / egomi_beam_rows add to scores (oracle/sampling.py restates it on the host).
#pragma once
#include <math.h>

__device__ __forceinline__ unsigned f2key(float v) {
    unsigned u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);           // order-preserving: a < b  <=>  key(a) < key(b)
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float gumbel_from_bits(unsigned r) {
    const float u = ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f);          // (0, 1) strictly
    return -logf(-logf(u));
}
