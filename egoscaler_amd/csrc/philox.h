// The random draw of the token-choice kernels (choice.h; sample.hip, beam.hip): Philox4x32-10 and the Gumbel noise that egomi_sample_rows /
// egomi_beam_rows add to the scores of one element.  oracle/sampling.py (gumbel_noise) restates gumbel_noise() on the host.
#pragma once
#include <math.h>

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
// g = -log(-log u) of element (row, c) at draw counter `ctr`: counter (c / 4, row, ctr lo, ctr hi), key (seed lo, seed hi), word c % 4
__device__ __forceinline__ float gumbel_noise(unsigned row, unsigned c, unsigned long long seed, unsigned long long ctr) {
    unsigned r[4];
    philox4x32(c >> 2, row, (unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
    return gumbel_from_bits(r[c & 3]);
}
