// The row pass shared by csrc/logprob.hip (egomi_token_logprob, egomi_bin_stats) and csrc/grammar.hip (egomi_traj_grammar_step): a row of V bf16 or
// fp32 logits read once by a 1024-thread workgroup through aligned 16-byte loads, its maximum and sum of exponentials, and the float64
// workgroup sum.  One copy: the three kernels take m and s from the same code, so the same row gives them the same bits.
#pragma once
#include "common.h"
#include <math.h>

#define LPB_THREADS 1024
#define LPB_NPT 32                       // values per thread held in registers (4 chunks of 8)

// The 8 elements [8c, 8c + 8) of the row at byte address `row` (naturally aligned, any 16-byte phase `mb`), through aligned 16-byte loads.
// Blocks without a byte of [row, row_end) are not read (zeros stand in); the caller drops elements >= V by index.
template <typename T> __device__ __forceinline__ void lp_load8(uintptr_t row, uintptr_t row_end, unsigned mb, int c, float (&v)[8]);
template <> __device__ __forceinline__ void lp_load8<bf16_t>(uintptr_t row, uintptr_t row_end, unsigned mb, int c, float (&v)[8]) {
    const uintptr_t a = row + (uintptr_t)c * 16 - mb;                   // 16-byte aligned; holds element 8c at byte mb
    uint32_t w[9];
    const u32x4 z = {0u, 0u, 0u, 0u};
    const u32x4 A = *reinterpret_cast<const u32x4*>(a);                 // element 8c < V lies in it
    const u32x4 B = (mb != 0 && a + 16 < row_end) ? *reinterpret_cast<const u32x4*>(a + 16) : z;
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = A[i]; w[4 + i] = B[i]; }
    w[8] = 0u;
    const unsigned bs = (mb & 3u) * 8u;                                  // 0 or 16 bits
    uint32_t o[4];
    switch (mb >> 2) {                                                   // uniform over the workgroup
        case 0: _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = __funnelshift_r(w[i], w[i + 1], bs); break;
        case 1: _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = __funnelshift_r(w[1 + i], w[2 + i], bs); break;
        case 2: _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = __funnelshift_r(w[2 + i], w[3 + i], bs); break;
        default: _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = __funnelshift_r(w[3 + i], w[4 + i], bs); break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(o[i] << 16);
        v[2 * i + 1] = __uint_as_float(o[i] & 0xFFFF0000u);
    }
}
template <> __device__ __forceinline__ void lp_load8<float>(uintptr_t row, uintptr_t row_end, unsigned mb, int c, float (&v)[8]) {
    const uintptr_t a = row + (uintptr_t)c * 32 - mb;
    uint32_t w[12];
    const u32x4 z = {0u, 0u, 0u, 0u};
    const u32x4 A = *reinterpret_cast<const u32x4*>(a);
    const u32x4 B = (a + 16 < row_end) ? *reinterpret_cast<const u32x4*>(a + 16) : z;
    const u32x4 C = (mb != 0 && a + 32 < row_end) ? *reinterpret_cast<const u32x4*>(a + 32) : z;
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = A[i]; w[4 + i] = B[i]; w[8 + i] = C[i]; }
    switch (mb >> 2) {
        case 0: _Pragma("unroll") for (int i = 0; i < 8; ++i) v[i] = __uint_as_float(w[i]); break;
        case 1: _Pragma("unroll") for (int i = 0; i < 8; ++i) v[i] = __uint_as_float(w[1 + i]); break;
        case 2: _Pragma("unroll") for (int i = 0; i < 8; ++i) v[i] = __uint_as_float(w[2 + i]); break;
        default: _Pragma("unroll") for (int i = 0; i < 8; ++i) v[i] = __uint_as_float(w[3 + i]); break;
    }
}

// The row's maximum m and s = sum exp(x - m) over its V elements, as every thread of the 1024-thread workgroup gets them (see the top comment:
// element e belongs to thread (e / 8) % 1024, aligned 16-byte loads, the row in registers for REG, accurate expf).  `red` is 16 floats of LDS.
template <typename T, bool REG>
__device__ __forceinline__ void lp_row_max_sumexp(const T* lg, int V, float* red, float& m_out, float& s_out) {
    const int tid = threadIdx.x;
    const uintptr_t row = (uintptr_t)lg, row_end = row + (uintptr_t)V * sizeof(T);
    const unsigned mb = (unsigned)(row & 15u);
    const int nchunk = (V + 7) >> 3;
    const int niter = REG ? LPB_NPT / 8 : (nchunk + LPB_THREADS - 1) / LPB_THREADS;
    const float NEG_INF = -INFINITY;
    float x[REG ? LPB_NPT : 8];

    float m = NEG_INF;
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * LPB_THREADS + tid;
        float v[8];
        if (c < nchunk) lp_load8<T>(row, row_end, mb, c, v);
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {
            const float e = (c < nchunk && c * 8 + j < V) ? v[j] : NEG_INF;
            if (REG) x[i * 8 + j] = e;
            m = fmaxf(m, e);
        }
    }
    m = block_max(m, red);
    float s = 0.f;
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * LPB_THREADS + tid;
        if (!REG) {
            float v[8];
            if (c < nchunk) lp_load8<T>(row, row_end, mb, c, v);
            _Pragma("unroll") for (int j = 0; j < 8; ++j) x[j] = (c < nchunk && c * 8 + j < V) ? v[j] : NEG_INF;
        }
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {
            const float e = x[(REG ? i * 8 : 0) + j];
            s += e == NEG_INF ? 0.f : expf(e - m);                       // (a NaN logit stays NaN: it is not -inf)
        }
    }
    m_out = m;
    s_out = block_sum(s, red);
}

// two float64 sums over the workgroup at once; `red` is 32 doubles of LDS; every thread gets both
__device__ __forceinline__ void block_sum2_f64(double& a, double& b, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[16 + w] = b; }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
    for (int i = 0; i < LPB_THREADS / 64; ++i) { ta += red[i]; tb += red[16 + i]; }
    a = ta; b = tb;
}

