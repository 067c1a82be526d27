// The pieces of one step's token choice that sample.hip (sample_rows_kernel) and beam.hip (beam_rows_kernel) share: the row a workgroup
// holds, the block-wide integer reductions, HF's TopK / TopP warpers, the Gumbel draw of one element (philox.h) and the repetition-penalty
// scatter.  One copy each: the processed scores and the tokens of egomi_sample_rows AND egomi_beam_rows are these functions' bits, and a
// further logits processor is written once, here.
//
// One 1024-thread workgroup per row; thread tid owns the elements c = i * 1024 + tid, i < niter.  Every fp32 sum below is a per-thread
// accumulation over i ascending followed by one block_sum (common.h); the integer reductions are exact in any order.
#pragma once
#include "common.h"
#include "philox.h"
#include <math.h>

#define CH_THREADS 1024
#define CH_WAVES (CH_THREADS / 64)
#define CH_NPT 32                        // values per thread held in registers: V <= 32768

__device__ __forceinline__ unsigned f2key(float v) {
    unsigned u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);           // order-preserving: a < b  <=>  key(a) < key(b)
}
__device__ __forceinline__ float key2f(unsigned k) {
    k ^= (k >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(k);
}

// block-wide integer sum / 64-bit maximum of a CH_THREADS workgroup; `red` is CH_WAVES words of LDS; all threads get the result
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < CH_WAVES; ++i) t += red[i];
    return t;
}
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(v & 0xFFFFFFFFu), o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        v = other > v ? other : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < CH_WAVES; ++w) v = red[w] > v ? red[w] : v;
    return v;
}

// The workgroup's row.  REG: in registers (V <= CH_THREADS * CH_NPT), padding lanes hold -inf.  Otherwise in the fp32 scores row `sc`
// (L2), which the steps below re-read; a step that writes it ends with a barrier.
template <bool REG> struct ChoiceRow {
    float x[REG ? CH_NPT : 1];
    float* sc;
    int V;
    __device__ __forceinline__ int niter() const { return REG ? CH_NPT : (V + CH_THREADS - 1) / CH_THREADS; }
    __device__ __forceinline__ float get(int i, int c) const { return REG ? x[i] : (c < V ? sc[c] : -INFINITY); }
    __device__ __forceinline__ void set(int i, int c, float v) { if (REG) x[i] = v; else sc[c] = v; }               // c < V
    // position in the stable ascending sort: (value image << 32) | index
    __device__ __forceinline__ unsigned long long key(int i, int c) const { return ((unsigned long long)f2key(get(i, c)) << 32) | (unsigned)c; }
};

// the largest key of the row that is < `below` (0 when there is none); below = ~0: the arg-max with the HIGHEST index on ties = the last
// element of the stable ascending sort
template <bool REG> __device__ __forceinline__ unsigned long long row_max_below(const ChoiceRow<REG>& row, unsigned long long below,
                                                                                unsigned long long* red64) {
    const int tid = threadIdx.x, V = row.V, niter = row.niter();
    unsigned long long best = 0ull;
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * CH_THREADS + tid;
        if (c >= V) continue;
        const unsigned long long k = row.key(i, c);
        if (k < below && k > best) best = k;
    }
    return block_max_u64(best, red64);
}

// HF TopKLogitsWarper with the effective k (top_k, raised to min_tokens_to_keep by the caller): the k-th largest value by a 32-step radix
// select on the integer image (count(key >= candidate) per step); everything below it is removed, ties with it are kept (HF: scores < kth).
template <bool REG> __device__ __forceinline__ void top_k_step(ChoiceRow<REG>& row, int k, int* redi) {
    const int tid = threadIdx.x, V = row.V, niter = row.niter();
    if (k <= 0 || k >= V) return;
    unsigned prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        int n = 0;
        _Pragma("unroll") for (int i = 0; i < niter; ++i) { const int c = i * CH_THREADS + tid; n += (c < V && f2key(row.get(i, c)) >= cand) ? 1 : 0; }
        if (block_sum_int(n, redi) >= k) prefix = cand;
    }
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * CH_THREADS + tid;
        if (c < V && f2key(row.get(i, c)) < prefix) row.set(i, c, -INFINITY);
    }
    if (!REG) __syncthreads();
}

// HF TopPLogitsWarper.  HF sorts ascending (stable), takes softmax + cumsum and removes the maximal prefix whose cumulative probability is
// <= 1 - top_p.  With e = exp(x - max): "prefix mass <= thr" is monotone in the (value, index) order, so a radix walk over the 64-bit key
// finds the first kept element without sorting: 32 value steps + ceil(log2 V) index steps, each a block-wide fp32 sum.  Ties at the
// boundary value are removed lowest index first, exactly what the stable ascending sort does.  `top` is the row's largest key
// (row_max_below(~0)); keys >= `keep`, the min_tokens_to_keep-th largest key, are never removed (min_tokens_to_keep = 1: keep = top).
// In registers e is staged once; otherwise the walk recomputes it from the scores row.
template <bool REG> __device__ __forceinline__ void top_p_step(ChoiceRow<REG>& row, float top_p, unsigned long long top, unsigned long long keep,
                                                               float* redf) {
    const int tid = threadIdx.x, V = row.V, niter = row.niter();
    const float NEG_INF = -INFINITY;
    const float m = key2f((unsigned)(top >> 32));
    float zl = 0.f;
    float e[REG ? CH_NPT : 1];                                    // exp(x - max), 0 for removed / padding lanes
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * CH_THREADS + tid;
        const float v = row.get(i, c);
        const float ev = (c < V && v != NEG_INF) ? expf(v - m) : 0.f;
        if (REG) e[i] = ev;
        zl += ev;
    }
    const float Z = block_sum(zl, redf);
    const float thr = (float)(1.0 - (double)top_p) * Z;
    int idx_bits = 1;
    while ((1 << idx_bits) < V) ++idx_bits;
    unsigned long long prefix = 0ull;
    for (int step = 0; step < 32 + idx_bits; ++step) {
        const int bit = step < 32 ? 63 - step : idx_bits - 1 - (step - 32);
        const unsigned long long cand = prefix | (1ull << bit);
        float s = 0.f;
        _Pragma("unroll") for (int i = 0; i < niter; ++i) {
            const int c = i * CH_THREADS + tid;
            const float v = row.get(i, c);
            s += (c < V && row.key(i, c) < cand) ? (REG ? e[i] : (v != NEG_INF ? expf(v - m) : 0.f)) : 0.f;
        }
        if (block_sum(s, redf) <= thr) prefix = cand;
    }
    // everything strictly below `prefix` is the removed prefix of the ascending order
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * CH_THREADS + tid;
        if (c >= V) continue;
        const unsigned long long k = row.key(i, c);
        if (k < prefix && k < keep) row.set(i, c, NEG_INF);
    }
    if (!REG) __syncthreads();
}

// HF RepetitionPenaltyLogitsProcessor on the staged row sc[0:V] for the tokens sq[from:to]: each from its ORIGINAL value orig(t) (the raw
// logit, or its log-prob), so that a token seen twice is penalised once.  The caller puts a barrier on either side.
template <typename F> __device__ __forceinline__ void rep_penalty_scatter(float* sc, int V, const int64_t* sq, int from, int to, float penalty,
                                                                          F orig) {
    for (int j = from + threadIdx.x; j < to; j += CH_THREADS) {
        const long long t = sq[j];
        if (t >= 0 && t < V) {
            const float s = orig(t);
            sc[t] = s < 0.f ? s * penalty : s / penalty;
        }
    }
}
