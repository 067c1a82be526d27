// Single-token decode against a static KV cache (A13): kv_append, qkv_finish (the q|k|v consumer of the split-K slabs; its arithmetic is
// qkv_finish.h on row_pieces.h, and the slabs + residual + RMSNorm consumer is in elementwise.hip), argmax; the attention over the
// cache is attn_decode.hip.  Replaces the cache update of HF LlamaAttention.forward (modeling_llama.py:243-281 with
// past_key_values.update) and the greedy step of GenerationMixin.generate reached from model_arch.py:94-108.  Cache layout
// [B, H, Smax, hd] keeps every (batch, head) stream contiguous.  All launches take their lengths as arguments, so 32 steps can be
// captured into one hipGraph with per-step constants.
#include "common.h"
#include "qkv_finish.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
// kv_append: rows [B*S, (3*)H*hd] of the k / v projections -> cache[b, h, pos0 + s, :]
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void kv_append_kernel(const T* k, const T* v, long long ld, T* kc, T* vc, int B, int S, int H, int hd,
                                                        int Smax, int pos0) {
    const int cpr = hd / 8;                                      // 8-element chunks per (row, head)
    const long long total = (long long)B * S * H * cpr;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % cpr);
        const int h = (int)((e / cpr) % H);
        const long long row = e / ((long long)cpr * H);
        const int b = (int)(row / S), s = (int)(row % S);
        const long long src = row * ld + (long long)h * hd + c * 8;
        const long long dst = (((long long)b * H + h) * Smax + pos0 + s) * hd + c * 8;
        float x[8];
        load8<T>(k + src, x); store8<T>(kc + dst, x);
        load8<T>(v + src, x); store8<T>(vc + dst, x);
    }
}

extern "C" int egomi_kv_append(const void* k, const void* v, int64_t ld, void* kcache, void* vcache, int B, int S, int H, int hd, int Smax,
                               int pos0, int dtype, egomi_stream_t stream) {
    if (!k || !v || !kcache || !vcache) return EGOMI_E_BADARG;
    if (B <= 0 || S <= 0 || H <= 0 || hd <= 0 || hd % 8 || ld % 8 || ld < (int64_t)H * hd || pos0 < 0 || pos0 + S > Smax) return EGOMI_E_SHAPE;
    const long long total = (long long)B * S * H * (hd / 8);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(kv_append_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)k, (const T*)v,
                                             (long long)ld, (T*)kcache, (T*)vcache, B, S, H, hd, Smax, pos0));
    return egomi_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Consumers of EGOMI_EPI_SLABS products (include/egomi.h): the single-token step's split-K projections leave fp32 K-slice
// slabs; the consumers sum them (slice order, like splitk_reduce_kernel) while doing the next operation of the layer, with
// the rounding sequence of the separate kernels they replace (bit-identical results: the same device functions, row_pieces.h).
// The o_proj / down_proj consumer, egomi_slabs_rmsnorm, is elementwise.hip's rmsnorm_slabs_kernel, the training step's tail-row kernel.
//
// qkv_finish (single-token step): q|k|v = bf16(sum_s slab[s]) [B, 3*H*hd]; RoPE at position `pos` on q and k (rope_vec8_kernel's
// arithmetic, HF apply_rotary_pos_emb; qkv_finish.h), q written to qkv (attn_decode reads it there), k and v written straight into the
// [B,H,Smax,hd] caches at `pos`.  Replaces splitk_reduce + rope + kv_append.  One thread per 8 rotation pairs / 16 v columns.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void qkv_finish_kernel(const float* slabs, int sk, long long slab_stride, T* qkv, long long ld, const float* cos_tab,
                                                         const float* sin_tab, int pos, T* kc, T* vc, int B, int H, int hd, int Smax) {
    const int half = hd >> 1, cpv = half >> 3;
    const long long total = (long long)B * 3 * H * cpv;
    const long long d = (long long)H * hd;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int i = (int)(e % cpv) * 8;
        const int h = (int)((e / cpv) % H);
        const int part = (int)((e / ((long long)cpv * H)) % 3);
        const long long b = e / ((long long)cpv * H * 3);
        const long long col = part * d + (long long)h * hd + i;
        float oa[8], ob[8];
        qkv_sum_round_rope<T>(slabs + b * 3 * d + col, sk, slab_stride, half, cos_tab + (long long)pos * half + i, sin_tab + (long long)pos * half + i,
                              part < 2, oa, ob);
        if (part == 0) {
            store8<T>(qkv + b * ld + col, oa);
            store8<T>(qkv + b * ld + col + half, ob);
        } else {
            T* dst = (part == 1 ? kc : vc) + ((b * H + h) * Smax + pos) * hd + i;
            store8<T>(dst, oa);
            store8<T>(dst + half, ob);
        }
    }
}

extern "C" int egomi_qkv_finish(const float* slabs, int slices, void* qkv, int64_t ld, const float* cos_tab, const float* sin_tab, int pos,
                                void* kcache, void* vcache, int B, int H, int hd, int Smax, int dtype, egomi_stream_t stream) {
    if (!slabs || !qkv || !cos_tab || !sin_tab || !kcache || !vcache) return EGOMI_E_BADARG;
    if (slices < 1 || B <= 0 || H <= 0 || hd <= 0 || (hd / 2) % 8 || ld % 8 || ld < 3ll * H * hd || pos < 0 || pos >= Smax) return EGOMI_E_SHAPE;
    if (((uintptr_t)slabs | (uintptr_t)qkv | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)cos_tab | (uintptr_t)sin_tab) & 15) return EGOMI_E_SHAPE;
    const long long total = (long long)B * 3 * H * (hd / 16);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(qkv_finish_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, slabs, slices, (long long)B * 3 * H * hd,
                                             (T*)qkv, (long long)ld, cos_tab, sin_tab, pos, (T*)kcache, (T*)vcache, B, H, hd, Smax));
    return egomi_launch_status();
}

// ------------------------------------------------------------------------------------------------
// greedy step: ids[b] = argmax_v logits[b, v] (lowest index on ties, like torch.argmax on CPU/GPU for
// distinct values); also stored at seq[b * ld_seq + pos] when seq != NULL.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void argmax_rows_kernel(const T* logits, long long ld, int V, int64_t* ids, int64_t* seq, long long ld_seq, int pos) {
    __shared__ unsigned long long red[16];
    const int b = blockIdx.x;
    unsigned long long best = 0ull;
    for (int c = threadIdx.x; c < V; c += 1024) {
        const float v = Cvt<T>::ld(logits + (long long)b * ld + c);
        unsigned u = __float_as_uint(v);
        u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;                // order-preserving
        const unsigned long long key = ((unsigned long long)u << 32) | (0xFFFFFFFFu - (unsigned)c);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned lo = __shfl_xor((unsigned)(best & 0xFFFFFFFFu), o, 64);
        unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) best = red[w] > best ? red[w] : best;
        const int64_t id = (int64_t)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));
        ids[b] = id;
        if (seq) seq[(long long)b * ld_seq + pos] = id;
    }
}

extern "C" int egomi_argmax_rows(const void* logits, int64_t ld, int B, int V, int64_t* ids, int64_t* seq, int64_t ld_seq, int pos, int dtype,
                                 egomi_stream_t stream) {
    if (!logits || !ids) return EGOMI_E_BADARG;
    if (B <= 0 || V <= 0 || ld < V || (seq && (pos < 0 || pos >= ld_seq))) return EGOMI_E_SHAPE;
    EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(argmax_rows_kernel<T>, dim3(B), dim3(1024), 0, (hipStream_t)stream, (const T*)logits, (long long)ld, V,
                                             ids, seq, (long long)ld_seq, pos));
    return egomi_launch_status();
}
