// The arithmetic that the row kernels share, each piece written once: every kernel that sums K-slice slabs, rounds "as stored", applies
// RMSNorm to a row or rotates q|k calls these, so "the fused kernel equals the separate kernels bit for bit" holds by construction.
// Users: the RMSNorm and RoPE kernels of elementwise.hip, qkv_finish.h (decode.hip, kv8.hip).  Device functions only; each kernel keeps
// its own loop shape, element-to-lane mapping and grid.
#pragma once
#include "common.h"

// v = sum_s slab[s], 8 columns at p, slice s at p + s * stride (EGOMI_EPI_SLABS, include/egomi.h).  Starts from 0 and adds in slice
// order, like splitk_reduce_kernel: the order is the contract.
__device__ __forceinline__ void slab_sum8(const float* p, int sk, long long stride, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    for (int s = 0; s < sk; ++s) {
        float t[8];
        load8<float>(p + (long long)s * stride, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += t[j];
    }
}

// v as a T array would hold it: what the combine pass (or any earlier kernel) would have stored
template <typename T>
__device__ __forceinline__ float round_as_stored(float v) { return sizeof(T) == 2 ? bf2f(f2bf(v)) : v; }
template <typename T>
__device__ __forceinline__ void round_as_stored8(float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = round_as_stored<T>(v[j]);
}

// y[0..7] = w * T(x * rstd): HF LlamaRMSNorm (modeling_llama.py:53-67) casts x_hat back to the input dtype before the weight multiply
template <typename T>
__device__ __forceinline__ void rmsnorm_apply_store8(const float (&x)[8], float rstd, const T* w, T* y) {
    float ww[8], o[8];
    load8<T>(w, ww);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = ww[j] * round_as_stored<T>(x[j] * rstd);
    store8<T>(y, o);
}

// One rotation pair: oa = a*c - b*s, ob = b*c + a*s (HF apply_rotary_pos_emb with the half-split rotate_half).
// bf16: the tables are cast to bf16 and each product is rounded to bf16 (the sum is rounded by the store): one result, `fuse` is unused.
// fp32: each output is a sum of two products, which -ffp-contract=fast rounds in more than one way.  The results are pinned bit for
// bit, so the rounding is written out and the caller says which one its kernel has always had:
//   ROPE_ROUNDED   both products rounded;
//   ROPE_FUSE_COS  the product with the cosine fused into the sum, the product with the sine rounded;
//   ROPE_FUSE_MIX  oa as ROPE_FUSE_COS, ob with the product with the sine fused and the product with the cosine rounded.
// No numerical reason separates them: they are what the compiler made of `a*c + (-b)*s` in each kernel before the rounding was written
// down.  A change that is allowed to move fp32 results can use one value everywhere.
enum { ROPE_ROUNDED = 0, ROPE_FUSE_COS = 1, ROPE_FUSE_MIX = 2 };
template <typename T>
__device__ __forceinline__ void rope_pair(float a, float b, float c, float s, int fuse, float& oa, float& ob) {
#pragma clang fp contract(off)
    if (sizeof(T) == 2) {
        c = bf2f(f2bf(c)); s = bf2f(f2bf(s));
        oa = bf2f(f2bf(a * c)) + bf2f(f2bf(-b * s));
        ob = bf2f(f2bf(b * c)) + bf2f(f2bf(a * s));
    } else if (fuse == ROPE_ROUNDED) {
        oa = a * c + -b * s;
        ob = b * c + a * s;
    } else {
        oa = fmaf(a, c, -b * s);
        ob = fuse == ROPE_FUSE_COS ? fmaf(b, c, a * s) : fmaf(a, s, b * c);
    }
}

// 8 pairs.  inverse: the transpose rotation (backward).  fp32: bit j of `fuse_cos` set = pair j is ROPE_FUSE_COS, clear = ROPE_ROUNDED
// (a compile-time constant at every call site; it differs between kernels, see rope_pair).
template <typename T>
__device__ __forceinline__ void rope_rotate8(const float (&a)[8], const float (&b)[8], const float (&c)[8], const float (&s)[8], bool inverse,
                                             unsigned fuse_cos, float (&oa)[8], float (&ob)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) rope_pair<T>(a[j], b[j], c[j], inverse ? -s[j] : s[j], (fuse_cos >> j) & 1, oa[j], ob[j]);
}
