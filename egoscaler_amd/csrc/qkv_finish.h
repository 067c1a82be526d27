// The arithmetic that qkv_finish_kernel (decode.hip) and qkv_finish_fp8_kernel (kv8.hip) share: one thread's 8 rotation pairs of the
// single-token step's q|k|v product, columns i..i+7 (a / oa) and half+i..half+i+7 (bb / ob) of one head.
#pragma once
#include "common.h"

// One fp32 rotation pair: oa = a*c - bb*s, ob = bb*c + a*s.  Each is a sum of two products, which -ffp-contract=fast may round in more
// than one way; the results are pinned bit for bit, so the rounding is written out.  `fused`: the product with the cosine is fused into
// the sum, the product with the sine is rounded; otherwise both products are rounded.
__device__ __forceinline__ void rope_pair_f32(float a, float bb, float c, float s, bool fused, float& oa, float& ob) {
#pragma clang fp contract(off)
    const float as = a * s, bs = -bb * s;
    if (fused) {
        oa = fmaf(a, c, bs);
        ob = fmaf(bb, c, as);
    } else {
        oa = a * c + bs;
        ob = bb * c + as;
    }
}

// oa|ob = rope(round(sum_s slab[s])).  `slab` points at column i of the head in slice 0, `cos_row` / `sin_row` at entry i of the
// position's table row.  The slabs are summed in slice order (like splitk_reduce_kernel) and rounded to what the combine pass would
// have stored; `rotate` (q and k, not v) applies RoPE with rope_vec8_kernel's arithmetic and rounding sequence (HF apply_rotary_pos_emb).
template <typename T>
__device__ __forceinline__ void qkv_sum_round_rope(const float* slab, int sk, long long slab_stride, int half, const float* cos_row,
                                                   const float* sin_row, bool rotate, float (&oa)[8], float (&ob)[8]) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s2 = 0; s2 < sk; ++s2) {
        float t[8];
        load8<float>(slab + (long long)s2 * slab_stride, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += t[j];
        load8<float>(slab + (long long)s2 * slab_stride + half, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) bb[j] += t[j];
    }
    if (sizeof(T) == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = bf2f(f2bf(a[j])); bb[j] = bf2f(f2bf(bb[j])); }       // the product as the combine pass would have stored it
    }
    if (rotate) {
        float c[8], sn[8];
        load8<float>(cos_row, c);
        load8<float>(sin_row, sn);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float cj = c[j], sj = sn[j];
            if (sizeof(T) == 2) {
                cj = bf2f(f2bf(cj)); sj = bf2f(f2bf(sj));
                oa[j] = bf2f(f2bf(a[j] * cj)) + bf2f(f2bf(-bb[j] * sj));
                ob[j] = bf2f(f2bf(bb[j] * cj)) + bf2f(f2bf(a[j] * sj));
            } else {
                // j < 6 fused, the last two pairs not: no numerical reason, it is what the compiler made of `a*c + (-bb)*s` in both
                // kernels before the rounding was written down, kept so that fp32 results do not move.  A change that is allowed to
                // move them can fuse all eight.
                rope_pair_f32(a[j], bb[j], cj, sj, j < 6, oa[j], ob[j]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { oa[j] = a[j]; ob[j] = bb[j]; }
    }
}
