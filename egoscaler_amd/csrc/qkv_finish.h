// The arithmetic that qkv_finish_kernel (decode.hip) and qkv_finish_fp8_kernel (kv8.hip) share: one thread's 8 rotation pairs of the
// single-token step's q|k|v product, columns i..i+7 (oa) and half+i..half+i+7 (ob) of one head.  The pieces (slab sum, rounding,
// rotation) are row_pieces.h's, the ones the training-step kernels of elementwise.hip use.
#pragma once
#include "row_pieces.h"

// oa|ob = rope(round(sum_s slab[s])).  `slab` points at column i of the head in slice 0, `cos_row` / `sin_row` at entry i of the
// position's table row.  `rotate`: q and k, not v.
template <typename T>
__device__ __forceinline__ void qkv_sum_round_rope(const float* slab, int sk, long long slab_stride, int half, const float* cos_row,
                                                   const float* sin_row, bool rotate, float (&oa)[8], float (&ob)[8]) {
    float a[8], b[8];
    slab_sum8(slab, sk, slab_stride, a);
    slab_sum8(slab + half, sk, slab_stride, b);
    round_as_stored8<T>(a);
    round_as_stored8<T>(b);
    if (rotate) {
        float c[8], sn[8];
        load8<float>(cos_row, c);
        load8<float>(sin_row, sn);
        rope_rotate8<T>(a, b, c, sn, false, 0x3f, oa, ob);         // fp32: pairs 0..5 fused, 6 and 7 rounded, in both kernels
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { oa[j] = a[j]; ob[j] = b[j]; }
    }
}
