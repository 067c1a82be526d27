// OCP e4m3fn helpers shared by the fp8 KV cache (kv8.hip, attn_decode.hip) and the fp8 weights of the decode projections (w8.hip).
// Quantisation rule of both (normative): s = amax / 448 (IEEE division), or 1 when amax == 0; code = e4m3fn_rne(x / s) (IEEE division,
// no reciprocal-multiply); value = float(code) * s.  Bit-equal to torch's `(x / s).to(torch.float8_e4m3fn)`.
#pragma once
#include "common.h"

// torch c10 fp8e4m3fn_from_fp32_value: RNE, no saturation (|y| >= 480 -> NaN 0x7F), sign kept (-0 -> 0x80)
__device__ __forceinline__ uint32_t e4m3fn_rne(float f) {
    uint32_t b = __float_as_uint(f);
    const uint32_t sign = b & 0x80000000u;
    b ^= sign;
    uint32_t r;
    if (b >= (1087u << 20)) {
        r = 0x7Fu;
    } else if (b < (121u << 23)) {                                   // below the smallest normal: the magic-add of c10
        r = __float_as_uint(__uint_as_float(b) + __uint_as_float(141u << 23)) - (141u << 23);
    } else {
        r = (b + (uint32_t)(-(120 << 23)) + 0x7FFFFu + ((b >> 20) & 1u)) >> 20;
    }
    return (r | (sign >> 24)) & 0xFFu;
}

__device__ __forceinline__ float e4m3fn_scale(float amax) {
#pragma clang fp contract(off)
    return amax == 0.f ? 1.0f : amax / 448.0f;
}

// 4 codes in one word -> 4 floats (exact)
__device__ __forceinline__ void e4m3fn_decode4(uint32_t w, float* o) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}

