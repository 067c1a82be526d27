// FP8 (OCP e4m3fn) KV cache for single-token decode: the twins of kv_append and qkv_finish (decode.hip) on a cache of 8-bit codes with
// one fp32 scale per (layer, row, head, position), and the numerics of that cache.  Attention over it is the Fp8Cache policy of
// attn_decode.hip.
//
// Layout: codes uint8 [B, H, Smax, hd] per layer (the bf16 cache's layout), scales fp32 [B, H, Smax] per layer (each (b, h) stream
// contiguous).  Decode attention streams hd + 4 bytes per key and tensor instead of 2 * hd.
//
// Numerics (normative).  For each (row, head, position) take the hd values x_j of K (and, separately, of V) that the bf16 / fp32
// kernels would store — after RoPE, and for bf16 after the bf16 rounding those kernels apply:
//   amax   = max_j |x_j|
//   s      = amax / 448.0f  (IEEE division), or 1.0f when amax == 0
//   code_j = e4m3fn_rne(x_j / s)  (IEEE division; no reciprocal-multiply)
//   value  = float(code_j) * s
// e4m3fn_rne is torch's float -> float8_e4m3fn conversion (round to nearest even, |y| >= 480 and NaN -> 0x7F | sign), written out in
// software (fp8.h, shared with w8.hip) so that the codes are bit-equal to torch's `(x / s[..., None]).to(torch.float8_e4m3fn)`.  Decoding uses the hardware
// v_cvt_pk_f32_fp8 (OCP on gfx950), which is exact for every finite code.
//
// Decode attention (attn_decode.hip): score_t = (sum_j code_j * q_j * scale) * s_k[t]; acc += (p_t * s_v[t]) * code, with attn_decode's online softmax
// and wave combine.  A masked or out-of-range key never reaches the accumulators through a multiplication by p = 0: its code words and
// its p * s_v are SELECTED to zero (unwritten cache bytes may hold NaN codes 0x7F / 0xFF and NaN scales, and NaN * 0 is NaN).
#include "common.h"
#include "fp8.h"
#include "qkv_finish.h"
#include <math.h>

// 8 values -> 8 codes (little-endian: element j in byte j)
__device__ __forceinline__ u32x2 kv8_encode8(const float (&x)[8], float s) {
#pragma clang fp contract(off)
    u32x2 w;
    w[0] = e4m3fn_rne(x[0] / s) | (e4m3fn_rne(x[1] / s) << 8) | (e4m3fn_rne(x[2] / s) << 16) | (e4m3fn_rne(x[3] / s) << 24);
    w[1] = e4m3fn_rne(x[4] / s) | (e4m3fn_rne(x[5] / s) << 8) | (e4m3fn_rne(x[6] / s) << 16) | (e4m3fn_rne(x[7] / s) << 24);
    return w;
}

// max over the G consecutive lanes of an aligned group (G a power of two <= 64)
template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------
// kv_append_fp8: rows [B*S, (3*)H*hd] of the k / v projections -> codes[b, h, pos0 + s, :], scales[b, h, pos0 + s].  One thread per
// 8-element chunk (kv_append_kernel's indexing); the CPR = hd / 8 threads of a head vector are consecutive lanes of one wave.
// ------------------------------------------------------------------------------------------------
template <typename T, int CPR>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const T* k, const T* v, long long ld, uint8_t* kc, uint8_t* vc, float* ks, float* vs,
                                                            int B, int S, int H, int Smax, int pos0) {
    constexpr int HD = CPR * 8;
    const long long total = (long long)B * S * H * CPR;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {   // whole groups enter
        const int c = (int)(e % CPR);
        const int h = (int)((e / CPR) % H);
        const long long row = e / ((long long)CPR * H);
        const int b = (int)(row / S), s = (int)(row % S);
        const long long src = row * ld + (long long)h * HD + c * 8;
        const long long slot = ((long long)b * H + h) * Smax + pos0 + s;
        float xk[8], xv[8];
        load8<T>(k + src, xk);
        load8<T>(v + src, xv);
        float ak = 0.f, av = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { ak = fmaxf(ak, fabsf(xk[j])); av = fmaxf(av, fabsf(xv[j])); }
        const float sk = e4m3fn_scale(group_max<CPR>(ak)), sv = e4m3fn_scale(group_max<CPR>(av));
        *reinterpret_cast<u32x2*>(kc + slot * HD + c * 8) = kv8_encode8(xk, sk);
        *reinterpret_cast<u32x2*>(vc + slot * HD + c * 8) = kv8_encode8(xv, sv);
        if (c == 0) { ks[slot] = sk; vs[slot] = sv; }
    }
}

extern "C" int egomi_kv_append_fp8(const void* k, const void* v, int64_t ld, uint8_t* kcodes, uint8_t* vcodes, float* kscale, float* vscale, int B,
                                   int S, int H, int hd, int Smax, int pos0, int dtype, egomi_stream_t stream) {
    if (!k || !v || !kcodes || !vcodes || !kscale || !vscale) return EGOMI_E_BADARG;
    if (B <= 0 || S <= 0 || H <= 0 || ld % 8 || ld < (int64_t)H * hd || pos0 < 0 || pos0 + S > Smax) return EGOMI_E_SHAPE;
    if (hd != 32 && hd != 64 && hd != 128) return EGOMI_E_UNSUPPORTED;
    if (((uintptr_t)kcodes | (uintptr_t)vcodes) & 7 || ((uintptr_t)kscale | (uintptr_t)vscale) & 3) return EGOMI_E_SHAPE;
    const long long total = (long long)B * S * H * (hd / 8);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipStream_t st = (hipStream_t)stream;
#define KA8(CPRV) EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((kv_append_fp8_kernel<T, CPRV>), dim3(grid), dim3(256), 0, st, (const T*)k, (const T*)v, \
                                                           (long long)ld, kcodes, vcodes, kscale, vscale, B, S, H, Smax, pos0))
    if (hd == 128) KA8(16); else if (hd == 64) KA8(8); else KA8(4);
#undef KA8
    return egomi_launch_status();
}

// ------------------------------------------------------------------------------------------------
// qkv_finish_fp8: qkv_finish_kernel (decode.hip) with k and v quantised into the fp8 caches at `pos`.  q|k|v = round(sum of the slabs),
// RoPE(pos) on q and k with the bf16 kernel's rounding sequence (the same code: qkv_finish.h, on the pieces of row_pieces.h), q -> qkv (bit-equal to qkv_finish).  One thread per 8 rotation pairs
// (columns i..i+7 and half+i..half+i+7 of a head): the CPV = hd / 16 threads of a head are consecutive lanes, amax is a CPV-lane
// shuffle reduction.
// ------------------------------------------------------------------------------------------------
template <typename T, int CPV>
__global__ __launch_bounds__(256) void qkv_finish_fp8_kernel(const float* slabs, int sk, long long slab_stride, T* qkv, long long ld, const float* cos_tab,
                                                             const float* sin_tab, int pos, uint8_t* kc, uint8_t* vc, float* ks, float* vs, int B, int H,
                                                             int Smax) {
    constexpr int HD = CPV * 16, half = HD / 2;
    const long long total = (long long)B * 3 * H * CPV;
    const long long d = (long long)H * HD;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {   // whole groups enter
        const int i = (int)(e % CPV) * 8;
        const int h = (int)((e / CPV) % H);
        const int part = (int)((e / ((long long)CPV * H)) % 3);
        const long long b = e / ((long long)CPV * H * 3);
        const long long col = part * d + (long long)h * HD + i;
        float oa[8], ob[8];
        qkv_sum_round_rope<T>(slabs + b * 3 * d + col, sk, slab_stride, half, cos_tab + (long long)pos * half + i, sin_tab + (long long)pos * half + i,
                              part < 2, oa, ob);
        if (part == 0) {
            store8<T>(qkv + b * ld + col, oa);
            store8<T>(qkv + b * ld + col + half, ob);
        }
        // parts are uniform over a head's CPV lanes, but the q group's lanes take part in no shuffle of another group: every lane
        // computes amax, the q lanes just do not store
        round_as_stored8<T>(oa);                                     // what the bf16 cache would hold
        round_as_stored8<T>(ob);
        float am = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) am = fmaxf(am, fmaxf(fabsf(oa[j]), fabsf(ob[j])));
        const float s = e4m3fn_scale(group_max<CPV>(am));
        if (part > 0) {
            const long long slot = (b * H + h) * Smax + pos;
            uint8_t* dst = (part == 1 ? kc : vc) + slot * HD + i;
            *reinterpret_cast<u32x2*>(dst) = kv8_encode8(oa, s);
            *reinterpret_cast<u32x2*>(dst + half) = kv8_encode8(ob, s);
            if (i == 0) (part == 1 ? ks : vs)[slot] = s;
        }
    }
}

extern "C" int egomi_qkv_finish_fp8(const float* slabs, int slices, void* qkv, int64_t ld, const float* cos_tab, const float* sin_tab, int pos,
                                    uint8_t* kcodes, uint8_t* vcodes, float* kscale, float* vscale, int B, int H, int hd, int Smax, int dtype,
                                    egomi_stream_t stream) {
    if (!slabs || !qkv || !cos_tab || !sin_tab || !kcodes || !vcodes || !kscale || !vscale) return EGOMI_E_BADARG;
    if (slices < 1 || B <= 0 || H <= 0 || ld % 8 || ld < 3ll * H * hd || pos < 0 || pos >= Smax) return EGOMI_E_SHAPE;
    if (hd != 32 && hd != 64 && hd != 128) return EGOMI_E_UNSUPPORTED;
    if (((uintptr_t)slabs | (uintptr_t)qkv | (uintptr_t)cos_tab | (uintptr_t)sin_tab) & 15 || ((uintptr_t)kcodes | (uintptr_t)vcodes) & 7 ||
        ((uintptr_t)kscale | (uintptr_t)vscale) & 3) return EGOMI_E_SHAPE;
    const long long total = (long long)B * 3 * H * (hd / 16);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipStream_t st = (hipStream_t)stream;
#define QF8(CPVV) EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((qkv_finish_fp8_kernel<T, CPVV>), dim3(grid), dim3(256), 0, st, slabs, slices,              \
                                                           (long long)B * 3 * H * hd, (T*)qkv, (long long)ld, cos_tab, sin_tab, pos, kcodes, vcodes, \
                                                           kscale, vscale, B, H, Smax))
    if (hd == 128) QF8(8); else if (hd == 64) QF8(4); else QF8(2);
#undef QF8
    return egomi_launch_status();
}
