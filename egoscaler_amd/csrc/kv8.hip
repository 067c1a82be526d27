// FP8 (OCP e4m3fn) KV cache for single-token decode: the twins of kv_append, qkv_finish, attn_decode (decode.hip) and
// attn_decode_rows (beam.hip) on a cache of 8-bit codes with one fp32 scale per (layer, row, head, position).
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
// Decode attention: score_t = (sum_j code_j * q_j * scale) * s_k[t]; acc += (p_t * s_v[t]) * code, with attn_decode's online softmax
// and wave combine.  A masked or out-of-range key never reaches the accumulators through a multiplication by p = 0: its code words and
// its p * s_v are SELECTED to zero (unwritten cache bytes may hold NaN codes 0x7F / 0xFF and NaN scales, and NaN * 0 is NaN).
#include "common.h"
#include "fp8.h"
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
// RoPE(pos) on q and k with the bf16 kernel's rounding sequence, q -> qkv (bit-equal to qkv_finish).  One thread per 8 rotation pairs
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
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s2 = 0; s2 < sk; ++s2) {
            float t[8];
            load8<float>(slabs + (long long)s2 * slab_stride + b * 3 * d + col, t);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] += t[j];
            load8<float>(slabs + (long long)s2 * slab_stride + b * 3 * d + col + half, t);
#pragma unroll
            for (int j = 0; j < 8; ++j) bb[j] += t[j];
        }
        if (sizeof(T) == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] = bf2f(f2bf(a[j])); bb[j] = bf2f(f2bf(bb[j])); }
        }
        float oa[8], ob[8];
        if (part < 2) {
            float c[8], sn[8];
            load8<float>(cos_tab + (long long)pos * half + i, c);
            load8<float>(sin_tab + (long long)pos * half + i, sn);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float cj = c[j], sj = sn[j];
                if (sizeof(T) == 2) {
                    cj = bf2f(f2bf(cj)); sj = bf2f(f2bf(sj));
                    oa[j] = bf2f(f2bf(a[j] * cj)) + bf2f(f2bf(-bb[j] * sj));
                    ob[j] = bf2f(f2bf(bb[j] * cj)) + bf2f(f2bf(a[j] * sj));
                } else {
                    oa[j] = a[j] * cj + (-bb[j]) * sj;
                    ob[j] = bb[j] * cj + a[j] * sj;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { oa[j] = a[j]; ob[j] = bb[j]; }
        }
        if (part == 0) {
            store8<T>(qkv + b * ld + col, oa);
            store8<T>(qkv + b * ld + col + half, ob);
        }
        // parts are uniform over a head's CPV lanes, but the q group's lanes take part in no shuffle of another group: every lane
        // computes amax, the q lanes just do not store
        if (sizeof(T) == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { oa[j] = bf2f(f2bf(oa[j])); ob[j] = bf2f(f2bf(ob[j])); }    // what the bf16 cache would hold
        }
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

// ------------------------------------------------------------------------------------------------
// attn_decode_fp8 / attn_decode_rows_fp8: attn_decode_kernel / attn_decode_rows_kernel on the fp8 cache.  256 threads per (b, h), 4 lanes
// per key (HD/4 dims each), and each lane takes TWO keys per iteration (slot and slot + 16): 32 keys per wave-iteration, so a lane keeps
// the bf16 kernel's bytes in flight (2 x HD/4 code bytes per tensor).  ROWS: key t of logical row b lives in physical row kv_row[b, t]
// (an entry outside [0, n_phys) is a masked key); block order (item, head, beam) as in attn_decode_rows_kernel.
// ------------------------------------------------------------------------------------------------
template <int DPL>
__device__ __forceinline__ void load_codes(const uint8_t* p, uint32_t (&w)[DPL / 4]) {
    if constexpr (DPL % 16 == 0) {
#pragma unroll
        for (int c = 0; c < DPL / 16; ++c) {
            const u32x4 r = *reinterpret_cast<const u32x4*>(p + c * 16);
            w[4 * c] = r[0]; w[4 * c + 1] = r[1]; w[4 * c + 2] = r[2]; w[4 * c + 3] = r[3];
        }
    } else {
        const u32x2 r = *reinterpret_cast<const u32x2*>(p);
        w[0] = r[0]; w[1] = r[1];
    }
}

template <typename T, int HD, bool ROWS>
__global__ __launch_bounds__(256) void attn_decode_fp8_kernel(const T* q, long long ld_q, const uint8_t* kc, const uint8_t* vc, const float* ks,
                                                              const float* vs, const int* kv_row, long long ld_kv, int n_phys, const uint8_t* key_mask,
                                                              long long ld_mask, T* out, long long ld_o, int H, int nb, int Smax, int Tlen, float scale) {
    constexpr int DPL = HD / 4, NW = DPL / 4;
    __shared__ float sm_m[4], sm_l[4];
    __shared__ float sm_acc[4][HD];
    int b, h;
    if (ROWS) {
        const int j = blockIdx.x % nb, bi = blockIdx.x / (nb * H);
        h = (blockIdx.x / nb) % H;
        b = bi * nb + j;
    } else {
        b = blockIdx.x / H;
        h = blockIdx.x % H;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane & 3, kslot = lane >> 2;
    float qv[DPL];
#pragma unroll
    for (int c = 0; c < DPL / 8; ++c) {
        float t[8];
        load8<T>(q + (long long)b * ld_q + (long long)h * HD + part * DPL + c * 8, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) qv[c * 8 + j] = t[j] * scale;
    }
    const int* rows = ROWS ? kv_row + (long long)b * ld_kv : nullptr;
    float m = -INFINITY, l = 0.f, acc[DPL];
#pragma unroll
    for (int j = 0; j < DPL; ++j) acc[j] = 0.f;
    for (int k0 = wave * 32; k0 < Tlen; k0 += 128) {
        bool ok[2];
        long long slot[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int key = k0 + kslot + 16 * u;
            ok[u] = key < Tlen;
            const int kr = key < Tlen ? key : Tlen - 1;
            int pr = b;
            if (ROWS) {
                pr = rows[kr];
                if (pr < 0 || pr >= n_phys) { ok[u] = false; pr = 0; }
            }
            if (ok[u] && key_mask) ok[u] = key_mask[(long long)b * ld_mask + key] != 0;
            slot[u] = ((long long)pr * H + h) * Smax + kr;
        }
        uint32_t kw[2][NW], vw[2][NW];
        float sk[2], sv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            load_codes<DPL>(kc + slot[u] * HD + part * DPL, kw[u]);
            load_codes<DPL>(vc + slot[u] * HD + part * DPL, vw[u]);
            sk[u] = ks[slot[u]];
            sv[u] = vs[slot[u]];
        }
        float sc[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < NW; ++c) {
                float x[4];
                e4m3fn_decode4(ok[u] ? kw[u][c] : 0u, x);                 // select, never multiply a NaN code by zero
#pragma unroll
                for (int j = 0; j < 4; ++j) dot += x[j] * qv[c * 4 + j];
            }
            dot += __shfl_xor(dot, 1, 64);
            dot += __shfl_xor(dot, 2, 64);
            sc[u] = ok[u] ? dot * sk[u] : -INFINITY;
        }
        float mx = fmaxf(sc[0], sc[1]);
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float m_new = fmaxf(m, mx);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = m == -INFINITY ? 0.f : __expf(m - m_safe);
        const float p0 = ok[0] ? __expf(sc[0] - m_safe) : 0.f;
        const float p1 = ok[1] ? __expf(sc[1] - m_safe) : 0.f;
        float ps = p0 + p1;
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) ps += __shfl_xor(ps, o, 64);
        l = l * alpha + ps;
        m = m_new;
        const float pv0 = ok[0] ? p0 * sv[0] : 0.f, pv1 = ok[1] ? p1 * sv[1] : 0.f;
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            float x0[4], x1[4];
            e4m3fn_decode4(ok[0] ? vw[0][c] : 0u, x0);
            e4m3fn_decode4(ok[1] ? vw[1][c] : 0u, x1);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c * 4 + j] = acc[c * 4 + j] * alpha + pv0 * x0[j] + pv1 * x1[j];
        }
    }
    // reduce the 16 key slots of the wave (lanes with equal `part`)
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
        float a = acc[j];
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
        acc[j] = a;
    }
    if (lane < 4) {
#pragma unroll
        for (int j = 0; j < DPL; ++j) sm_acc[wave][lane * DPL + j] = acc[j];
        if (lane == 0) { sm_m[wave] = m; sm_l[wave] = l; }
    }
    __syncthreads();
    if (threadIdx.x < HD) {
        float mm = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
        const float ms = mm == -INFINITY ? 0.f : mm;
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = sm_m[w] == -INFINITY ? 0.f : __expf(sm_m[w] - ms);
            num += f * sm_acc[w][threadIdx.x];
            den += f * sm_l[w];
        }
        Cvt<T>::st(out + (long long)b * ld_o + (long long)h * HD + threadIdx.x, den > 0.f ? num / den : 0.f);
    }
}

static int attn_decode_fp8_launch(bool rows, const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale,
                                  const float* vscale, const int32_t* kv_row, int64_t ld_kv, int n_phys, const uint8_t* key_mask, int64_t ld_mask,
                                  void* out, int64_t ld_o, int B, int nb, int H, int hd, int Smax, int T_len, float scale, int dtype,
                                  egomi_stream_t stream) {
    if (dtype != EGOMI_F32 && dtype != EGOMI_BF16) return EGOMI_E_BADARG;
    if (hd != 32 && hd != 64 && hd != 128) return EGOMI_E_UNSUPPORTED;
    if (((uintptr_t)kcodes | (uintptr_t)vcodes | (uintptr_t)q) & 15 || ((uintptr_t)kscale | (uintptr_t)vscale) & 3) return EGOMI_E_SHAPE;
    hipStream_t s = (hipStream_t)stream;
#define AD8(TT, HDV, RW)                                                                                                                    \
    EGOMI_LAUNCH((attn_decode_fp8_kernel<TT, HDV, RW>), dim3(B * H), dim3(256), 0, s, (const TT*)q, (long long)ld_q, kcodes, vcodes, kscale, \
                 vscale, (const int*)kv_row, (long long)ld_kv, n_phys, key_mask, (long long)ld_mask, (TT*)out, (long long)ld_o, H, nb, Smax, T_len,  \
                 scale)
#define AD8_HD(TT, RW)                                                                  \
    do {                                                                                \
        if (hd == 128) AD8(TT, 128, RW); else if (hd == 64) AD8(TT, 64, RW); else AD8(TT, 32, RW); \
    } while (0)
    if (dtype == EGOMI_BF16) { if (rows) AD8_HD(bf16_t, true); else AD8_HD(bf16_t, false); }
    else { if (rows) AD8_HD(float, true); else AD8_HD(float, false); }
#undef AD8_HD
#undef AD8
    return egomi_launch_status();
}

extern "C" int egomi_attn_decode_fp8(const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale, const float* vscale,
                                     const uint8_t* key_mask, int64_t ld_mask, void* out, int64_t ld_o, int B, int H, int hd, int Smax, int T_len,
                                     float scale, int dtype, egomi_stream_t stream) {
    if (!q || !kcodes || !vcodes || !kscale || !vscale || !out) return EGOMI_E_BADARG;
    if (B <= 0 || H <= 0 || T_len <= 0 || T_len > Smax || ld_q % 8 || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd) return EGOMI_E_SHAPE;
    if (key_mask && ld_mask < T_len) return EGOMI_E_SHAPE;
    return attn_decode_fp8_launch(false, q, ld_q, kcodes, vcodes, kscale, vscale, nullptr, 0, B, key_mask, ld_mask, out, ld_o, B, 1, H, hd, Smax,
                                  T_len, scale, dtype, stream);
}

extern "C" int egomi_attn_decode_rows_fp8(const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale,
                                          const float* vscale, const int32_t* kv_row, int64_t ld_kv, int n_phys, const uint8_t* key_mask,
                                          int64_t ld_mask, void* out, int64_t ld_o, int B, int nb, int H, int hd, int Smax, int T_len, float scale,
                                          int dtype, egomi_stream_t stream) {
    if (!q || !kcodes || !vcodes || !kscale || !vscale || !kv_row || !out) return EGOMI_E_BADARG;
    if (B <= 0 || nb <= 0 || B % nb || H <= 0 || n_phys <= 0 || T_len <= 0 || T_len > Smax || ld_kv < T_len || ld_q % 8 ||
        ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd) return EGOMI_E_SHAPE;
    if (key_mask && ld_mask < T_len) return EGOMI_E_SHAPE;
    return attn_decode_fp8_launch(true, q, ld_q, kcodes, vcodes, kscale, vscale, kv_row, ld_kv, n_phys, key_mask, ld_mask, out, ld_o, B, nb, H, hd,
                                  Smax, T_len, scale, dtype, stream);
}
