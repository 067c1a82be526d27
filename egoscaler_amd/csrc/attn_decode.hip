// Single-token decode attention (A13): one query per (row, head) against keys [0, T) of a static KV cache.  ONE kernel serves the four
// entry points egomi_attn_decode, egomi_attn_decode_rows, egomi_attn_decode_fp8 and egomi_attn_decode_rows_fp8; they differ in a cache
// policy (where a key's slice is fetched from and how it becomes floats) and in ROWS (whether the physical cache row comes from a table).
//
// Replaces the cached branch of HF LlamaAttention.forward (modeling_llama.py:243-281 with past_key_values.update) + eager attention for
// one query.  HBM-bound: per step each (row, head) streams its K and V rows once; cache layout [B, H, Smax, hd] keeps every stream
// contiguous.  Every length is a launch argument, so 32 steps can be captured into one hipGraph with per-step constants.
//
// One 256-thread block per (row, head); 4 lanes per key (HD/4 dims per lane), 16 key slots per wave, Cache::KPL keys per lane and round,
// online softmax per wave, waves combined through LDS in wave order.  The order of the floating-point operations is part of the
// contract (the forms are pinned bit for bit): each policy keeps the association its form has always had.
#include "common.h"
#include "fp8.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
// Cache policies.  A lane's slice of one key is DPL = HD/4 consecutive dims of cache slot ((row * H + h) * Smax + t); the kernel asks for
// it in chunks of CH floats.  fetch() starts a key's loads, k_chunk() / v_chunk() turn chunk c into floats, score() finishes the reduced
// q.k of a visible key, v_weight() is what multiplies the key's V values.
// ------------------------------------------------------------------------------------------------

// The model's dtype, [n_rows, H, Smax, HD].  An invisible key is still read (its clamped slot is in bounds) and multiplied by p = 0.
template <typename T, int HD>
struct DenseCache {
    static constexpr int KPL = 1, CH = 8, DPL = HD / 4;
    const T *kc, *vc;
    struct Key { long long off; };
    __device__ __forceinline__ void fetch(Key& k, long long slot, int part) const { k.off = slot * HD + part * DPL; }
    __device__ __forceinline__ void k_chunk(const Key& k, bool, int c, float (&x)[CH]) const { load8<T>(kc + k.off + c * 8, x); }
    __device__ __forceinline__ void v_chunk(const Key& k, bool, int c, float (&x)[CH]) const { load8<T>(vc + k.off + c * 8, x); }
    __device__ __forceinline__ float score(const Key&, float dot) const { return dot; }
    __device__ __forceinline__ float v_weight(const Key&, bool, float p) const { return p; }
};

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

// e4m3fn codes uint8 [n_rows, H, Smax, HD] with one fp32 scale per slot (numerics: the header of kv8.hip, normative):
// score_t = (sum_j code_j * q_j * scale) * s_k[t]; acc += (p_t * s_v[t]) * code.  A lane takes TWO keys per round (slot and slot + 16), 32
// keys per wave-round, so it keeps the dense form's bytes in flight (2 x HD/4 code bytes per tensor).  An invisible key never reaches
// the accumulators through a multiplication by p = 0: its code words and its p * s_v are SELECTED to zero (unwritten cache bytes may
// hold NaN codes 0x7F / 0xFF and NaN scales, and NaN * 0 is NaN).
template <typename T, int HD>
struct Fp8Cache {
    static constexpr int KPL = 2, CH = 4, DPL = HD / 4, NW = DPL / 4;
    const uint8_t *kc, *vc;
    const float *ks, *vs;
    struct Key { uint32_t kw[NW], vw[NW]; float sk, sv; };
    __device__ __forceinline__ void fetch(Key& k, long long slot, int part) const {
        load_codes<DPL>(kc + slot * HD + part * DPL, k.kw);
        load_codes<DPL>(vc + slot * HD + part * DPL, k.vw);
        k.sk = ks[slot];
        k.sv = vs[slot];
    }
    __device__ __forceinline__ void k_chunk(const Key& k, bool ok, int c, float (&x)[CH]) const { e4m3fn_decode4(ok ? k.kw[c] : 0u, x); }
    __device__ __forceinline__ void v_chunk(const Key& k, bool ok, int c, float (&x)[CH]) const { e4m3fn_decode4(ok ? k.vw[c] : 0u, x); }
    __device__ __forceinline__ float score(const Key& k, float dot) const { return dot * k.sk; }
    __device__ __forceinline__ float v_weight(const Key& k, bool ok, float p) const { return ok ? p * k.sv : 0.f; }
};

// ------------------------------------------------------------------------------------------------
// The kernel.  key_mask [B, T] (1 = visible) may be NULL.  ROWS: key t of logical row b lives in physical row kv_row[b, t] of the
// [n_phys, H, Smax, hd] cache; an entry outside [0, n_phys) makes the key invisible and its read goes to row 0.  Block order with ROWS
// is (item, head, beam): the nb beams of an item read the same prompt rows back to back, so the shared prompt comes from HBM once and
// from L2 / MALL for the other beams.
// At head_dim 32 every form fits 64 VGPRs, eight resident waves per SIMD; the launch bound says so, because left alone the scheduler spends
// four registers more on the fp8 rows form and drops the eighth wave (profiles/attn_decode_unify.txt).
// ------------------------------------------------------------------------------------------------
template <typename T, int HD, typename Cache, bool ROWS>
__global__ __launch_bounds__(256, HD == 32 ? 8 : 1) void attn_decode_kernel(const Cache cache, const T* q, long long ld_q, const int* kv_row, long long ld_kv,
                                                          int n_phys, const uint8_t* key_mask, long long ld_mask, T* out, long long ld_o, int H,
                                                          int nb, int Smax, int Tlen, float scale) {
    constexpr int DPL = HD / 4, KPL = Cache::KPL, CH = Cache::CH;      // dims per lane, keys per lane and round, floats per chunk
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
    const int part = lane & 3, kslot = lane >> 2;                       // 16 key slots per wave
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
    for (int k0 = wave * 16 * KPL; k0 < Tlen; k0 += 64 * KPL) {
        bool ok[KPL];
        long long slot[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
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
        typename Cache::Key kv[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) cache.fetch(kv[u], slot[u], part);
        float sc[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < DPL / CH; ++c) {
                float x[CH];
                cache.k_chunk(kv[u], ok[u], c, x);
#pragma unroll
                for (int j = 0; j < CH; ++j) dot += x[j] * qv[c * CH + j];
            }
            dot += __shfl_xor(dot, 1, 64);
            dot += __shfl_xor(dot, 2, 64);
            sc[u] = ok[u] ? cache.score(kv[u], dot) : -INFINITY;
        }
        float mx = sc[0];
#pragma unroll
        for (int u = 1; u < KPL; ++u) mx = fmaxf(mx, sc[u]);
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float m_new = fmaxf(m, mx);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = m == -INFINITY ? 0.f : __expf(m - m_safe);
        float p[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) p[u] = ok[u] ? __expf(sc[u] - m_safe) : 0.f;
        float ps = p[0];
#pragma unroll
        for (int u = 1; u < KPL; ++u) ps += p[u];
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) ps += __shfl_xor(ps, o, 64);
        l = l * alpha + ps;
        m = m_new;
        float pv[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) pv[u] = cache.v_weight(kv[u], ok[u], p[u]);
#pragma unroll
        for (int c = 0; c < DPL / CH; ++c) {
            float x[KPL][CH];
#pragma unroll
            for (int u = 0; u < KPL; ++u) cache.v_chunk(kv[u], ok[u], c, x[u]);
            // acc * alpha + sum_u pv[u] * x[u] is a sum of products, which -ffp-contract=fast may round in more than one way (and then
            // holds the fp8 loads in up to 41 more VGPRs); the results are pinned bit for bit, so the association is written out:
            // acc * alpha is rounded and every key is one fma onto it.  Only the dense cache at head_dim 32 is pinned the other way
            // round, p * x rounded and acc * alpha fused: no numerical reason, it is what the compiler made of that instantiation
            // before the rounding was written down.  A change that is allowed to move results can drop the branch.
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                float a;
                if (KPL == 1 && HD == 32) {
                    a = fmaf(acc[c * CH + j], alpha, pv[0] * x[0][j]);
                } else {
                    a = acc[c * CH + j] * alpha;
#pragma unroll
                    for (int u = 0; u < KPL; ++u) a = fmaf(pv[u], x[u][j], a);
                }
                acc[c * CH + j] = a;
            }
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

// ------------------------------------------------------------------------------------------------
// Host side: one launcher behind the four entry points.  Each entry point keeps its own pointer and shape checks.
// ------------------------------------------------------------------------------------------------
namespace {
struct DecodeArgs {
    const void *q, *kc, *vc;
    const float *ks, *vs;                      // fp8 cache only
    const int32_t* kv_row;                     // rows forms only
    int64_t ld_q, ld_kv, ld_mask, ld_o;
    const uint8_t* key_mask;
    void* out;
    int n_phys, B, nb, H, hd, Smax, T_len, dtype;
    float scale;
    egomi_stream_t stream;
};

template <typename T, int HD, bool ROWS, typename Cache>
void launch_cache(const DecodeArgs& a, Cache cache) {
    EGOMI_LAUNCH((attn_decode_kernel<T, HD, Cache, ROWS>), dim3(a.B * a.H), dim3(256), 0, (hipStream_t)a.stream, cache, (const T*)a.q,
                 (long long)a.ld_q, (const int*)a.kv_row, (long long)a.ld_kv, a.n_phys, a.key_mask, (long long)a.ld_mask, (T*)a.out,
                 (long long)a.ld_o, a.H, a.nb, a.Smax, a.T_len, a.scale);
}
template <typename T, int HD, bool ROWS>
void launch_hd(bool fp8, const DecodeArgs& a) {
    if (fp8) launch_cache<T, HD, ROWS>(a, Fp8Cache<T, HD>{(const uint8_t*)a.kc, (const uint8_t*)a.vc, a.ks, a.vs});
    else launch_cache<T, HD, ROWS>(a, DenseCache<T, HD>{(const T*)a.kc, (const T*)a.vc});
}
template <typename T, bool ROWS>
void launch_dtype(bool fp8, const DecodeArgs& a) {
    if (a.hd == 128) launch_hd<T, 128, ROWS>(fp8, a); else if (a.hd == 64) launch_hd<T, 64, ROWS>(fp8, a); else launch_hd<T, 32, ROWS>(fp8, a);
}

// After the caller's shape checks: another dtype is a bad argument, another head_dim is unsupported.  Only the fp8 forms have ever
// checked alignment (16 B for q and the codes, 4 B for the scales); the dense forms do not.
int attn_decode_launch(bool fp8, bool rows, const DecodeArgs& a) {
    if (a.dtype != EGOMI_F32 && a.dtype != EGOMI_BF16) return EGOMI_E_BADARG;
    if (a.hd != 32 && a.hd != 64 && a.hd != 128) return EGOMI_E_UNSUPPORTED;
    if (fp8 && (((uintptr_t)a.kc | (uintptr_t)a.vc | (uintptr_t)a.q) & 15 || ((uintptr_t)a.ks | (uintptr_t)a.vs) & 3)) return EGOMI_E_SHAPE;
    if (a.dtype == EGOMI_BF16) { if (rows) launch_dtype<bf16_t, true>(fp8, a); else launch_dtype<bf16_t, false>(fp8, a); }
    else { if (rows) launch_dtype<float, true>(fp8, a); else launch_dtype<float, false>(fp8, a); }
    return egomi_launch_status();
}

// what all four forms pass; the fp8 forms add ks / vs, the rows forms kv_row, ld_kv, n_phys and nb
DecodeArgs decode_args(const void* q, int64_t ld_q, const void* kc, const void* vc, const uint8_t* key_mask, int64_t ld_mask, void* out, int64_t ld_o,
                       int B, int H, int hd, int Smax, int T_len, float scale, int dtype, egomi_stream_t stream) {
    DecodeArgs a{};
    a.q = q; a.ld_q = ld_q; a.kc = kc; a.vc = vc; a.key_mask = key_mask; a.ld_mask = ld_mask; a.out = out; a.ld_o = ld_o;
    a.B = B; a.H = H; a.hd = hd; a.Smax = Smax; a.T_len = T_len; a.scale = scale; a.dtype = dtype; a.stream = stream;
    a.n_phys = B; a.nb = 1;                    // every row reads its own physical row
    return a;
}
void set_rows(DecodeArgs& a, const int32_t* kv_row, int64_t ld_kv, int n_phys, int nb) { a.kv_row = kv_row; a.ld_kv = ld_kv; a.n_phys = n_phys; a.nb = nb; }

// checks shared by the four forms, after their NULL checks
bool shape_ok(const DecodeArgs& a) {
    return a.B > 0 && a.H > 0 && a.T_len > 0 && a.T_len <= a.Smax && a.ld_q % 8 == 0 && a.ld_q >= (int64_t)a.H * a.hd &&
           a.ld_o >= (int64_t)a.H * a.hd && !(a.key_mask && a.ld_mask < a.T_len);
}
// and what the rows forms need on top
bool rows_ok(const DecodeArgs& a) { return a.nb > 0 && a.B % a.nb == 0 && a.n_phys > 0 && a.ld_kv >= a.T_len; }
}  // namespace

extern "C" int egomi_attn_decode(const void* q, int64_t ld_q, const void* kcache, const void* vcache, const uint8_t* key_mask, int64_t ld_mask,
                                 void* out, int64_t ld_o, int B, int H, int hd, int Smax, int T_len, float scale, int dtype,
                                 egomi_stream_t stream) {
    if (!q || !kcache || !vcache || !out) return EGOMI_E_BADARG;
    const DecodeArgs a = decode_args(q, ld_q, kcache, vcache, key_mask, ld_mask, out, ld_o, B, H, hd, Smax, T_len, scale, dtype, stream);
    if (!shape_ok(a)) return EGOMI_E_SHAPE;
    return attn_decode_launch(false, false, a);
}

extern "C" int egomi_attn_decode_rows(const void* q, int64_t ld_q, const void* kcache, const void* vcache, const int32_t* kv_row, int64_t ld_kv,
                                      int n_phys, const uint8_t* key_mask, int64_t ld_mask, void* out, int64_t ld_o, int B, int nb, int H, int hd,
                                      int Smax, int T_len, float scale, int dtype, egomi_stream_t stream) {
    if (!q || !kcache || !vcache || !kv_row || !out) return EGOMI_E_BADARG;
    DecodeArgs a = decode_args(q, ld_q, kcache, vcache, key_mask, ld_mask, out, ld_o, B, H, hd, Smax, T_len, scale, dtype, stream);
    set_rows(a, kv_row, ld_kv, n_phys, nb);
    if (!shape_ok(a) || !rows_ok(a)) return EGOMI_E_SHAPE;
    return attn_decode_launch(false, true, a);
}

extern "C" int egomi_attn_decode_fp8(const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale, const float* vscale,
                                     const uint8_t* key_mask, int64_t ld_mask, void* out, int64_t ld_o, int B, int H, int hd, int Smax, int T_len,
                                     float scale, int dtype, egomi_stream_t stream) {
    if (!q || !kcodes || !vcodes || !kscale || !vscale || !out) return EGOMI_E_BADARG;
    DecodeArgs a = decode_args(q, ld_q, kcodes, vcodes, key_mask, ld_mask, out, ld_o, B, H, hd, Smax, T_len, scale, dtype, stream);
    a.ks = kscale; a.vs = vscale;
    if (!shape_ok(a)) return EGOMI_E_SHAPE;
    return attn_decode_launch(true, false, a);
}

extern "C" int egomi_attn_decode_rows_fp8(const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale,
                                          const float* vscale, const int32_t* kv_row, int64_t ld_kv, int n_phys, const uint8_t* key_mask,
                                          int64_t ld_mask, void* out, int64_t ld_o, int B, int nb, int H, int hd, int Smax, int T_len, float scale,
                                          int dtype, egomi_stream_t stream) {
    if (!q || !kcodes || !vcodes || !kscale || !vscale || !kv_row || !out) return EGOMI_E_BADARG;
    DecodeArgs a = decode_args(q, ld_q, kcodes, vcodes, key_mask, ld_mask, out, ld_o, B, H, hd, Smax, T_len, scale, dtype, stream);
    a.ks = kscale; a.vs = vscale;
    set_rows(a, kv_row, ld_kv, n_phys, nb);
    if (!shape_ok(a) || !rows_ok(a)) return EGOMI_E_SHAPE;
    return attn_decode_launch(true, true, a);
}
