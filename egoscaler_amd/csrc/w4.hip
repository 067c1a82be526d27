// Int4 weights with group scales for the single-token decode projections (W4A16): q|k|v, o_proj, gate|up and down_proj of a cached
// decode step (HF LlamaAttention / LlamaMLP forward, modeling_llama.py:243-281,174-176; the generate() step of model_arch.py:77-108 /
// pointllm.py:255-275).  The weights are what a decode step streams; 4-bit codes are 0.53 of the fp8 form's bytes (w8.hip).
//
// Numerics (normative).  W bf16 [N, K], K % 32 == 0, N % 4 == 0.
//   groups   group g covers columns [128 g, min(K, 128 g + 128)): the last one may be 32, 64 or 96 wide.  NG = ceil(K / 128).
//   scale    a = max |W[n,k]| over the group; s[g,n] = a / 7.0f (IEEE division), 1.0f when a == 0.
//   code     code[n,k] = clamp(rintf(W[n,k] / s[g,n]), -7, 7): IEEE division, round-half-even (torch.round), no contraction.
//   codes    the nibble code + 8 (1 .. 15), packed uint8 [N, K / 2], row stride a multiple of 16 bytes.  The 32 codes of columns
//            [32 u, 32 u + 32) are bytes [16 u, 16 u + 16) of the row; within the block the order is the natural one: byte b of the
//            row holds column 2 b in its low nibble and column 2 b + 1 in its high nibble (the identity permutation: the decode below
//            masks the even and the odd columns' nibbles into bytes, which no other order makes cheaper).  decode.w4_quantize /
//            w4_unpack restate it.
//   scales   fp32 [NG, N], group-major: the four accumulator rows n .. n + 3 of an MFMA lane are one 16-byte load.
//   product  y[m,n] = sum_g s[g,n] * (sum_{k in g} x[m,k] * code[n,k]), x bf16, fp32 accumulation in a fixed order; a group's partial
//            sum is finished before its scale is applied.
//
// Decode.  An e4m3fn byte b < 16 is the number b * 2^-9 (the subnormals and the first binade are one linear ramp), so a packed word is
// masked into the bytes of its even and of its odd columns, v_cvt_pk_f32_fp8 turns two such bytes into (code + 8) * 2^-9, one
// v_pk_fma_f32 (* 512, - 8) into the two codes, and v_cvt_pk_bf16_f32 packs a pair: 15 VALU instructions per 8 codes, every step exact.
// The codes themselves meet x on v_mfma_f32_16x16x32_bf16, every product exact as in w8.hip; the group's sum G joins the accumulator as
// fma(s, G, acc).  (An offset form, bf16 (16 + nibble) from one and-or and G - 24 sum x, costs 8 instructions per 8 codes, but rounds
// G at 24 |sum x| instead of |G|: on the tiny model one such flipped bf16 rounding in o_proj moved the logits by 2.5e-3 against a bf16
// decoder on the dequantized weights, where this form is bit-equal to it.)
//
// wq_w4_kernel: wq_w8_kernel's structure (w8.hip).  A block = 4 waves on the same 64 weight rows and 16 * MT activation rows (MT = 1 for
// M <= 16, else 2: an M-chunk); the K range is cut over splitk slices x 4 waves in steps of 128 = one scale group, so slot boundaries are
// group boundaries.  Per step a lane reads ONE 16-byte block of each of its 4 weight rows (the 4 lanes of a row: 64 contiguous bytes) and
// the 16 bytes of its rows' scales straight into registers, with the next step's loads in flight under the current MFMAs.  Lane group
// grp = lane >> 4 owns unit 4 c + grp of step c: columns 128 c + 32 grp + 8 p + e meet element e of MFMA p in the weight and in the
// activation fragment alike.  The last slot takes the K % 128 tail as one more step in which lane groups past the tail multiply zeros.
// The 4 waves meet in LDS (fixed order) and the block writes bf16 rows (+ residual) or its fp32 K-slice slab.
// The arguments, the plan, the slab count, the reduce kernel of a planned split and the host entry are wq_gemm.h's, shared with w8.hip.
#include "wq_gemm.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
// quantize_rows_int4: one block per row, a 16-lane cluster per group (8 columns = one packed word per lane).  Off the hot path.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_rows_int4_kernel(const bf16_t* w, long long ldw, int N, int K, uint8_t* codes, long long ldc, float* scales) {
#pragma clang fp contract(off)
    const bf16_t* row = w + (long long)blockIdx.x * ldw;
    uint32_t* out = reinterpret_cast<uint32_t*>(codes + (long long)blockIdx.x * ldc);
    const int nwords = K >> 3;
    for (int base = 0; base < nwords; base += 256) {                     // 256 words = 16 whole groups: a cluster never straddles a group
        const int wi = base + (int)threadIdx.x;
        const bool live = wi < nwords;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = live ? bf2f(row[8 * wi + e]) : 0.f;
        float am = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(v[e]));
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 16));
        const float s = am == 0.f ? 1.0f : am / 7.0f;
        if (!live) continue;
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float c = fminf(fmaxf(rintf(v[e] / s), -7.f), 7.f);
            word |= (uint32_t)((int)c + 8) << (4 * e);
        }
        out[wi] = word;
        if ((threadIdx.x & 15) == 0) scales[(long long)(wi >> 4) * N + blockIdx.x] = s;
    }
}

extern "C" int egomi_quantize_rows_int4(const void* w, int64_t ldw, int N, int K, uint8_t* codes, int64_t ldc, float* scales, egomi_stream_t stream) {
    if (!w || !codes || !scales) return EGOMI_E_BADARG;
    if (N <= 0 || K <= 0 || ldw < K || ldc < K / 2) return EGOMI_E_SHAPE;
    if (((uintptr_t)codes & 3) || (ldc & 3)) return EGOMI_E_SHAPE;
    if (K & 31) return EGOMI_E_UNSUPPORTED;
    EGOMI_LAUNCH(quantize_rows_int4_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (long long)ldw, N, K, codes, (long long)ldc, scales);
    return egomi_launch_status();
}

// ------------------------------------------------------------------------------------------------
// gemm_w4
// ------------------------------------------------------------------------------------------------
// one packed word -> its 8 columns as bf16 (exact), in column order
__device__ __forceinline__ bf16x8 w4_decode8(uint32_t c) {
    const uint32_t ev = c & 0x0F0F0F0Fu, od = (c >> 4) & 0x0F0F0F0Fu;   // bytes = the nibbles of columns 0, 2, 4, 6 / 1, 3, 5, 7
    const f32x2 e0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)ev, false) * 512.f - 8.f;   // columns 0, 2
    const f32x2 e1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)ev, true) * 512.f - 8.f;    // columns 4, 6
    const f32x2 o0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)od, false) * 512.f - 8.f;   // columns 1, 3
    const f32x2 o1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)od, true) * 512.f - 8.f;    // columns 5, 7
    bf16x8 r;
    r[0] = (__bf16)e0[0]; r[1] = (__bf16)o0[0]; r[2] = (__bf16)e0[1]; r[3] = (__bf16)o0[1];
    r[4] = (__bf16)e1[0]; r[5] = (__bf16)o1[0]; r[6] = (__bf16)e1[1]; r[7] = (__bf16)o1[1];
    return r;
}

template <int MT>
__global__ __launch_bounds__(256) void wq_w4_kernel(WqArgs g) {
    __shared__ float red[4][WQ_BN][16 * MT + 1];
    const int item = (int)(blockIdx.x & 7) * g.per_xcd + (int)(blockIdx.x >> 3);    // dispatch round-robins XCDs: item-major per XCD
    if (item >= g.items) return;
    const int mc = item % g.mch, rest = item / g.mch;
    const int slice = rest % g.splitk, nt = rest / g.splitk;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nl = lane & 15, grp = lane >> 4;
    const int n0 = nt * WQ_BN, m0 = mc * 16 * MT;
    const int U = g.K >> 5, C = U >> 2;                                  // 32-deep units, whole 128-deep steps = whole groups
    const int slot = slice * 4 + wave, nslots = g.splitk * 4;
    // slots own whole steps; the last one also takes the ragged last group (U % 4 units)
    const int c0 = (int)((long long)C * slot / nslots), c1 = (int)((long long)C * (slot + 1) / nslots);
    const int tail = slot + 1 == nslots ? U & 3 : 0;
    const uint8_t* wp[4];
    const float* sp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int r = n0 + 16 * j + nl;
        r = r < g.N ? r : g.N - 1;                                       // clamped rows are computed and never stored
        wp[j] = g.w + (long long)r * g.ldw + 16 * grp;
        int n = n0 + 16 * j + 4 * grp;                                   // the lane's accumulator rows n .. n + 3 (N % 4 == 0)
        n = n < g.N ? n : g.N - 4;
        sp[j] = g.s + n;
    }
    const bf16_t* xp[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m0 + 16 * i + nl;
        m = m < g.M ? m : g.M - 1;
        xp[i] = g.x + (long long)m * g.ldx + 32 * grp;
    }
    f32x4 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 wr[2][4];
    f32x4 sr[2][4];
    bf16x8 xr[2][MT][4];
    auto load = [&](int buf, int c) {                                    // step c = group c: units 4 c .. 4 c + 3
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wr[buf][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[j] + (long long)c * 64));
            sr[buf][j] = *reinterpret_cast<const f32x4*>(sp[j] + (long long)c * g.N);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int p = 0; p < 4; ++p) xr[buf][i][p] = *reinterpret_cast<const bf16x8*>(xp[i] + (long long)c * 128 + 8 * p);
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 G[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) G[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const bf16x8 wf = w4_decode8(wr[buf][j][p]);
#pragma unroll
                for (int i = 0; i < MT; ++i) G[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xr[buf][i][p], G[i], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = fmaf(sr[buf][j][r], G[i][r], acc[i][j][r]);
        }
    };
    int c = c0;
    if (c < c1) load(0, c);
    while (c < c1) {
        if (c + 1 < c1) load(1, c + 1);
        compute(0);
        ++c;
        if (c < c1) {
            if (c + 1 < c1) load(0, c + 1);
            compute(1);
            ++c;
        }
    }
    if (tail) {                                                          // group C, `tail` units wide: lane groups past it read unit 4 C and multiply x = 0
        const bool live = grp < tail;
        const long long back = live ? 0 : grp;                           // in units
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wr[0][j] = *reinterpret_cast<const u32x4*>(wp[j] + (long long)C * 64 - back * 16);
            sr[0][j] = *reinterpret_cast<const f32x4*>(sp[j] + (long long)C * g.N);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(xp[i] + (long long)C * 128 - back * 32 + 8 * p);
                xr[0][i][p] = __builtin_bit_cast(bf16x8, live ? v : (u32x4){0u, 0u, 0u, 0u});
            }
        compute(0);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][16 * j + 4 * grp + r][16 * i + nl] = acc[i][j][r];   // D: row n = 4 (lane >> 4) + r, column m = lane & 15
    __syncthreads();
    const int mr = threadIdx.x >> 4, n4 = (threadIdx.x & 15) * 4;
    const int n = n0 + n4;
    if (n >= g.N) return;                                                // N % 4 == 0: n .. n + 3 are all in range
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m0 + 16 * i + mr;
        if (m >= g.M) break;
        const int ml = 16 * i + mr;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ((red[0][n4 + k][ml] + red[1][n4 + k][ml]) + red[2][n4 + k][ml]) + red[3][n4 + k][ml];
        if (g.ws) {                                                      // this K slice's slab [M, N] fp32
            *reinterpret_cast<f32x4*>(g.ws + ((long long)slice * g.M + m) * g.N + n) = (f32x4){v[0], v[1], v[2], v[3]};
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float y = g.res ? v[k] + bf2f(g.res[(long long)m * g.ldr + n + k]) : v[k];
            g.out[(long long)m * g.ldo + n + k] = f2bf(y);
        }
    }
}

struct W4Codec {
    static constexpr int CODES_PER_BYTE = 2;
    static constexpr uintptr_t SCALE_ALIGN_MASK = 15;                    // the scales are read 16 bytes at a time
    static constexpr auto kernel1 = &wq_w4_kernel<1>, kernel2 = &wq_w4_kernel<2>;
};

extern "C" int egomi_gemm_w4_slab_count(int M, int N, int K, int64_t workspace_bytes) { return wq_slab_count(M, N, K, workspace_bytes); }

extern "C" int egomi_gemm_w4(const void* x, int64_t ldx, const uint8_t* codes, int64_t ldw, const float* scales, void* out, int64_t ldo,
                             const void* residual, int64_t ldr, int M, int N, int K, int epilogue, void* workspace, int64_t workspace_bytes,
                             egomi_stream_t stream) {
    return wq_gemm<W4Codec>(x, ldx, codes, ldw, scales, out, ldo, residual, ldr, M, N, K, epilogue, workspace, workspace_bytes, stream);
}
