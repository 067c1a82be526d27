// FP8 (OCP e4m3fn) weights for the single-token decode projections (W8A16): q|k|v, o_proj, gate|up and down_proj of a cached decode
// step (HF LlamaAttention / LlamaMLP forward, modeling_llama.py:243-281,174-176; the generate() step of model_arch.py:77-108 /
// pointllm.py:255-275).  The weights are what a decode step streams; codes halve those bytes.
//
// Numerics (normative).  Per output row n of W [N, K]:  s_n = amax_k |W[n,k]| / 448 (1 when amax == 0), code[n,k] = e4m3fn_rne(W[n,k] / s_n)
// (fp8.h, the KV cache's rule, bit-equal to torch's (W.float() / s[:, None]).to(torch.float8_e4m3fn)).  The product is
//   y[m,n] = s_n * sum_k x[m,k] * float(code[n,k])
// with x bf16, fp32 accumulation in a fixed order, and s_n applied after accumulation (in split-K mode to each K-slice, so the slabs sum
// to the scaled product).  Every e4m3fn value is exact in bf16, so the codes are decoded to bf16 in registers (v_cvt_pk_f32_fp8, then
// v_cvt_pk_bf16_f32) and multiplied on v_mfma_f32_16x16x32_bf16: every product is exact, as in the bf16 kernel.
//
// wq_w8_kernel: gemv_m16_kernel's structure (gemm_fast.hip) with byte-wide weights.  A block = 4 waves on the same 64 weight rows and
// 16 * MT activation rows (MT = 1 for M <= 16, else 2: an M-chunk); the K range is cut over splitk slices x 4 waves in steps of 128.  Per
// 128-deep step a lane reads 2 x 16 B of each of its 4 weight rows (the 4 lanes of a row: 64 contiguous bytes per load instruction)
// straight into registers, with the next step's loads in flight under the current MFMAs.  A lane's K positions within a step are
// {16 grp .. 16 grp + 15} and {64 + 16 grp .. 64 + 16 grp + 15}; the activation fragment uses the same map, so every k meets its own k.
// The 4 waves meet in LDS (fixed order) and the block writes bf16 rows (+ residual) or its fp32 K-slice slab.  M > 16: the blocks of one
// weight tile (its M-chunks) are consecutive work items on one XCD, so the tile crosses HBM once and the other chunks read it from L2.
// The arguments, the plan, the slab count, the reduce kernel of a planned split and the host entry are wq_gemm.h's, shared with w4.hip.
#include "wq_gemm.h"
#include "fp8.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
// quantize_rows_fp8: one block per row; amax, s, codes.  Runs once per set of weights, off the hot path.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const bf16_t* w, long long ldw, int K, uint8_t* codes, long long ldc, float* scales) {
#pragma clang fp contract(off)
    __shared__ float red[16];
    const bf16_t* row = w + (long long)blockIdx.x * ldw;
    float am = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) am = fmaxf(am, fabsf(bf2f(row[k])));
    const float s = e4m3fn_scale(block_max(am, red));
    uint8_t* out = codes + (long long)blockIdx.x * ldc;
    for (int k = threadIdx.x; k < K; k += 256) out[k] = (uint8_t)e4m3fn_rne(bf2f(row[k]) / s);
    if (threadIdx.x == 0) scales[blockIdx.x] = s;
}

extern "C" int egomi_quantize_rows_fp8(const void* w, int64_t ldw, int N, int K, uint8_t* codes, int64_t ldc, float* scales, egomi_stream_t stream) {
    if (!w || !codes || !scales) return EGOMI_E_BADARG;
    if (N <= 0 || K <= 0 || ldw < K || ldc < K) return EGOMI_E_SHAPE;
    if (N > 0x7FFFFFFF) return EGOMI_E_UNSUPPORTED;
    EGOMI_LAUNCH(quantize_rows_fp8_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (long long)ldw, K, codes, (long long)ldc, scales);
    return egomi_launch_status();
}

// ------------------------------------------------------------------------------------------------
// gemm_w8
// ------------------------------------------------------------------------------------------------
// 8 codes -> 8 bf16 (exact)
__device__ __forceinline__ bf16x8 w8_decode8(uint32_t lo, uint32_t hi) {
    float f[8];
    e4m3fn_decode4(lo, f);
    e4m3fn_decode4(hi, f + 4);
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (__bf16)f[i];
    return r;
}

template <int MT>
__global__ __launch_bounds__(256) void wq_w8_kernel(WqArgs g) {
    __shared__ float red[4][WQ_BN][16 * MT + 1];
    const int item = (int)(blockIdx.x & 7) * g.per_xcd + (int)(blockIdx.x >> 3);    // dispatch round-robins XCDs: item-major per XCD
    if (item >= g.items) return;
    const int mc = item % g.mch, rest = item / g.mch;
    const int slice = rest % g.splitk, nt = rest / g.splitk;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nl = lane & 15, grp = lane >> 4;
    const int n0 = nt * WQ_BN, m0 = mc * 16 * MT;
    const int U = g.K >> 5, C = U >> 2;                                  // 32-deep units, whole 128-deep steps
    const int slot = slice * 4 + wave, nslots = g.splitk * 4;
    // slots own whole steps; the last one also takes the U % 4 single units
    const int u0 = 4 * (int)((long long)C * slot / nslots), u1 = slot + 1 == nslots ? U : 4 * (int)((long long)C * (slot + 1) / nslots);
    const uint8_t* wp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int r = n0 + 16 * j + nl;
        r = r < g.N ? r : g.N - 1;                                       // clamped rows are computed and never stored
        wp[j] = g.w + (long long)r * g.ldw;
    }
    const bf16_t* xp[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m0 + 16 * i + nl;
        m = m < g.M ? m : g.M - 1;
        xp[i] = g.x + (long long)m * g.ldx;
    }
    f32x4 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 wr[2][4][2];
    bf16x8 xr[2][MT][4];
    auto load = [&](int buf, int u) {
        const long long k0 = (long long)u * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wr[buf][j][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[j] + k0 + 16 * grp));
            wr[buf][j][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[j] + k0 + 64 + 16 * grp));
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            xr[buf][i][0] = *reinterpret_cast<const bf16x8*>(xp[i] + k0 + 16 * grp);
            xr[buf][i][1] = *reinterpret_cast<const bf16x8*>(xp[i] + k0 + 16 * grp + 8);
            xr[buf][i][2] = *reinterpret_cast<const bf16x8*>(xp[i] + k0 + 64 + 16 * grp);
            xr[buf][i][3] = *reinterpret_cast<const bf16x8*>(xp[i] + k0 + 64 + 16 * grp + 8);
        }
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const u32x4& c = wr[buf][j][p >> 1];
                const bf16x8 wf = w8_decode8(c[2 * (p & 1)], c[2 * (p & 1) + 1]);
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xr[buf][i][p], acc[i][j], 0, 0, 0);
            }
    };
    int u = u0;
    if (u + 4 <= u1) load(0, u);
    while (u + 4 <= u1) {
        if (u + 8 <= u1) load(1, u + 4);
        compute(0);
        u += 4;
        if (u + 4 <= u1) {
            if (u + 8 <= u1) load(0, u + 4);
            compute(1);
            u += 4;
        }
    }
    for (; u < u1; ++u) {                                                // K % 128 != 0: the last slot's 1-3 extra units, 8 elements per lane
        const long long k = (long long)u * 32 + 8 * grp;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x2 c = *reinterpret_cast<const u32x2*>(wp[j] + k);
            const bf16x8 wf = w8_decode8(c[0], c[1]);
#pragma unroll
            for (int i = 0; i < MT; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, *reinterpret_cast<const bf16x8*>(xp[i] + k), acc[i][j], 0, 0, 0);
        }
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
    float sc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sc[c] = g.s[n + c];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m0 + 16 * i + mr;
        if (m >= g.M) break;
        const int ml = 16 * i + mr;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (((red[0][n4 + c][ml] + red[1][n4 + c][ml]) + red[2][n4 + c][ml]) + red[3][n4 + c][ml]) * sc[c];
        if (g.ws) {                                                      // this K slice's slab [M, N] fp32
            *reinterpret_cast<f32x4*>(g.ws + ((long long)slice * g.M + m) * g.N + n) = (f32x4){v[0], v[1], v[2], v[3]};
            continue;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float y = g.res ? v[c] + bf2f(g.res[(long long)m * g.ldr + n + c]) : v[c];
            g.out[(long long)m * g.ldo + n + c] = f2bf(y);
        }
    }
}

struct W8Codec {
    static constexpr int CODES_PER_BYTE = 1;
    static constexpr uintptr_t SCALE_ALIGN_MASK = 0;                     // the scales are read one float at a time
    static constexpr auto kernel1 = &wq_w8_kernel<1>, kernel2 = &wq_w8_kernel<2>;
};

extern "C" int egomi_gemm_w8_slab_count(int M, int N, int K, int64_t workspace_bytes) { return wq_slab_count(M, N, K, workspace_bytes); }

extern "C" int egomi_gemm_w8(const void* x, int64_t ldx, const uint8_t* codes, int64_t ldw, const float* scales, void* out, int64_t ldo,
                             const void* residual, int64_t ldr, int M, int N, int K, int epilogue, void* workspace, int64_t workspace_bytes,
                             egomi_stream_t stream) {
    return wq_gemm<W8Codec>(x, ldx, codes, ldw, scales, out, ldo, residual, ldr, M, N, K, epilogue, workspace, workspace_bytes, stream);
}
