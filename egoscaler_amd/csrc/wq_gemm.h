// What the quantized decode-weight products (w8.hip: fp8 codes, w4.hip: int4 codes; y = x . dequantized(W)^T for M <= 512 rows) share:
// the arguments, the plan and the slab count read from it, the reduce kernel of a planned split, and the host entry with its checks.
// Each format keeps its whole kernel in its own file, epilogue included.  One templated kernel body over a per-format codec was built
// and gave the same bits, but no form of it compiled to the former instruction streams, and each measured 0.25-0.5 % slower at 8 rows;
// a shared epilogue function alone also changes the MT = 2 kernels.  So the sharing stops where the four kernels' code stays what it
// was (profiles/wq_frame_ab.txt).  A format supplies a codec:
//   CODES_PER_BYTE    a code row of K columns is K / CODES_PER_BYTE bytes
//   SCALE_ALIGN_MASK  alignment the kernel's scale loads need of the scales pointer
//   kernel1, kernel2  the format's kernel for MT = 1 (M <= 16) and MT = 2: void (*)(WqArgs)
#pragma once
#include "common.h"

#define WQ_BN 64

struct WqArgs {
    const bf16_t* x; const uint8_t* w; const float* s; bf16_t* out; const bf16_t* res; float* ws;
    long long ldx, ldw, ldo, ldr;
    int M, N, K;
    int splitk, mch, items, per_xcd;
};

// planned split of an EGOMI_EPI_NONE product: out = bf16(sum of the slabs in slice order (+ residual)).  static: one per including file.
static __global__ __launch_bounds__(256) void gemm_wq_reduce_kernel(WqArgs g) {
    const long long total = (long long)g.M * (g.N / 4);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int m = (int)(e / (g.N / 4)), n = (int)(e % (g.N / 4)) * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(g.ws + (long long)m * g.N + n);
        for (int s2 = 1; s2 < g.splitk; ++s2) v += *reinterpret_cast<const f32x4*>(g.ws + ((long long)s2 * g.M + m) * g.N + n);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float y = g.res ? v[k] + bf2f(g.res[(long long)m * g.ldr + n + k]) : v[k];
            g.out[(long long)m * g.ldo + n + k] = f2bf(y);
        }
    }
}

struct WqPlan { int mt, mch, tiles_n, splitk; };

// The one plan of a product, whatever its format: wq_slab_count and wq_gemm both read it, so the count a caller is told is the count
// the launch writes, and decode.Decoder may size one workspace for either format.  -> EGOMI_OK or EGOMI_E_UNSUPPORTED.
static int wq_plan(int M, int N, int K, int epilogue, int64_t ws_bytes, WqPlan& p) {
    if (M < 1 || M > 512 || N < 4 || (N & 3) || K < 32 || (K & 31)) return EGOMI_E_UNSUPPORTED;
    p.mt = M <= 16 ? 1 : 2;
    p.mch = (M + 16 * p.mt - 1) / (16 * p.mt);
    p.tiles_n = (N + WQ_BN - 1) / WQ_BN;
    const long long blocks = (long long)p.tiles_n * p.mch;
    // ~700 blocks of 4 waves (gemv_m16_kernel's measured sweet spot at M = 8), every wave at least one 128-deep step
    int sk = (int)((704 + blocks / 2) / blocks);
    const int sk_max = (K / 32) / 16;
    if (sk > sk_max) sk = sk_max;
    if (sk < 1) sk = 1;
    const long long per_slab = (long long)M * N * 4;
    if ((long long)sk * per_slab > ws_bytes) sk = (int)(ws_bytes / per_slab);
    if (epilogue == EGOMI_EPI_SLABS) {
        if (sk < 1) return EGOMI_E_UNSUPPORTED;                          // not even one slab fits the workspace
    } else if (sk < 2) {
        sk = 1;                                                          // no split: no workspace needed
    }
    if ((long long)p.tiles_n * sk * p.mch > 0x7FFFFFF8ll) return EGOMI_E_UNSUPPORTED;
    p.splitk = sk;
    return EGOMI_OK;
}

static int wq_slab_count(int M, int N, int K, int64_t workspace_bytes) {
    WqPlan p;
    return wq_plan(M, N, K, EGOMI_EPI_SLABS, workspace_bytes, p) == EGOMI_OK ? p.splitk : 0;
}

template <class Codec>
static int wq_gemm(const void* x, int64_t ldx, const uint8_t* codes, int64_t ldw, const float* scales, void* out, int64_t ldo, const void* residual,
                   int64_t ldr, int M, int N, int K, int epilogue, void* workspace, int64_t workspace_bytes, egomi_stream_t stream) {
    if (!x || !codes || !scales) return EGOMI_E_BADARG;
    if (epilogue != EGOMI_EPI_NONE && epilogue != EGOMI_EPI_SLABS) return EGOMI_E_UNSUPPORTED;
    if (epilogue == EGOMI_EPI_NONE && !out) return EGOMI_E_BADARG;
    if (epilogue == EGOMI_EPI_SLABS && (!workspace || residual)) return EGOMI_E_BADARG;
    if (M <= 0 || N <= 0 || K <= 0 || ldx < K || ldw < K / Codec::CODES_PER_BYTE || workspace_bytes < 0) return EGOMI_E_SHAPE;
    if (epilogue == EGOMI_EPI_NONE && (ldo < N || (residual && ldr < N))) return EGOMI_E_SHAPE;
    if (((uintptr_t)x & 15) || (ldx & 7) || ((uintptr_t)codes & 15) || (ldw & 15) || ((uintptr_t)scales & Codec::SCALE_ALIGN_MASK) ||
        ((uintptr_t)workspace & 15))
        return EGOMI_E_SHAPE;
    WqPlan p;
    if (const int rc = wq_plan(M, N, K, epilogue, workspace ? workspace_bytes : 0, p)) return rc;
    WqArgs g;
    g.x = (const bf16_t*)x; g.w = codes; g.s = scales; g.out = (bf16_t*)out; g.res = (const bf16_t*)residual;
    g.ws = (epilogue == EGOMI_EPI_SLABS || p.splitk > 1) ? (float*)workspace : nullptr;
    g.ldx = ldx; g.ldw = ldw; g.ldo = ldo; g.ldr = ldr;
    g.M = M; g.N = N; g.K = K;
    g.splitk = p.splitk; g.mch = p.mch;
    g.items = p.tiles_n * p.splitk * p.mch;
    g.per_xcd = (g.items + 7) / 8;
    hipStream_t st = (hipStream_t)stream;
    if (p.mt == 1) EGOMI_LAUNCH(Codec::kernel1, dim3(8 * g.per_xcd), dim3(256), 0, st, g);
    else EGOMI_LAUNCH(Codec::kernel2, dim3(8 * g.per_xcd), dim3(256), 0, st, g);
    if (epilogue == EGOMI_EPI_NONE && p.splitk > 1) {
        const long long total = (long long)M * (N / 4);
        const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        EGOMI_LAUNCH(gemm_wq_reduce_kernel, dim3(grid), dim3(256), 0, st, g);
    }
    return egomi_launch_status();
}
