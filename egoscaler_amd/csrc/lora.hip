// LoRA adapters on the decoder projections: the low-rank products of PEFT's lora.Linear.forward (peft/tuners/lora/layer.py,
// Linear.forward: result = base_layer(x) + lora_B(lora_A(dropout(x))) * scaling, scaling = lora_alpha / r; no dropout, no bias) and of
// its backward.  With A [r, K], B [N, r], s = lora_alpha / r, for one adapted projection y = x W^T + s (x A^T) B^T:
//   forward   T = x A^T                      (lora_down;  n adapters that share x in one pass over x: A stacked [n r, K])
//             y += s T B^T                   (lora_up, into the base product's output)
//   backward  U = dY B                       (lora_down with Q given transposed)
//             dX += s U A                    (lora_up with Q given transposed; the n adapters of one input in one pass)
//             dA = s U^T x,  dB = s dY^T T    (lora_wgrad into fp32 main_grad, overwrite or accumulate)
//   merge     W' = W + s B A                 (lora_up on W: one fp32 sum, rounded once to the model dtype)
//
// Numerics.  fp32 accumulation in a fixed order; no atomics, so a repeated call writes the same bits.  lora_wgrad reduces over M in
// fixed 256-row slices into an fp32 workspace and sums the slices in slice order.  lora_up rounds once: y = T(float(y) + alpha * acc).
//
// Column map `il` (the interleaved-32 layout of the stacked [Wgate;Wup] product, engine.stack_gate_up): logical column c of the wide
// activation operand lies at 64 * (c / 32) + c % 32 (the caller offsets the pointer by 32 for the up half).
//
// The products are skinny (r <= 64).  lora_down (the pass over every adapted input and output gradient) runs on bf16 MFMA where the shape
// allows (lora_down_mfma_kernel); lora_up, lora_wgrad and the other lora_down shapes (fp32, K % 32 != 0) are LDS-tiled fp32 FMA loops.
// Every global access is guarded by its logical bounds (MFMA rows past M are clamped and never stored); no LDS-DMA.
#include "common.h"

#define LORA_RMAX 192        // n * r of one lora_down / lora_up call: up to 3 adapters of r = 64
#define LORA_MSLICE 256      // lora_wgrad: rows per M slice
#define LORA_KSLICE 512      // lora_down: K per slice (fp32 partials summed in slice order)

__device__ __forceinline__ long long lora_col(int c, int il) { return il ? 64LL * (c >> 5) + (c & 31) : (long long)c; }

// ------------------------------------------------------------------------------------------------
// lora_down: Y[m, j] = alpha * sum_k X[m, col(k)] * Q(j, k), Q(j, k) = qt ? Q[k ldq + j] : Q[j ldq + k].  16 rows x all R x one
// 512-deep K slice per block (blockIdx.y); several slices write fp32 partials ws[slice][m][j], summed in slice order by lora_down_sum.
// LDS is sized by R at launch (the 16 x 64 x tile plus R x 65 of Q).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ X, long long ldx, const T* __restrict__ Q, long long ldq, int qt,
                                                        T* __restrict__ Y, long long ldy, float* __restrict__ ws, int M, int K, int R,
                                                        float alpha, int il) {
    extern __shared__ float lds[];
    float (*xs)[65] = reinterpret_cast<float (*)[65]>(lds);
    float (*qs)[65] = reinterpret_cast<float (*)[65]>(lds + 16 * 65);
    const int t = threadIdx.x, row = t & 15, j0 = t >> 4;
    const int m0 = blockIdx.x * 16;
    const int kb = blockIdx.y * LORA_KSLICE, ke = min(K, kb + LORA_KSLICE);
    float acc[LORA_RMAX / 16];
#pragma unroll
    for (int i = 0; i < LORA_RMAX / 16; ++i) acc[i] = 0.f;
    for (int k0 = kb; k0 < ke; k0 += 64) {
        for (int e = t; e < 16 * 64; e += 256) {
            const int r = e >> 6, c = e & 63, m = m0 + r, k = k0 + c;
            xs[r][c] = (m < M && k < ke) ? Cvt<T>::ld(X + (long long)m * ldx + lora_col(k, il)) : 0.f;
        }
        for (int e = t; e < R * 64; e += 256) {
            int j, c;
            if (qt) { c = e / R; j = e - c * R; } else { j = e >> 6; c = e & 63; }     // coalesced along Q's contiguous index
            const int k = k0 + c;
            qs[j][c] = k < ke ? Cvt<T>::ld(Q + (qt ? (long long)k * ldq + j : (long long)j * ldq + k)) : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < 64; ++c) {
            const float xv = xs[row][c];
#pragma unroll
            for (int i = 0; i < LORA_RMAX / 16; ++i)
                if (j0 + 16 * i < R) acc[i] += xv * qs[j0 + 16 * i][c];
        }
        __syncthreads();
    }
    const int m = m0 + row;
    if (m >= M) return;
    if (gridDim.y == 1) {
#pragma unroll
        for (int i = 0; i < LORA_RMAX / 16; ++i)
            if (j0 + 16 * i < R) Cvt<T>::st(Y + (long long)m * ldy + j0 + 16 * i, alpha * acc[i]);
        return;
    }
    float* w = ws + ((long long)blockIdx.y * M + m) * R;
#pragma unroll
    for (int i = 0; i < LORA_RMAX / 16; ++i)
        if (j0 + 16 * i < R) w[j0 + 16 * i] = acc[i];
}

// bf16 form on v_mfma_f32_16x16x32_bf16 (K % 32 == 0, 16-B aligned rows of x; what the engine issues): 4 waves x 16 rows = 64 rows x all
// R x one 512-deep K slice per block.  Per 32-deep step a lane reads 8 consecutive k of its row of x (one 16-B load; an 8-run never
// crosses a 32-column group, so the il map keeps it contiguous) and the same 8 k of row j = 16 jt + lane % 16 of Q for each 16-row tile
// jt of Q; the MFMA's D holds Y^T: row j = 16 jt + 4 (lane / 16) + v, column m = lane % 16.  Fixed order, same partial layout as above.
__global__ __launch_bounds__(256) void lora_down_mfma_kernel(const bf16_t* __restrict__ X, long long ldx, const bf16_t* __restrict__ Q,
                                                             long long ldq, int qt, bf16_t* __restrict__ Y, long long ldy, float* __restrict__ ws,
                                                             int M, int K, int R, float alpha, int il) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nl = lane & 15, grp = lane >> 4;
    const int m0 = blockIdx.x * 64 + wave * 16;
    const int kb = blockIdx.y * LORA_KSLICE, ke = min(K, kb + LORA_KSLICE);
    const int JT = (R + 15) >> 4;
    int mr = m0 + nl;
    mr = mr < M ? mr : M - 1;                                          // clamped rows are computed and never stored
    const bf16_t* xr = X + (long long)mr * ldx;
    f32x4 acc[LORA_RMAX / 16];
#pragma unroll
    for (int i = 0; i < LORA_RMAX / 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k0 = kb; k0 < ke; k0 += 32) {
        const int k = k0 + 8 * grp;
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xr + lora_col(k, il));
#pragma unroll
        for (int jt = 0; jt < LORA_RMAX / 16; ++jt) {
            if (jt >= JT) break;
            const int j = 16 * jt + nl;
            bf16x8 qf;
            if (j >= R) {
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[e] = (__bf16)0.f;
            } else if (!qt) {
                qf = *reinterpret_cast<const bf16x8*>(Q + (long long)j * ldq + k);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const bf16_t u = Q[(long long)(k + e) * ldq + j]; qf[e] = *reinterpret_cast<const __bf16*>(&u); }
            }
            acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, xf, acc[jt], 0, 0, 0);
        }
    }
    const int m = m0 + nl;
    if (m >= M) return;
#pragma unroll
    for (int jt = 0; jt < LORA_RMAX / 16; ++jt) {
        if (jt >= JT) break;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = 16 * jt + 4 * grp + v;
            if (j >= R) continue;
            if (gridDim.y == 1) Y[(long long)m * ldy + j] = f2bf(alpha * acc[jt][v]);
            else ws[((long long)blockIdx.y * M + m) * R + j] = acc[jt][v];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lora_down_sum_kernel(const float* __restrict__ ws, int slices, int M, int R, T* __restrict__ Y,
                                                            long long ldy, float alpha) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n = (long long)M * R;
    if (e >= n) return;
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += ws[(long long)z * n + e];
    const int m = (int)(e / R), j = (int)(e - (long long)m * R);
    Cvt<T>::st(Y + (long long)m * ldy + j, alpha * s);
}

// ------------------------------------------------------------------------------------------------
// lora_up: Y[m, col(n)] = T(float(Y) + alpha * sum_j P[m, j] * Q(n, j)), Q(n, j) = qt ? Q[j ldq + n] : Q[n ldq + j].  32 x 64 per block.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void lora_up_kernel(const T* __restrict__ P, long long ldp, const T* __restrict__ Q, long long ldq, int qt,
                                                      T* __restrict__ Y, long long ldy, int M, int N, int R, float alpha, int il) {
    extern __shared__ float lds[];                                   // ps [32][R + 1], qs [64][R + 1]: sized by R at launch
    const int Rp = R + 1;
    float* ps_ = lds;
    float* qs_ = lds + 32 * Rp;
#define ps(r, j) ps_[(r) * Rp + (j)]
#define qs(c, j) qs_[(c) * Rp + (j)]
    const int t = threadIdx.x, col = t & 63, r0 = t >> 6;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 64;
    for (int e = t; e < 32 * R; e += 256) {
        const int r = e / R, j = e - r * R, m = m0 + r;
        ps(r, j) = m < M ? Cvt<T>::ld(P + (long long)m * ldp + j) : 0.f;
    }
    for (int e = t; e < 64 * R; e += 256) {
        int c, j;
        if (qt) { j = e >> 6; c = e & 63; } else { c = e / R; j = e - c * R; }
        const int n = n0 + c;
        qs(c, j) = n < N ? Cvt<T>::ld(Q + (qt ? (long long)j * ldq + n : (long long)n * ldq + j)) : 0.f;
    }
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int j = 0; j < R; ++j) {
        const float q = qs(col, j);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += ps(r0 + 4 * i, j) * q;
    }
#undef ps
#undef qs
    const int n = n0 + col;
    if (n >= N) return;
    const long long cn = lora_col(n, il);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + r0 + 4 * i;
        if (m < M) {
            T* y = Y + (long long)m * ldy + cn;
            Cvt<T>::st(y, Cvt<T>::ld(y) + alpha * acc[i]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// lora_wgrad: G[p, q] (+)= alpha * sum_m L[m, colL(p)] * Rm[m, q].  64 x 64 outputs per block, one 256-row M slice per blockIdx.z;
// a slice's partial sums go to ws[z] (fp32 [slices, P, Q]) and lora_wgrad_sum adds the slices in slice order.  One slice: straight to G.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const T* __restrict__ L, long long ldl, const T* __restrict__ Rm, long long ldr,
                                                         float* __restrict__ out, long long ldo, int M, int Pd, int Qd, float alpha,
                                                         int accumulate, int il) {
    __shared__ float ls[16][64];
    __shared__ float rs[16][64];
    const int t = threadIdx.x, pb = (t >> 4) * 4, qb = (t & 15) * 4;
    const int p0 = blockIdx.y * 64, q0 = blockIdx.x * 64;
    const int mb = blockIdx.z * LORA_MSLICE, me = min(M, mb + LORA_MSLICE);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int m0 = mb; m0 < me; m0 += 16) {
        for (int e = t; e < 16 * 64; e += 256) {
            const int r = e >> 6, c = e & 63, m = m0 + r;
            ls[r][c] = (m < me && p0 + c < Pd) ? Cvt<T>::ld(L + (long long)m * ldl + lora_col(p0 + c, il)) : 0.f;
            rs[r][c] = (m < me && q0 + c < Qd) ? Cvt<T>::ld(Rm + (long long)m * ldr + q0 + c) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = ls[r][pb + i]; b[i] = rs[r][qb + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
        }
        __syncthreads();
    }
    float* o = out + (long long)blockIdx.z * Pd * Qd;            // slice partials (ldo ignored), or G itself when gridDim.z == 1
    const bool direct = gridDim.z == 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + pb + i;
        if (p >= Pd) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = q0 + qb + j;
            if (q >= Qd) continue;
            if (direct) {
                float* g = out + (long long)p * ldo + q;
                *g = (accumulate ? *g : 0.f) + alpha * acc[i][j];
            } else {
                o[(long long)p * Qd + q] = acc[i][j];
            }
        }
    }
}

__global__ __launch_bounds__(256) void lora_wgrad_sum_kernel(const float* __restrict__ ws, int slices, int Pd, int Qd, float* __restrict__ G,
                                                             long long ldg, float alpha, int accumulate) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n = (long long)Pd * Qd;
    if (e >= n) return;
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += ws[(long long)z * n + e];
    const int p = (int)(e / Qd), q = (int)(e - (long long)p * Qd);
    float* g = G + (long long)p * ldg + q;
    *g = (accumulate ? *g : 0.f) + alpha * s;
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
static bool lora_r_ok(int R) { return R >= 8 && R <= LORA_RMAX && R % 8 == 0; }

extern "C" int64_t egomi_lora_down_workspace_bytes(int M, int K, int R) {
    const int slices = (K + LORA_KSLICE - 1) / LORA_KSLICE;
    return slices > 1 ? (int64_t)slices * M * R * 4 : 0;
}

extern "C" int egomi_lora_down(const void* x, int64_t ldx, const void* q, int64_t ldq, int q_trans, void* y, int64_t ldy, int M, int K,
                               int R, float alpha, int il, void* workspace, int64_t workspace_bytes, int dtype, egomi_stream_t stream) {
    if (!x || !q || !y) return EGOMI_E_BADARG;
    if (M <= 0 || K <= 0 || R <= 0) return EGOMI_E_SHAPE;
    if (!lora_r_ok(R) || (il && K % 32) || (dtype != EGOMI_F32 && dtype != EGOMI_BF16)) return EGOMI_E_UNSUPPORTED;
    if (ldy < R || ldx < (il ? 2LL * K - 32 : (long long)K) || ldq < (q_trans ? R : K)) return EGOMI_E_SHAPE;
    const int slices = (K + LORA_KSLICE - 1) / LORA_KSLICE;
    const int64_t need = egomi_lora_down_workspace_bytes(M, K, R);
    if (need > 0 && (!workspace || workspace_bytes < need)) return EGOMI_E_SHAPE;
    const bool a16 = ((uintptr_t)x & 15) == 0 && ldx % 8 == 0 && (q_trans || (((uintptr_t)q & 15) == 0 && ldq % 8 == 0));
    if (dtype == EGOMI_BF16 && K % 32 == 0 && a16) {
        EGOMI_LAUNCH(lora_down_mfma_kernel, dim3((M + 63) / 64, slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (long long)ldx,
                     (const bf16_t*)q, (long long)ldq, q_trans, (bf16_t*)y, (long long)ldy, (float*)workspace, M, K, R, alpha, il);
    } else {
        const size_t lds = (size_t)(16 + R) * 65 * sizeof(float);
        EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(lora_down_kernel<T>, dim3((M + 15) / 16, slices), dim3(256), lds, (hipStream_t)stream,
                                                 (const T*)x, (long long)ldx, (const T*)q, (long long)ldq, q_trans, (T*)y, (long long)ldy,
                                                 (float*)workspace, M, K, R, alpha, il));
    }
    if (need > 0) {
        const long long n = (long long)M * R;
        EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(lora_down_sum_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                                 (const float*)workspace, slices, M, R, (T*)y, (long long)ldy, alpha));
    }
    return egomi_launch_status();
}

extern "C" int egomi_lora_up(const void* p, int64_t ldp, const void* q, int64_t ldq, int q_trans, void* y, int64_t ldy, int M, int N, int R,
                             float alpha, int il, int dtype, egomi_stream_t stream) {
    if (!p || !q || !y) return EGOMI_E_BADARG;
    if (M <= 0 || N <= 0 || R <= 0) return EGOMI_E_SHAPE;
    if (!lora_r_ok(R) || (il && N % 32) || (dtype != EGOMI_F32 && dtype != EGOMI_BF16) || M > 65535 * 32) return EGOMI_E_UNSUPPORTED;
    if (ldp < R || ldy < (il ? 2LL * N - 32 : (long long)N) || ldq < (q_trans ? N : R)) return EGOMI_E_SHAPE;
    const size_t lds = (size_t)(32 + 64) * (R + 1) * sizeof(float);     // > 64 KiB from R = 171 on (dX of three adapters of r = 64)
    EGOMI_DISPATCH_DTYPE(dtype, (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lora_up_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                          (int)lds));
    EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(lora_up_kernel<T>, dim3((N + 63) / 64, (M + 31) / 32), dim3(256), lds, (hipStream_t)stream,
                                             (const T*)p, (long long)ldp, (const T*)q, (long long)ldq, q_trans, (T*)y, (long long)ldy, M, N, R,
                                             alpha, il));
    return egomi_launch_status();
}

extern "C" int64_t egomi_lora_wgrad_workspace_bytes(int M, int P, int Q) {
    const int slices = (M + LORA_MSLICE - 1) / LORA_MSLICE;
    return slices > 1 ? (int64_t)slices * P * Q * 4 : 0;
}

extern "C" int egomi_lora_wgrad(const void* l, int64_t ldl, const void* r, int64_t ldr, float* g, int64_t ldg, int M, int P, int Q,
                                float alpha, int accumulate, int il, void* workspace, int64_t workspace_bytes, int dtype,
                                egomi_stream_t stream) {
    if (!l || !r || !g) return EGOMI_E_BADARG;
    if (M <= 0 || P <= 0 || Q <= 0 || ldg < Q || ldr < Q) return EGOMI_E_SHAPE;
    if ((P > LORA_RMAX && Q > LORA_RMAX) || (il && P % 32) || (dtype != EGOMI_F32 && dtype != EGOMI_BF16)) return EGOMI_E_UNSUPPORTED;
    if (ldl < (il ? 2LL * P - 32 : (long long)P)) return EGOMI_E_SHAPE;
    const int slices = (M + LORA_MSLICE - 1) / LORA_MSLICE;
    const int64_t need = egomi_lora_wgrad_workspace_bytes(M, P, Q);
    if (slices > 65535 || (P + 63) / 64 > 65535) return EGOMI_E_UNSUPPORTED;
    if (need > 0 && (!workspace || workspace_bytes < need)) return EGOMI_E_SHAPE;
    float* out = need > 0 ? (float*)workspace : g;
    EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH(lora_wgrad_kernel<T>, dim3((Q + 63) / 64, (P + 63) / 64, slices), dim3(256), 0,
                                             (hipStream_t)stream, (const T*)l, (long long)ldl, (const T*)r, (long long)ldr, out,
                                             (long long)ldg, M, P, Q, alpha, accumulate, il));
    if (need > 0) {
        const long long n = (long long)P * Q;
        EGOMI_LAUNCH(lora_wgrad_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace,
                     slices, P, Q, g, (long long)ldg, alpha, accumulate);
    }
    return egomi_launch_status();
}
