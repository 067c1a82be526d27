// Global gradient norm on the device (include/egomi.h "gradient-norm clipping"): the float64 sum of squares of a table of gradient
// tensors in two launches and no atomics, and the one-thread kernel that turns it into the clipping coefficient.
// gfx950 only.
#include "common.h"
#include <math.h>

// elements per stage-1 workgroup: a compile-time constant and a function of nothing else, so that a segment's partials (and with them its
// bits) depend on its element count alone.  A multiple of 8, so every chunk of a 16-B aligned segment starts 16-B aligned.
static constexpr long long GN_CHUNK = 32768;
static constexpr int GN_T = 256;

__host__ __device__ __forceinline__ long long gn_chunks_of(long long numel) { return numel > 0 ? (numel - 1) / GN_CHUNK + 1 : 0; }

// inclusive scan of one int64 per thread over a block of NT threads (Hillis-Steele on two LDS rows); buf holds 2*NT values.
// Ends with a barrier, so buf may be reused at once.
template <int NT> __device__ __forceinline__ long long gn_block_scan(long long v, long long* buf) {
    const int t = threadIdx.x;
    int src = 0;
    buf[t] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
        long long x = buf[src * NT + t];
        if (t >= o) x += buf[src * NT + t - o];
        buf[(src ^ 1) * NT + t] = x;
        __syncthreads();
        src ^= 1;
    }
    const long long r = buf[src * NT + t];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void gn_acc(double& acc, float f) {
#pragma clang fp contract(off)
    const double d = (double)f;          // (the square of a widened fp32 / bf16 value is exact in float64; only the sum rounds)
    acc += d * d;
}

// One chunk of one segment: x points at the chunk, len <= GN_CHUNK elements.  Element e belongs to lane (e / V) % 256, V = the elements of
// one 16-B vector, and a lane adds its elements in ascending order: VEC = false (a segment that is not 16-B aligned) takes the same
// elements in the same order with 4-B / 2-B loads, as adamw_kernel / adamw_vec4_kernel split their work.  No load reaches past x + len.
template <typename G, bool VEC> __device__ __forceinline__ double gn_chunk_sumsq(const G* x, long long len) {
    constexpr int V = 16 / (int)sizeof(G);
    const long long nvec = len / V;
    double acc = 0.0;
#pragma unroll 4
    for (long long i = threadIdx.x; i * V < len; i += GN_T) {
        if (VEC && i < nvec) {
            const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x) + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (sizeof(G) == 4) gn_acc(acc, __uint_as_float(r[j]));
                else { gn_acc(acc, __uint_as_float(r[j] << 16)); gn_acc(acc, __uint_as_float(r[j] & 0xFFFF0000u)); }
            }
        } else {
            for (int j = 0; j < V; ++j) {
                const long long e = i * V + j;
                if (e < len) gn_acc(acc, Cvt<G>::ld(x + e));
            }
        }
    }
    return acc;
}

__device__ __forceinline__ double gn_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Stage 1: workgroup c handles chunk c of the table (chunks numbered segment by segment).  Which segment that is follows from the element
// counts, which are device data: the block scans them itself (a slice per thread, one block scan, the owning thread walks its slice).
__global__ __launch_bounds__(GN_T) void grad_sumsq_chunk_kernel(const int64_t* __restrict__ seg_addr, const int64_t* __restrict__ seg_numel,
                                                                const int32_t* __restrict__ seg_dtype, int dtype, int n_seg,
                                                                double* __restrict__ partial) {
    __shared__ long long scan[2 * GN_T];
    __shared__ long long s_first;
    __shared__ int s_seg;
    __shared__ double red[GN_T / 64];
    const int t = threadIdx.x;
    const long long c = blockIdx.x;
    const long long per = ((long long)n_seg + GN_T - 1) / GN_T;
    const long long lo = min(t * per, (long long)n_seg), hi = min(lo + per, (long long)n_seg);
    long long mine = 0;
    for (long long s = lo; s < hi; ++s) mine += gn_chunks_of(seg_numel[s]);
    if (t == 0) s_seg = -1;
    const long long incl = gn_block_scan<GN_T>(mine, scan);
    if (incl - mine <= c && c < incl) {
        long long b = incl - mine;
        for (long long s = lo; s < hi; ++s) {
            const long long nc = gn_chunks_of(seg_numel[s]);
            if (c < b + nc) { s_seg = (int)s; s_first = b; break; }
            b += nc;
        }
    }
    __syncthreads();
    const int seg = s_seg;
    if (seg < 0) return;                                   // the caller's n_chunks exceeds the table's: nothing to do here
    const long long base = (c - s_first) * GN_CHUNK;
    const long long len = min(GN_CHUNK, (long long)seg_numel[seg] - base);
    const int dt = seg_dtype ? seg_dtype[seg] : dtype;
    const uintptr_t a = (uintptr_t)seg_addr[seg];
    double acc;
    if (dt == EGOMI_F32) {
        const float* x = reinterpret_cast<const float*>(a) + base;
        acc = (a & 15) == 0 ? gn_chunk_sumsq<float, true>(x, len) : gn_chunk_sumsq<float, false>(x, len);
    } else if (dt == EGOMI_BF16) {
        const bf16_t* x = reinterpret_cast<const bf16_t*>(a) + base;
        acc = (a & 15) == 0 ? gn_chunk_sumsq<bf16_t, true>(x, len) : gn_chunk_sumsq<bf16_t, false>(x, len);
    } else {
        acc = __builtin_nan("");                           // a dtype the table may not hold: nothing is read, the segment reports NaN
    }
    acc = gn_wave_sum(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) partial[c] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Stage 2, one workgroup: where each segment's partials start (the same scan, kept in the workspace), then one wave per segment —
// lane l adds partials l, l + 64, ... in ascending order, then the fixed xor tree — and last the segments, thread t adding segments
// t, t + 1024, ... in ascending order, a fixed tree per wave and the 16 waves in order.  A segment's bits depend on its number of
// partials and their values only.  A table that needs more chunks than the caller launched reports NaN instead of reading unwritten partials.
__global__ __launch_bounds__(1024) void grad_sumsq_finish_kernel(const int64_t* __restrict__ seg_numel, int n_seg, long long n_chunks,
                                                                 const double* __restrict__ partial, long long* __restrict__ seg_start,
                                                                 double* __restrict__ seg_sumsq, double* __restrict__ total_sumsq) {
    __shared__ long long scan[2 * 1024];
    __shared__ double red[16];
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const long long per = ((long long)n_seg + 1023) / 1024;
    const long long lo = min(t * per, (long long)n_seg), hi = min(lo + per, (long long)n_seg);
    long long mine = 0;
    for (long long s = lo; s < hi; ++s) mine += gn_chunks_of(seg_numel[s]);
    long long b = gn_block_scan<1024>(mine, scan) - mine;
    for (long long s = lo; s < hi; ++s) {
        seg_start[s] = b;
        b += gn_chunks_of(seg_numel[s]);
    }
    __syncthreads();
    for (long long s = w; s < n_seg; s += 16) {
        const long long st = seg_start[s], nc = gn_chunks_of(seg_numel[s]);
        double acc = 0.0;
        if (st + nc > n_chunks) acc = __builtin_nan("");
        else
            for (long long i = l; i < nc; i += 64) acc += partial[st + i];
        acc = gn_wave_sum(acc);
        if (l == 0) seg_sumsq[s] = acc;
    }
    __syncthreads();
    double acc = 0.0;
    for (long long s = t; s < n_seg; s += 1024) acc += seg_sumsq[s];
    acc = gn_wave_sum(acc);
    if (l == 0) red[w] = acc;
    __syncthreads();
    if (t == 0) {
        double tot = red[0];
        for (int i = 1; i < 16; ++i) tot += red[i];
        *total_sumsq = tot;
    }
}

extern "C" int64_t egomi_grad_sumsq_chunk(void) { return GN_CHUNK; }

extern "C" size_t egomi_grad_sumsq_workspace_bytes(int n_seg, int64_t n_chunks) {
    if (n_seg <= 0 || n_chunks <= 0) return 0;
    return ((size_t)n_chunks + (size_t)n_seg) * 8;          // one float64 partial per chunk, one int64 first-chunk index per segment
}

extern "C" int egomi_grad_sumsq(const int64_t* seg_addr, const int64_t* seg_numel, const int32_t* seg_dtype, int dtype, int n_seg,
                                int64_t n_chunks, double* seg_sumsq, double* total_sumsq, void* workspace, size_t workspace_bytes,
                                egomi_stream_t stream) {
    if (!seg_addr || !seg_numel || !seg_sumsq || !total_sumsq || !workspace) return EGOMI_E_BADARG;
    if (dtype != EGOMI_F32 && dtype != EGOMI_BF16) return EGOMI_E_UNSUPPORTED;
    if (n_seg <= 0 || n_chunks < n_seg || n_chunks > 0x7fffffffLL || ((uintptr_t)workspace & 7)) return EGOMI_E_SHAPE;
    if (workspace_bytes < egomi_grad_sumsq_workspace_bytes(n_seg, n_chunks)) return EGOMI_E_SHAPE;
    double* partial = (double*)workspace;
    long long* seg_start = (long long*)(partial + n_chunks);
    EGOMI_LAUNCH(grad_sumsq_chunk_kernel, dim3((unsigned)n_chunks), dim3(GN_T), 0, (hipStream_t)stream, seg_addr, seg_numel, seg_dtype, dtype,
                 n_seg, partial);
    EGOMI_LAUNCH(grad_sumsq_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, seg_numel, n_seg, (long long)n_chunks,
                 (const double*)partial, seg_start, seg_sumsq, total_sumsq);
    return egomi_launch_status();
}

// total_norm, coefficient and effective gradient scale of one step; see the header for the formulas.  One thread, float64.
__global__ void clip_scale_kernel(const double* __restrict__ total_sumsq, float grad_scale, float max_norm, float* __restrict__ out,
                                  double* __restrict__ stats) {
#pragma clang fp contract(off)
    const double norm = (double)grad_scale * sqrt(*total_sumsq);
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;                            // (a NaN stays a NaN, as torch.clamp leaves it)
    const float norm_f = (float)norm;
    out[0] = norm_f;
    out[1] = (float)coef;
    out[2] = coef >= 1.0 ? grad_scale : (float)((double)grad_scale * coef);
    const bool finite = isfinite(norm_f);
    stats[0] += 1.0;
    if (finite && coef < 1.0) stats[1] += 1.0;
    if (!finite) stats[2] += 1.0;
    else {
        stats[3] += (double)norm_f;
        if ((double)norm_f > stats[4]) stats[4] = (double)norm_f;
    }
}

extern "C" int egomi_clip_scale(const double* total_sumsq, float grad_scale, float max_norm, float* out, double* stats,
                                egomi_stream_t stream) {
    if (!total_sumsq || !out || !stats || !(max_norm > 0.0f)) return EGOMI_E_BADARG;
    EGOMI_LAUNCH(clip_scale_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, total_sumsq, grad_scale, max_norm, out, stats);
    return egomi_launch_status();
}
