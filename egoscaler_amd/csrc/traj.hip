// A14 on the device: trajectory <-> token ids for whole batches, and displacement metrics.
// replaces (integer contracts, bit-exact):
//   models/pointllm/utils/utils.py:13-16  discretize_action   np.digitize(v, linspace(-1,1,nb)) - 1
//   models/pointllm/utils/utils.py:18-21  token_to_action     linspace[idx]
//   models/pointllm/utils/utils.py:47-104 str_to_float (rt2, 6-DoF): split on <tsep>, first run of six
//       <p*> tokens per segment, unmatched segments repeat the previous step
//   models/pointllm/dataset.py:16-19,150-194 sequence layout  <ts> (p*6 <tsep>)*T <te> eos pad...
//   models/utils/metrics.py:7-55          ADE / FDE (documented [T,D] form); best-of-K minima of them (minADE_K / minFDE_K); the medoid of
//       K samples under the same displacement (metrics.py:38-55 between two samples instead of a sample and the ground truth)
// The bin edges are computed once on the host in float64 exactly as numpy.linspace does and passed in.
#include "common.h"
#include "traj_disp.h"
#include <math.h>

// ids[b, :] = <ts> (p p p p p p <tsep>) x steps[b] <te> <eos> pad...   ; mask = 1 on non-pad
__global__ __launch_bounds__(256) void traj_tokenize_kernel(const float* traj, const int32_t* steps, int Tmax, const double* bins, int nb,
                                                            int64_t p0, int64_t ts, int64_t tsep, int64_t te, int64_t eos, int64_t pad,
                                                            int L, int64_t* ids, uint8_t* mask, int32_t* err) {
    const int b = blockIdx.x;
    int T = steps ? steps[b] : Tmax;
    T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
    const int need = 1 + 7 * T + 2;
    if (need > L) { if (threadIdx.x == 0) err[b] = 1; T = (L - 3) / 7; }
    else if (threadIdx.x == 0) err[b] = 0;
    const int real = 1 + 7 * T + 2;
    for (int j = threadIdx.x; j < L; j += 256) {
        int64_t t;
        if (j == 0) t = ts;
        else if (j < 1 + 7 * T) {
            const int s = (j - 1) / 7, c = (j - 1) % 7;
            if (c == 6) t = tsep;
            else {
                const double v = (double)traj[((long long)b * Tmax + s) * 6 + c];
                // np.digitize(v, bins) = number of edges <= v  (bins increasing, right=False); NaN -> nb
                int lo = 0, hi = nb;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (bins[mid] <= v) lo = mid + 1; else hi = mid; }
                int bin = (v != v) ? nb : lo;
                bin -= 1;                                                   // utils.py:15
                bin = bin < 0 ? 0 : (bin > nb - 1 ? nb - 1 : bin);          // keep the id inside <p0..p{nb-1}>
                t = p0 + bin;
            }
        } else if (j == 1 + 7 * T) t = te;
        else if (j == 2 + 7 * T) t = eos;
        else t = pad;
        ids[(long long)b * L + j] = t;
        mask[(long long)b * L + j] = j < real;
    }
}

// The scan of one row of ids, a bit-exact restatement of str_to_float (rt2, 6-DoF): cut at the first eos (train.py:241-242), split on
// <tsep>, per segment the first run of six consecutive <p*> ids (the regex of utils.py:52-57); a segment without one repeats the previous
// step once there is one (utils.py:88-90).  parse(hit): a step was parsed at ids hit .. hit+5; emit(n): step n goes out, as parsed last.
// Returns the number of steps (<= Tmax).  Both detokenize kernels are this scan: their n_steps cannot differ.
template <typename Parse, typename Emit>
__device__ __forceinline__ int traj_scan(const int64_t* r, int L, int nb, int64_t p0, int64_t tsep, int64_t eos, int Tmax, Parse parse, Emit emit) {
    int n = 0, end = L;
    for (int j = 0; j < L; ++j) if (r[j] == eos) { end = j; break; }
    int seg0 = 0;
    bool have_last = false;
    while (seg0 <= end && n < Tmax) {
        int seg1 = seg0;
        while (seg1 < end && r[seg1] != tsep) ++seg1;                       // segment [seg0, seg1)
        int run = 0, hit = -1;
        for (int j = seg0; j < seg1; ++j) {
            if (r[j] >= p0 && r[j] < p0 + nb) { if (++run == 6) { hit = j - 5; break; } } else run = 0;
        }
        if (hit >= 0) { parse(hit); have_last = true; }
        if (have_last) { emit(n); ++n; }
        if (seg1 >= end) break;
        seg0 = seg1 + 1;
    }
    return n;
}

// one thread per sample: values[b, step, 6] (bin centres linspace[idx]) and n_steps[b]
__global__ __launch_bounds__(64) void traj_detokenize_kernel(const int64_t* ids, int B, int L, const double* bins, int nb, int64_t p0, int64_t tsep,
                                                             int64_t eos, int Tmax, float* out, int32_t* n_steps) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t* r = ids + (long long)b * L;
    float last[6];
    n_steps[b] = traj_scan(r, L, nb, p0, tsep, eos, Tmax,
        [&](int hit) { for (int c = 0; c < 6; ++c) last[c] = (float)bins[(int)(r[hit + c] - p0)]; },
        [&](int n) { for (int c = 0; c < 6; ++c) out[((long long)b * Tmax + n) * 6 + c] = last[c]; });
}

// the same scan, gathering the per-token statistics of egomi_bin_stats instead of bin centres: a step parsed from ids hit .. hit+5 takes
// mean / std of columns hit .. hit+5 and, with bin_mass, the smallest of their six masses; a copied step repeats all three.
__global__ __launch_bounds__(64) void traj_detokenize_soft_kernel(const int64_t* ids, int B, int L, int nb, int64_t p0, int64_t tsep, int64_t eos,
                                                                  const float* bin_mean, const float* bin_std, const float* bin_mass,
                                                                  long long ld_stat, int Tmax, float* mean, float* std, float* mass,
                                                                  int32_t* n_steps) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const long long sr = (long long)b * ld_stat;
    float lm[6], ls[6], lmass = 0.f;
    n_steps[b] = traj_scan(ids + (long long)b * L, L, nb, p0, tsep, eos, Tmax,
        [&](int hit) {
            for (int c = 0; c < 6; ++c) { lm[c] = bin_mean[sr + hit + c]; ls[c] = bin_std[sr + hit + c]; }
            if (bin_mass) {
                lmass = bin_mass[sr + hit];
                for (int c = 1; c < 6; ++c) { const float x = bin_mass[sr + hit + c]; lmass = (x < lmass || x != x) ? x : lmass; }   // a NaN mass wins
            }
        },
        [&](int n) {
            for (int c = 0; c < 6; ++c) {
                mean[((long long)b * Tmax + n) * 6 + c] = lm[c];
                std[((long long)b * Tmax + n) * 6 + c] = ls[c];
            }
            if (mass) mass[(long long)b * Tmax + n] = lmass;
        });
}

// per sample: ADE / FDE of gen against gt (traj_disp.h: traj_ade_fde, float64 like numpy); NaN when either holds no step
__global__ __launch_bounds__(64) void traj_metrics_kernel(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int Tmax,
                                                          int D, double* ade, double* fde) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int ng = traj_len(n_gen, b, Tmax), nt = traj_len(n_gt, b, Tmax);
    if (ng <= 0 || nt <= 0) { ade[b] = NAN; fde[b] = NAN; return; }
    traj_ade_fde(gt + (long long)b * Tmax * D, nt, gen + (long long)b * Tmax * D, ng, D, ade[b], fde[b]);
}

// best of K: gen [B, K, Tmax, D], n_gen [B, K]; per clip the minimum ADE and the minimum FDE over the samples with n_gen > 0 (each
// computed as traj_metrics_kernel does), best = arg-min ADE (lowest index on ties); no such sample: NaN, NaN, -1
__global__ __launch_bounds__(64) void traj_metrics_min_kernel(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int K,
                                                              int Tmax, int D, double* min_ade, double* min_fde, int32_t* best) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int nt = traj_len(n_gt, b, Tmax);
    double ba = NAN, bf = NAN;
    int bi = -1;
    for (int j = 0; j < K && nt > 0; ++j) {
        const int ng = traj_len(n_gen, (long long)b * K + j, Tmax);
        if (ng <= 0) continue;
        double ade, fde;
        traj_ade_fde(gt + (long long)b * Tmax * D, nt, gen + ((long long)b * K + j) * Tmax * D, ng, D, ade, fde);
        if (bi < 0 || ade < ba) { ba = ade; bi = j; }
        if (!(bf <= fde)) bf = fde;                                        // first sample (bf NaN) or a smaller FDE
    }
    min_ade[b] = ba;
    min_fde[b] = bf;
    best[b] = bi;
}

// medoid of K: gen [B, K, Tmax, D], n_gen [B, K] or NULL (= Tmax); sample j is valid when n_gen > 0 (traj_metrics_min_kernel's rule).
// cost[b, j] = mean of d(j, i) (traj_disp.h: traj_pair_dist, traj_modes_kernel's matrix) over the valid i != j, float64, summed in index
// order; one valid sample: 0; invalid j: NaN.  pick[b] = arg-min of cost over the valid samples (lowest index on ties), none: -1.
// One workgroup per clip, one thread per sample j.
#define MED_THREADS 256
#define MED_MAXK 1024
__global__ __launch_bounds__(MED_THREADS) void traj_medoid_kernel(const float* gen, const int32_t* n_gen, int K, int Tmax, int D, double* cost,
                                                                  int32_t* pick) {
    __shared__ double cs[MED_MAXK];
    const int b = blockIdx.x;
    const float* gb = gen + (long long)b * K * Tmax * D;
    for (int j = threadIdx.x; j < K; j += MED_THREADS) {
        const int nj = traj_len(n_gen, (long long)b * K + j, Tmax);
        double c = NAN;
        if (nj > 0) {
            double tot = 0.0;
            int others = 0;
            for (int i = 0; i < K; ++i) {
                const int ni = traj_len(n_gen, (long long)b * K + i, Tmax);
                if (i == j || ni <= 0) continue;
                tot += traj_pair_dist(gb + (long long)j * Tmax * D, nj, gb + (long long)i * Tmax * D, ni, D);
                ++others;
            }
            c = others ? tot / others : 0.0;
        }
        cs[j] = c;
        cost[(long long)b * K + j] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int bi = -1;
        double bc = 0.0;
        for (int j = 0; j < K; ++j) {
            const double c = cs[j];
            if (c != c) continue;                                            // invalid sample
            if (bi < 0 || c < bc) { bc = c; bi = j; }
        }
        pick[b] = bi;
    }
}

extern "C" int egomi_traj_tokenize(const float* traj, const int32_t* steps, int B, int Tmax, const double* bins, int num_bins, int64_t p0,
                                   int64_t ts, int64_t tsep, int64_t te, int64_t eos, int64_t pad, int L, int64_t* ids, uint8_t* mask,
                                   int32_t* err, egomi_stream_t stream) {
    if (!traj || !bins || !ids || !mask || !err) return EGOMI_E_BADARG;
    if (B <= 0 || Tmax <= 0 || num_bins <= 1 || L < 3) return EGOMI_E_SHAPE;
    EGOMI_LAUNCH(traj_tokenize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, traj, steps, Tmax, bins, num_bins, p0, ts, tsep, te, eos, pad, L, ids, mask, err);
    return egomi_launch_status();
}

extern "C" int egomi_traj_detokenize(const int64_t* ids, int B, int L, const double* bins, int num_bins, int64_t p0, int64_t tsep, int64_t eos,
                                     int Tmax, float* out, int32_t* n_steps, egomi_stream_t stream) {
    if (!ids || !bins || !out || !n_steps) return EGOMI_E_BADARG;
    if (B <= 0 || L <= 0 || Tmax <= 0 || num_bins <= 1) return EGOMI_E_SHAPE;
    EGOMI_LAUNCH(traj_detokenize_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, ids, B, L, bins, num_bins, p0, tsep, eos, Tmax, out, n_steps);
    return egomi_launch_status();
}

extern "C" int egomi_traj_detokenize_soft(const int64_t* ids, int B, int L, int num_bins, int64_t p0, int64_t tsep, int64_t eos,
                                          const float* bin_mean, const float* bin_std, const float* bin_mass, int64_t ld_stat, int Tmax,
                                          float* mean, float* std, float* mass, int32_t* n_steps, egomi_stream_t stream) {
    if (!ids || !bin_mean || !bin_std || !mean || !std || !n_steps || (bin_mass != nullptr) != (mass != nullptr)) return EGOMI_E_BADARG;
    if (B <= 0 || L <= 0 || Tmax <= 0 || num_bins <= 1 || ld_stat < L) return EGOMI_E_SHAPE;
    EGOMI_LAUNCH(traj_detokenize_soft_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, ids, B, L, num_bins, p0, tsep, eos, bin_mean,
                 bin_std, bin_mass, (long long)ld_stat, Tmax, mean, std, mass, n_steps);
    return egomi_launch_status();
}

extern "C" int egomi_traj_metrics(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int Tmax, int D, double* ade,
                                  double* fde, egomi_stream_t stream) {
    if (!gen || !gt || !ade || !fde) return EGOMI_E_BADARG;
    if (B <= 0 || Tmax <= 0 || D <= 0) return EGOMI_E_SHAPE;
    EGOMI_LAUNCH(traj_metrics_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, gen, n_gen, gt, n_gt, B, Tmax, D, ade, fde);
    return egomi_launch_status();
}

extern "C" int egomi_traj_metrics_min(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int K, int Tmax, int D,
                                      double* min_ade, double* min_fde, int32_t* best, egomi_stream_t stream) {
    if (!gen || !gt || !min_ade || !min_fde || !best) return EGOMI_E_BADARG;
    if (B <= 0 || K <= 0 || Tmax <= 0 || D <= 0) return EGOMI_E_SHAPE;
    EGOMI_LAUNCH(traj_metrics_min_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, gen, n_gen, gt, n_gt, B, K, Tmax, D, min_ade,
                 min_fde, best);
    return egomi_launch_status();
}

extern "C" int egomi_traj_medoid(const float* gen, const int32_t* n_gen, int B, int K, int Tmax, int D, double* cost, int32_t* pick,
                                 egomi_stream_t stream) {
    if (!gen || !cost || !pick) return EGOMI_E_BADARG;
    if (B <= 0 || K <= 0 || Tmax <= 0 || D <= 0) return EGOMI_E_SHAPE;
    if (K > MED_MAXK) return EGOMI_E_UNSUPPORTED;
    EGOMI_LAUNCH(traj_medoid_kernel, dim3(B), dim3(MED_THREADS), 0, (hipStream_t)stream, gen, n_gen, K, Tmax, D, cost, pick);
    return egomi_launch_status();
}
