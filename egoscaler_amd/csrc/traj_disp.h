// The displacement arithmetic and the length rule of the trajectory kernels, one copy each, so that what must agree bit for bit does:
//   traj_len        every kernel that reads gen / gt by a step count: traj.hip (traj_metrics_kernel, traj_metrics_min_kernel,
//                   traj_medoid_kernel), modes.hip (traj_modes_kernel), traj_full.hip
//   traj_step_dist  all of them: ||a - b||_2 over D dims of two float32 rows, in float64 (models/utils/metrics.py:38-55)
//   traj_ade_fde    traj_metrics_kernel, traj_metrics_min_kernel; traj_full.hip sums the same steps in the same order, lane-parallel
//   traj_pair_dist  traj_medoid_kernel's cost and traj_modes_kernel's distance matrix: the medoid's cost IS the index-order mean of a row
//                   of that matrix
// The multiply-add is written as fma(): that is what -ffp-contract=fast has always made of `s += df * df` in traj.hip and modes.hip, and
// spelled out it stays one rounding whatever contraction flag the including file is compiled with.
#pragma once
#include <math.h>
#include <stdint.h>

// how many steps of its Tmax-row buffer sample `at` holds: n[at], at most Tmax (never read past the buffer); no counts: Tmax.  <= 0: none
__device__ __forceinline__ int traj_len(const int32_t* n, long long at, int Tmax) {
    if (!n) return Tmax;
    const int v = n[at];
    return v > Tmax ? Tmax : v;
}

template <typename PA, typename PB> __device__ __forceinline__ double traj_step_dist(PA a, PB b, int D) {
    double s = 0.0;
    for (int c = 0; c < D; ++c) {
        const double df = (double)a[c] - (double)b[c];
        s = fma(df, df, s);
    }
    return sqrt(s);
}

// g [ng, D] against gt [nt, D], ng, nt > 0: g padded with its last step / cut to nt (metrics.py:40-52), then
// ade = mean_t ||gt_t - g_t||_2 (summed in index order, divided once), fde = ||gt_last - g_last||_2
__device__ __forceinline__ void traj_ade_fde(const float* gt, int nt, const float* g, int ng, int D, double& ade, double& fde) {
    double acc = 0.0, lastd = 0.0;
    for (int t = 0; t < nt; ++t) {
        const int tg = t < ng ? t : ng - 1;
        lastd = traj_step_dist(gt + (long long)t * D, g + (long long)tg * D, D);
        acc += lastd;
    }
    ade = acc / nt;
    fde = lastd;
}

// d(j, i) of two samples, nj, ni > 0: mean over t < max(nj, ni) of ||gj[min(t, nj - 1)] - gi[min(t, ni - 1)]||_2, each sample padded
// with its own last step, summed in index order and divided once; bit-symmetric in (j, i)
__device__ __forceinline__ double traj_pair_dist(const float* gj, int nj, const float* gi, int ni, int D) {
    const int n = nj > ni ? nj : ni;
    double acc = 0.0;
    for (int t = 0; t < n; ++t) {
        const int tj = t < nj ? t : nj - 1, ti = t < ni ? t : ni - 1;
        acc += traj_step_dist(gj + (long long)tj * D, gi + (long long)ti * D, D);
    }
    return acc / n;
}
