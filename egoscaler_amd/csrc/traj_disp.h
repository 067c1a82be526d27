// The displacement of one step, shared by every kernel whose ADE / FDE must agree bit for bit (traj.hip: traj_metrics_kernel,
// traj_metrics_min_kernel; traj_full.hip): ||a - b||_2 over D dims of two float32 rows, in float64 (models/utils/metrics.py:38-55).
// The multiply-add is written as fma(): that is what -ffp-contract=fast has always made of `s += df * df` in traj.hip, and spelled out it
// stays one rounding whatever contraction flag the including file is compiled with.
#pragma once
#include <math.h>

template <typename PA, typename PB> __device__ __forceinline__ double traj_step_dist(PA a, PB b, int D) {
    double s = 0.0;
    for (int c = 0; c < D; ++c) {
        const double df = (double)a[c] - (double)b[c];
        s = fma(df, df, s);
    }
    return sqrt(s);
}
