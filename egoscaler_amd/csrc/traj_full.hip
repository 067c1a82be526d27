// The whole metric module of the reference on the device, per sample: ADE, FDE, IDE, GD and DTW of K generated trajectories per clip
// against the clip's ground truth, with the per-clip minima and arg-minima, in one launch (egomi_traj_metrics_full, include/egomi.h).
// replaces (float64 from the float32 inputs):
//   models/utils/metrics.py:38-55  ADE   traj_metrics_kernel's rows (traj_disp.h: the same step distance, the same order), bit for bit
//   models/utils/metrics.py:7-27   FDE   likewise
//   models/utils/metrics.py:29-36  IDE   ||gt[0] - gen[0]||_2 over all D dims
//   models/utils/metrics.py:61-87  GD    mean over the ground-truth steps of 2 acos(clip(<q(gen_t), q(gt_t)>)), q = scipy's from_rotvec; the
//                                        dot product as it is, not its absolute value, as the reference has it
//   models/utils/metrics.py:57-59  DTW   the exact dynamic programme on the unpadded sequences (the reference calls fastdtw(radius=1), an
//                                        approximation that searches a window of the same table)
// One workgroup per clip: the clip's ground truth is staged once in LDS as float32 (rows < n_gt only), the samples are dealt over the
// workgroup's wavefronts.  This file is compiled with -ffp-contract=off (build.EXTRA): every rounding below is the one that is written.
#include "common.h"
#include "traj_disp.h"
#include <math.h>

#define FULL_THREADS 512                     // 8 wavefronts: a sample is a chain of latencies, so a CU interleaves two of them per SIMD
                                             // (16 would leave 128 registers per lane, which this kernel exceeds by a few and spills)
#define FULL_WAVES (FULL_THREADS / 64)
#define FULL_MAXT 256
#define FULL_MAXD 64
#define FULL_STRIP (FULL_MAXT / 64)          // rows of the DTW table a lane owns at most
#define FULL_COLS 5                          // ADE, FDE, IDE, GD, DTW

// scipy's Rotation.from_rotvec (the reference's call) of three float32 components: (s r, cos(|r| / 2))
__device__ __forceinline__ void rotvec_quat(const float* r, double q[4]) {
    const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
    const double a = sqrt(x * x + y * y + z * z);
    double s;
    if (a <= 1e-3) {
        const double a2 = a * a;
        s = 0.5 - a2 / 48.0 + a2 * a2 / 3840.0;
    } else {
        s = sin(a / 2.0) / a;
    }
    q[0] = s * x; q[1] = s * y; q[2] = s * z; q[3] = cos(a / 2.0);
}

__device__ __forceinline__ double rot_angle(const float* ra, const float* rb) {
    double qa[4], qb[4];
    rotvec_quat(ra, qa);
    rotvec_quat(rb, qb);
    double d = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3];
    d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
    return 2.0 * acos(d);
}

__device__ __forceinline__ double min3(double a, double b, double c) {
    const double m = b < a ? b : a;
    return c < m ? c : m;
}

extern __shared__ float full_gt[];           // [nt, D]: the clip's ground truth

__global__ __launch_bounds__(FULL_THREADS) void traj_metrics_full_kernel(const float* gen, const int32_t* n_gen, const float* gt,
                                                                         const int32_t* n_gt, int K, int Tmax, int D, int rot0, double* out,
                                                                         double* mins, int32_t* args) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = traj_len(n_gt, b, Tmax);
    const float* gtb = gt + (long long)b * Tmax * D;
    for (int i = threadIdx.x; i < nt * D; i += FULL_THREADS) full_gt[i] = gtb[i];      // nothing of gt beyond its nt rows is read
    __syncthreads();
    const bool rot = rot0 >= 0 && rot0 + 3 <= D;
    const double inf = HUGE_VAL;

    for (int j = wave; j < K; j += FULL_WAVES) {                                         // wave-uniform: every lane of a wave runs one sample
        const int ng = traj_len(n_gen, (long long)b * K + j, Tmax);
        double* o = out + ((long long)b * K + j) * FULL_COLS;
        if (ng <= 0 || nt <= 0) {
            if (lane < FULL_COLS) o[lane] = NAN;
            continue;
        }
        const float* g = gen + ((long long)b * K + j) * Tmax * D;

        // ADE, FDE, GD: lane l takes steps l, l + 64, ...; the sums run over the steps in index order, as traj_metrics_kernel's do
        double dsum = 0.0, asum = 0.0, lastd = 0.0;
        for (int t0 = 0; t0 < nt; t0 += 64) {
            const int t = t0 + lane, cnt = nt - t0 < 64 ? nt - t0 : 64;
            double d = 0.0, a = 0.0;
            if (t < nt) {
                const float* gr = g + (long long)(t < ng ? t : ng - 1) * D;              // padded with the last step / cut at nt
                d = traj_step_dist(full_gt + t * D, gr, D);
                if (rot) a = rot_angle(gr + rot0, full_gt + t * D + rot0);
            }
            for (int l = 0; l < cnt; ++l) {
                lastd = __shfl(d, l, 64);
                dsum += lastd;
                asum += __shfl(a, l, 64);
            }
        }
        const double ide = traj_step_dist(full_gt, g, D);

        // DTW: lane l owns the rows [l R, l R + R) of the ng x nt table and walks them column by column, one column behind lane l - 1:
        // at step s it fills column s - l, so a step is one anti-diagonal of strips.  Of the table it keeps the previous column of its
        // rows (prev) and the two values of the row above its strip that the lane before it passed down (up, upd).
        const int R = (ng + 63) >> 6, i0 = lane * R;
        const int rows = ng - i0 < 0 ? 0 : (ng - i0 < R ? ng - i0 : R);
        const int lanes = (ng + R - 1) / R;
        double prev[FULL_STRIP], upd = inf, tail = inf;
#pragma unroll
        for (int r = 0; r < FULL_STRIP; ++r) prev[r] = inf;
        for (int s = 0; s < nt + lanes - 1; ++s) {
            const double passed = __shfl_up(tail, 1, 64);                                // Dp(i0 - 1, s - lane): lane - 1 filled it a step ago
            const int k = s - lane;
            if (rows > 0 && k >= 0 && k < nt) {
                double up = lane ? passed : inf, diag = (lane && k) ? upd : inf;
                upd = passed;
                const float* y = full_gt + k * D;
#pragma unroll
                for (int r = 0; r < FULL_STRIP; ++r) {
                    if (r < rows) {
                        const double c = traj_step_dist(g + (long long)(i0 + r) * D, y, D);
                        const double left = prev[r];
                        const double v = (i0 + r == 0 && k == 0) ? c : c + min3(up, left, diag);
                        diag = left;
                        up = v;
                        prev[r] = v;
                    }
                }
                tail = up;
            }
        }
        const double dtw = __shfl(tail, lanes - 1, 64);                                  // Dp(ng - 1, nt - 1)

        if (lane == 0) {
            o[0] = dsum / nt;
            o[1] = lastd;
            o[2] = ide;
            o[3] = rot ? asum / nt : NAN;
            o[4] = dtw;
        }
    }
    if (!mins) return;
    __threadfence_block();
    __syncthreads();                                                                     // the clip's rows of `out` are written
    if (wave == 0 && lane < FULL_COLS) {                                                 // one lane per column, samples in index order
        double bv = NAN;
        int bi = -1;
        for (int j = 0; j < K; ++j) {
            const double v = out[((long long)b * K + j) * FULL_COLS + lane];
            if (v != v) continue;
            if (bi < 0 || v < bv) { bv = v; bi = j; }
        }
        mins[(long long)b * FULL_COLS + lane] = bv;
        args[(long long)b * FULL_COLS + lane] = bi;
    }
}

extern "C" int egomi_traj_metrics_full(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int K, int Tmax, int D,
                                       int rot0, double* out, double* mins, int32_t* args, egomi_stream_t stream) {
    if (!gen || !gt || !out || (mins != nullptr) != (args != nullptr)) return EGOMI_E_BADARG;
    if (B <= 0 || K < 1 || Tmax < 1 || Tmax > FULL_MAXT || D < 1 || D > FULL_MAXD) return EGOMI_E_SHAPE;
    EGOMI_LAUNCH(traj_metrics_full_kernel, dim3(B), dim3(FULL_THREADS), (size_t)Tmax * D * sizeof(float), (hipStream_t)stream, gen, n_gen, gt, n_gt,
                 K, Tmax, D, rot0, out, mins, args);
    return egomi_launch_status();
}
