// M diverse modes of K sampled trajectories, with confidences (A13): the short list a planner or a "minADE of M modes" evaluation wants
// from K samples, chosen without the ground truth.  Between the two extremes the package already has -- all K (traj_metrics_min_kernel) and
// one pick (traj_medoid_kernel, seq_rank_kernel) -- and built from their pieces: the pairwise displacement of the medoid, the ranking rule
// of seq_rank.
//
// egomi_traj_modes: one 256-thread workgroup per clip, K <= 64.
//   Phase 1, all 256 threads: the K (K - 1) / 2 unordered pairs are dealt round-robin; a thread computes d(j, i) with traj_medoid_kernel's own
//     function (traj_disp.h: traj_pair_dist, so that kernel's cost is the index-order mean of a row of `dist`, bit for bit) and stores it to both halves of a [64][64] float64
//     LDS tile, so the matrix is bit-symmetric; diagonal 0, NaN wherever j or i is invalid.  The tile goes out to `dist` row by row.
//   Phase 2, wavefront 0 alone, lane j = sample j, no barrier and no LDS write: lanes read column j of a tile row (tile[c][j] = d(j, c),
//     consecutive addresses), talk through ballots and shuffles, and keep everything else in registers.
//       order   key_j = -score_j (NaN -> -inf) or the centrality c_j = mean of d(j, i) over the valid i != j, summed in index order and
//               divided once (traj_medoid_kernel's cost); rank_j = number of valid i with a smaller key, or an equal key and a lower index
//       NMS     walk the ranks; the candidate becomes the next mode unless some picked mode m has !(d > radius)
//       fill    while slots are free: the valid unpicked sample with the largest minimum distance to the picked modes (ties -> lower
//               index), as long as that distance is > 0
//       assign  slot of the nearest mode (ties -> lower slot, a mode to itself), conf = members / n_valid
//   The order of every sum depends on (K, Tmax, D, n_gen) only; nothing is accumulated across threads: a replay is bit-equal.
#include "common.h"
#include "traj_disp.h"
#include <math.h>

#define MODES_THREADS 256
#define MODES_MAXK 64

__global__ __launch_bounds__(MODES_THREADS) void traj_modes_kernel(const float* gen, const int32_t* n_gen, const float* score, int K, int Tmax, int D,
                                                                   int M, double radius, double* dist, int32_t* modes, double* conf,
                                                                   int32_t* assign, int32_t* n_modes, int32_t* n_nms) {
    __shared__ double tile[MODES_MAXK][MODES_MAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* gb = gen + (long long)b * K * Tmax * D;

    // ---- phase 1: the distance matrix
    if (tid < K) tile[tid][tid] = traj_len(n_gen, (long long)b * K + tid, Tmax) > 0 ? 0.0 : NAN;
    const int npair = K * (K - 1) / 2;
    for (int p = tid; p < npair; p += MODES_THREADS) {
        int j = 0, rem = p;                                                 // pair p = (j, i), j < i, row by row
        while (rem >= K - 1 - j) { rem -= K - 1 - j; ++j; }
        const int i = j + 1 + rem;
        const int nj = traj_len(n_gen, (long long)b * K + j, Tmax), ni = traj_len(n_gen, (long long)b * K + i, Tmax);
        double d = NAN;
        if (nj > 0 && ni > 0) d = traj_pair_dist(gb + (long long)j * Tmax * D, nj, gb + (long long)i * Tmax * D, ni, D);
        tile[j][i] = d;
        tile[i][j] = d;
    }
    __syncthreads();
    if (dist) {
        double* db = dist + (long long)b * K * K;
        for (int e = tid; e < K * K; e += MODES_THREADS) db[e] = tile[e / K][e % K];
    }
    if (tid >= EGOMI_WAVE) return;

    // ---- phase 2: one wavefront, lane j owns sample j; the tile is read-only from here on
    const int j = tid;
    const bool valid = j < K && traj_len(n_gen, (long long)b * K + (j < K ? j : 0), Tmax) > 0;
    const unsigned long long vmask = __ballot(valid);
    const int nvalid = __popcll(vmask);

    double key = 0.0;
    if (score) {
        if (valid) {
            const float s = score[(long long)b * K + j];
            key = s != s ? (double)INFINITY : -(double)s;                   // descending score; a NaN score ranks as -inf
        }
    } else {
        double tot = 0.0;
        int others = 0;
        for (int i = 0; i < K; ++i) {
            if (!((vmask >> i) & 1ull) || i == j || !valid) continue;
            tot += tile[i][j];
            ++others;
        }
        key = others ? tot / others : 0.0;                                  // ascending centrality
    }
    int rank = 0;
    for (int i = 0; i < K; ++i) {
        const double ki = __shfl(key, i, EGOMI_WAVE);
        if (((vmask >> i) & 1ull) && (ki < key || (ki == key && i < j))) ++rank;
    }

    double mind = INFINITY;                                                 // smallest distance to a picked mode, and that mode's slot
    int slot = -1, mymode = -1, nm = 0;
    bool sup = false, picked = false;                                       // within the radius of a picked mode; a mode itself
    auto pick = [&](int c) {
        if (j == nm) mymode = c;
        if (valid) {
            const double d = tile[c][j];
            if (!(d > radius)) sup = true;
            if (d < mind) { mind = d; slot = nm; }
        }
        if (j == c) { picked = true; slot = nm; mind = 0.0; }
        ++nm;
    };
    for (int r = 0; r < nvalid && nm < M; ++r) {
        const int c = __ffsll((long long)__ballot(valid && rank == r)) - 1;
        if (c < 0 || __shfl((int)sup, c, EGOMI_WAVE)) continue;            // (c < 0: a NaN centrality, from non-finite input, has no rank)
        pick(c);
    }
    const int nnms = nm;
    while (nm < M) {
        double v = (valid && !picked && mind == mind) ? mind : -1.0;        // distances are >= 0: -1 stands for "no candidate"
        int vi = j;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, EGOMI_WAVE);
            const int oi = __shfl_xor(vi, o, EGOMI_WAVE);
            if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
        }
        if (!(v > 0.0)) break;                                              // nothing left, or exact duplicates of the picked modes
        pick(vi);
    }

    double cf = 0.0;
    for (int m = 0; m < nm; ++m) {
        const int cnt = __popcll(__ballot(valid && slot == m));
        if (j == m) cf = (double)cnt / (double)nvalid;
    }
    if (j < K) assign[(long long)b * K + j] = valid ? slot : -1;
    if (j < M) {
        modes[(long long)b * M + j] = mymode;
        conf[(long long)b * M + j] = cf;
    }
    if (j == 0) { n_modes[b] = nm; n_nms[b] = nnms; }
}

extern "C" int egomi_traj_modes(const float* gen, const int32_t* n_gen, const float* score, int B, int K, int Tmax, int D, int M, double radius,
                                double* dist, int32_t* modes, double* conf, int32_t* assign, int32_t* n_modes, int32_t* n_nms,
                                egomi_stream_t stream) {
    if (!gen || !modes || !conf || !assign || !n_modes || !n_nms) return EGOMI_E_BADARG;
    if (radius != radius || radius < 0.0) return EGOMI_E_BADARG;
    if (B <= 0 || K <= 0 || Tmax <= 0 || D <= 0 || M <= 0) return EGOMI_E_SHAPE;
    if (K > MODES_MAXK || M > MODES_MAXK) return EGOMI_E_UNSUPPORTED;
    EGOMI_LAUNCH(traj_modes_kernel, dim3(B), dim3(MODES_THREADS), 0, (hipStream_t)stream, gen, n_gen, score, K, Tmax, D, M, radius, dist, modes,
                 conf, assign, n_modes, n_nms);
    return egomi_launch_status();
}
