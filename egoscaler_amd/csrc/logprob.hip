// Which of K to keep, without the ground truth (A13): the log-probability of every generated token under the RAW model distribution,
// summed per sequence on the device inside the captured token loop, and the per-clip ranking of the K sequences by it.
//
// replaces transformers/generation/utils.py compute_transition_scores on generate(output_logits=True): HF keeps the raw logits of every
// step ([T, rows, V] on the host side of the loop), takes log_softmax of them and gathers the chosen tokens afterwards.  Here one launch per
// decode step, right after egomi_sample_rows / egomi_argmax_rows has written the step's ids, reads the same raw logits buffer (those kernels
// do not modify it) and keeps three numbers per row: the token's log-prob, the running sum and the token count.  `scores` (the PROCESSED
// rows, -inf where top-k / top-p removed a token) cannot serve: the log-softmax of a processed row is not the model's probability.
//
// egomi_token_logprob: one 1024-thread workgroup per row.  Element e of the row belongs to thread (e / 8) % 1024 whatever the row's
//   address is, so the fp32 sum runs in an order that depends on V only: a row's bits depend neither on R, on its slot, nor on its
//   alignment.  Every thread reads its 8-element chunks with 16-byte loads at 16-byte ALIGNED addresses (a row of V = 32262 bf16 logits
//   starts 12 bytes off every second line) and shifts the chunk into place in registers; a block that holds no byte of the row is not
//   read, and elements outside [0, V) are dropped by index, so padding columns and neighbouring rows never enter.  V <= 32768: the row
//   stays in registers between the max and the sum (read once); longer rows are read twice (L2).
//     m = max x;  s = sum exp(x - m)  (fp32, accurate expf / logf);  lp = (x[tok] - m) - log s
//   Bookkeeping by thread 0: tok_lp[r, col] = lp, sum_lp[r] += lp, n_tok[r] += 1, live[r] = 0 once the row emitted eos (the eos itself is
//   counted, the pads after it are not; a row with live[r] == 0 writes tok_lp[r, col] = 0 and nothing else).  The kernel keeps this flag
//   of its own because egomi_sample_rows has already set `done` for the step when it runs, and pad may equal eos.
//   A token id outside [0, V) (device data, so no error code can report it) reads x[clamp(tok)] and yields lp = NaN: the row's column,
//   its sum and everything ranked from it show NaN; nothing out of range is read.
//   No atomics, no length read from device memory: `col` is a launch constant like `pos` of the other step kernels.
// egomi_seq_rank: one workgroup per clip; score = sum_lp / n_tok^length_penalty (HF's beam convention: 1 = mean log-prob, 0 = the sum),
//   -inf for an empty row; order = the clip's K indices by descending score, by counting (rank of j = number of rows that beat it),
//   ties -> lower index, -inf rows last in index order.  A NaN score ranks as -inf.
// egomi_bin_stats: the same row pass (lp_row_max_sumexp, shared with egomi_token_logprob), then mass / mean / std / entropy of the step's
//   distribution over the waypoint bin tokens; described at the kernel below.
#include "lp_row.h"                      // lp_load8, lp_row_max_sumexp, block_sum2_f64: shared with csrc/grammar.hip

struct LogprobArgs {
    const void* logits; long long ld; int R, V;
    const int64_t* tok; long long eos; int* live;
    float* tok_lp; long long ld_lp; int col;
    float* sum_lp; int* n_tok;
};

template <typename T, bool REG>
__global__ __launch_bounds__(LPB_THREADS) void token_logprob_kernel(LogprobArgs a) {
    __shared__ float red[16];
    const int r = blockIdx.x, tid = threadIdx.x, V = a.V;
    if (a.live && a.live[r] == 0) {                                      // uniform; thread 0 alone ever writes live[r], after the barriers below
        if (tid == 0) a.tok_lp[(long long)r * a.ld_lp + a.col] = 0.f;
        return;
    }
    const T* lg = (const T*)a.logits + (long long)r * a.ld;
    float m, s;
    lp_row_max_sumexp<T, REG>(lg, V, red, m, s);
    if (tid == 0) {
        const long long t = a.tok[r];
        const bool bad = t < 0 || t >= V;
        const long long tc = t < 0 ? 0 : (t >= V ? V - 1 : t);
        const float xt = Cvt<T>::ld(lg + tc);
        const float lp = bad ? NAN : (xt - m) - logf(s);
        a.tok_lp[(long long)r * a.ld_lp + a.col] = lp;
        a.sum_lp[r] += lp;
        a.n_tok[r] += 1;
        if (a.live && a.eos >= 0 && t == a.eos) a.live[r] = 0;
    }
}

extern "C" int egomi_token_logprob(const void* logits, int64_t ld, int R, int V, const int64_t* tok, int64_t eos_id, int32_t* live, float* tok_lp,
                                   int64_t ld_lp, int col, float* sum_lp, int32_t* n_tok, int dtype, egomi_stream_t stream) {
    if (!logits || !tok || !tok_lp || !sum_lp || !n_tok) return EGOMI_E_BADARG;
    if (dtype != EGOMI_F32 && dtype != EGOMI_BF16) return EGOMI_E_BADARG;
    if (R <= 0 || V <= 0 || ld < V || col < 0 || ld_lp <= col) return EGOMI_E_SHAPE;
    if (((uintptr_t)logits) % (dtype == EGOMI_F32 ? 4 : 2)) return EGOMI_E_UNSUPPORTED;      // elements must be naturally aligned
    LogprobArgs a;
    a.logits = logits; a.ld = ld; a.R = R; a.V = V; a.tok = tok; a.eos = eos_id; a.live = live; a.tok_lp = tok_lp; a.ld_lp = ld_lp; a.col = col;
    a.sum_lp = sum_lp; a.n_tok = n_tok;
    if (V <= LPB_THREADS * LPB_NPT) EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((token_logprob_kernel<T, true>), dim3(R), dim3(LPB_THREADS), 0, (hipStream_t)stream, a));
    else EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((token_logprob_kernel<T, false>), dim3(R), dim3(LPB_THREADS), 0, (hipStream_t)stream, a));
    return egomi_launch_status();
}

// egomi_bin_stats: what the step's distribution says about a waypoint coordinate, from the same raw row.  m and s as above (the same function);
// then thread i < nb owns bin i: w_i = exp(x[p0 + i] - m) in fp32 (-inf -> 0; the element is re-read, its line is cache-hot), and Z = sum w,
// sum w v, the centred sum w (v - mean)^2 and -sum q log q (q = w / Z) run in float64 through the workgroup in a fixed order (xor butterfly
// per wave, the 16 wave results in index order).  Thread 0 stores mass = Z / s, mean, std, ent as fp32 at column `col`.  No state, no
// atomics, nothing read outside [row, row + V): a row's bits depend on (V, p0, nb, dtype) and its values only.
struct BinStatsArgs {
    const void* logits; long long ld; int V, p0, nb;
    const double* values;
    float *mass, *mean, *std, *ent; long long ld_out; int col;
};

template <typename T, bool REG>
__global__ __launch_bounds__(LPB_THREADS) void bin_stats_kernel(BinStatsArgs a) {
    __shared__ float red[16];
    __shared__ double red2[32];
    const int r = blockIdx.x, tid = threadIdx.x;
    const T* lg = (const T*)a.logits + (long long)r * a.ld;
    float m, s;
    lp_row_max_sumexp<T, REG>(lg, a.V, red, m, s);
    const bool own = tid < a.nb;
    double w = 0.0, v = 0.0;
    if (own) {
        const float xi = Cvt<T>::ld(lg + a.p0 + tid);
        w = (double)(xi == -INFINITY ? 0.f : expf(xi - m));
        v = a.values[tid];
    }
    double Z = w, wv = w * v;
    block_sum2_f64(Z, wv, red2);
    const double mean = wv / Z;                                          // Z = 0 (every bin -inf): NaN, and so are std and ent
    const double d = v - mean, q = w / Z;
    double m2 = own ? w * d * d : 0.0;
    double h = (!own || q == 0.0) ? 0.0 : -q * log(q);                   // 0 log 0 = 0; a NaN q stays NaN
    block_sum2_f64(m2, h, red2);
    if (tid == 0) {
        const long long o = (long long)r * a.ld_out + a.col;
        a.mass[o] = (float)Z / s;
        a.mean[o] = (float)mean;
        a.std[o] = (float)sqrt(m2 / Z);
        a.ent[o] = (float)h;
    }
}

extern "C" int egomi_bin_stats(const void* logits, int64_t ld, int R, int V, int p0, int nb, const double* values, float* mass, float* mean,
                               float* std, float* ent, int64_t ld_out, int col, int dtype, egomi_stream_t stream) {
    if (!logits || !values || !mass || !mean || !std || !ent) return EGOMI_E_BADARG;
    if (dtype != EGOMI_F32 && dtype != EGOMI_BF16) return EGOMI_E_BADARG;
    if (R <= 0 || V <= 0 || ld < V || col < 0 || ld_out <= col) return EGOMI_E_SHAPE;
    if (nb < 1 || nb > LPB_THREADS || p0 < 0 || (long long)p0 + nb > V) return EGOMI_E_SHAPE;
    if (((uintptr_t)logits) % (dtype == EGOMI_F32 ? 4 : 2)) return EGOMI_E_UNSUPPORTED;      // elements must be naturally aligned
    BinStatsArgs a;
    a.logits = logits; a.ld = ld; a.V = V; a.p0 = p0; a.nb = nb; a.values = values;
    a.mass = mass; a.mean = mean; a.std = std; a.ent = ent; a.ld_out = ld_out; a.col = col;
    if (V <= LPB_THREADS * LPB_NPT) EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((bin_stats_kernel<T, true>), dim3(R), dim3(LPB_THREADS), 0, (hipStream_t)stream, a));
    else EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((bin_stats_kernel<T, false>), dim3(R), dim3(LPB_THREADS), 0, (hipStream_t)stream, a));
    return egomi_launch_status();
}

#define RNK_THREADS 256
#define RNK_MAXK 1024

__global__ __launch_bounds__(RNK_THREADS) void seq_rank_kernel(const float* sum_lp, const int32_t* n_tok, int K, float length_penalty, float* score,
                                                               int32_t* order) {
    __shared__ float key[RNK_MAXK];
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < K; j += RNK_THREADS) {
        const int n = n_tok[(long long)b * K + j];
        // n^0 = 1 and n^1 = n exactly, whatever powf's last bit: the sum and the mean are what their names say
        const float den = length_penalty == 0.f ? 1.f : (length_penalty == 1.f ? (float)n : powf((float)n, length_penalty));
        const float sc = n > 0 ? sum_lp[(long long)b * K + j] / den : -INFINITY;
        score[(long long)b * K + j] = sc;
        key[j] = sc != sc ? -INFINITY : sc;                              // a NaN score ranks with the empty rows
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += RNK_THREADS) {
        const float kj = key[j];
        int rank = 0;
        for (int i = 0; i < K; ++i) rank += (key[i] > kj || (key[i] == kj && i < j)) ? 1 : 0;
        order[(long long)b * K + rank] = j;
    }
}

extern "C" int egomi_seq_rank(const float* sum_lp, const int32_t* n_tok, int B, int K, float length_penalty, float* score, int32_t* order,
                              egomi_stream_t stream) {
    if (!sum_lp || !n_tok || !score || !order) return EGOMI_E_BADARG;
    if (length_penalty != length_penalty) return EGOMI_E_BADARG;
    if (B <= 0 || K <= 0) return EGOMI_E_SHAPE;
    if (K > RNK_MAXK) return EGOMI_E_UNSUPPORTED;
    EGOMI_LAUNCH(seq_rank_kernel, dim3(B), dim3(RNK_THREADS), 0, (hipStream_t)stream, sum_lp, n_tok, K, length_penalty, score, order);
    return egomi_launch_status();
}
