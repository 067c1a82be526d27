// One decoding step's token choice for a whole batch, on the device (A13): logits -> processed scores -> next token.
//
// replaces what HF GenerationMixin.generate does between two forward passes when the reference calls it with its defaults
// (models/pointllm/model_arch.py:82-108: do_sample=True, top_k=50, top_p=0.95, temperature=1.0, repetition_penalty,
// output_scores=True): RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper
// (transformers/generation/logits_process.py:306-366,238-300,542-580,473-540), torch.multinomial on the softmax, the
// eos / pad bookkeeping of unfinished sequences, and the append to input_ids.  `scores` are the PROCESSED scores, as HF
// returns them (fp32, -inf where a warper removed the token).
//
// One 1024-thread workgroup per row; the row lives in registers (V <= 32768) or is re-read from the fp32 scores row (L2).
//   top-k, top-p : choice.h (top_k_step, top_p_step), the steps beam_rows_kernel takes too; here min_tokens_to_keep = 1
//   sample: Gumbel-max — argmax_i (score_i + g_i), g_i = -log(-log u_i), u_i from Philox4x32-10 keyed by (seed; row, i/4,
//           draw counter): an exact draw from softmax(scores) with no scan and no host RNG; seed and counter live in device
//           memory so a captured hipGraph draws fresh numbers at every replay.  do_sample = 0: plain arg-max (lowest index).
// No length is read from the host: `pos` is a launch constant, like every other decode entry point.
#include "choice.h"

#define SMP_THREADS CH_THREADS

struct SampleArgs {
    const void* logits; long long ld; int B, V;
    float* scores; long long ld_scores;
    int64_t* seq; long long ld_seq; int pos, rep_from;
    int64_t* ids; int* done;
    float rep_penalty, temperature; int top_k; float top_p; int do_sample;
    const unsigned long long* rng;        // [0] seed, [1] draw counter base (device memory)
    int draw;                             // added to the counter base: one value per captured step
    long long eos, pad;
};

template <typename T, bool REG>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(SampleArgs a) {
    __shared__ float redf[CH_WAVES];
    __shared__ int redi[CH_WAVES];
    __shared__ unsigned long long red64[CH_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
    const T* lg = (const T*)a.logits + (long long)b * a.ld;
    float* sc = a.scores + (long long)b * a.ld_scores;
    ChoiceRow<REG> row;
    row.sc = sc; row.V = V;
    const int niter = row.niter();
    const float NEG_INF = -INFINITY;

    // ---- repetition penalty (on the raw logits, tokens seq[b, rep_from : pos]) and temperature.  Element c = i*1024 + tid.
    if (a.rep_penalty != 1.0f && a.seq) {
        for (int c = tid; c < V; c += SMP_THREADS) sc[c] = Cvt<T>::ld(lg + c);
        __syncthreads();
        rep_penalty_scatter(sc, V, a.seq + (long long)b * a.ld_seq, a.rep_from, a.pos, a.rep_penalty, [&](long long t) { return Cvt<T>::ld(lg + t); });
        __syncthreads();
        _Pragma("unroll") for (int i = 0; i < niter; ++i) {
            const int c = i * SMP_THREADS + tid;
            float v = c < V ? sc[c] : NEG_INF;
            if (a.temperature != 1.0f && c < V) v = v / a.temperature;
            if (REG) row.x[i] = v; else if (c < V) sc[c] = v;
        }
    } else {
        _Pragma("unroll") for (int i = 0; i < niter; ++i) {
            const int c = i * SMP_THREADS + tid;
            float v = c < V ? Cvt<T>::ld(lg + c) : NEG_INF;
            if (a.temperature != 1.0f && c < V) v = v / a.temperature;
            if (REG) row.x[i] = v; else if (c < V) sc[c] = v;
        }
    }
    if (!REG) __syncthreads();

    top_k_step(row, a.top_k, redi);
    if (a.top_p < 1.0f) {                                          // min_tokens_to_keep = 1: the largest element is never removed
        const unsigned long long top = row_max_below(row, ~0ull, red64);
        top_p_step(row, a.top_p, top, top, redf);
    }

    // ---- processed scores out (HF output_scores) and the token
    unsigned long long best = 0ull;
    unsigned long long seed = 0, ctr = 0;
    if (a.do_sample && a.rng) { seed = a.rng[0]; ctr = a.rng[1] + (unsigned long long)a.draw; }
    _Pragma("unroll") for (int i = 0; i < niter; ++i) {
        const int c = i * SMP_THREADS + tid;
        if (c >= V) continue;
        float v = row.get(i, c);
        if (REG) sc[c] = v;
        if (a.do_sample && v != NEG_INF) v += gumbel_noise((unsigned)b, (unsigned)c, seed, ctr);
        // removed tokens (-inf) can never win: their key is the smallest finite-or-infinite image; ties -> lowest index
        const unsigned long long k = ((unsigned long long)f2key(v) << 32) | (0xFFFFFFFFu - (unsigned)c);
        best = k > best ? k : best;
    }
    best = block_max_u64(best, red64);
    if (tid == 0) {
        long long id = (long long)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));
        if (a.done) {                                            // HF: finished rows emit pad; a row finishes when it emits eos
            if (a.done[b]) id = a.pad;
            else if (a.eos >= 0 && id == a.eos) a.done[b] = 1;
        }
        a.ids[b] = id;
        if (a.seq) a.seq[(long long)b * a.ld_seq + a.pos] = id;
    }
}

extern "C" int egomi_sample_rows(const void* logits, int64_t ld, int B, int V, float* scores, int64_t ld_scores, int64_t* seq, int64_t ld_seq,
                                 int pos, int rep_from, int64_t* ids, int* done, float repetition_penalty, float temperature, int top_k,
                                 float top_p, int do_sample, const uint64_t* rng, int draw, int64_t eos_id, int64_t pad_id, int dtype,
                                 egomi_stream_t stream) {
    if (!logits || !scores || !ids) return EGOMI_E_BADARG;
    if (B <= 0 || V <= 0 || ld < V || ld_scores < V || (seq && (pos < 0 || pos >= ld_seq || rep_from < 0 || rep_from > pos))) return EGOMI_E_SHAPE;
    if (!(repetition_penalty > 0.f) || !(temperature > 0.f) || top_k < 0 || !(top_p > 0.f) || top_p > 1.f) return EGOMI_E_BADARG;
    if (do_sample && !rng) return EGOMI_E_BADARG;
    if (repetition_penalty != 1.0f && !seq) return EGOMI_E_BADARG;
    SampleArgs a;
    a.logits = logits; a.ld = ld; a.B = B; a.V = V; a.scores = scores; a.ld_scores = ld_scores; a.seq = seq; a.ld_seq = ld_seq; a.pos = pos;
    a.rep_from = rep_from; a.ids = ids; a.done = done; a.rep_penalty = repetition_penalty; a.temperature = temperature; a.top_k = top_k;
    a.top_p = top_p; a.do_sample = do_sample; a.rng = (const unsigned long long*)rng; a.draw = draw; a.eos = eos_id; a.pad = pad_id;
    const bool reg = V <= SMP_THREADS * CH_NPT;
    if (reg) EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((sample_rows_kernel<T, true>), dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, a));
    else EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((sample_rows_kernel<T, false>), dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, a));
    return egomi_launch_status();
}
