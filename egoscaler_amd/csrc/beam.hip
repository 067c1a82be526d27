// Beam search and beam sampling on the device (A13): HF GenerationMixin._beam_search (transformers 5.15 generation/utils.py:3208-3560)
// as two launches per step; attention reads the KV cache through the per-row table they maintain (attn_decode.hip, ROWS).
//
// Rows are LOGICAL beams r = b * nb + j (item b, beam j).  Per step:
//   beam_rows   (one 1024-thread workgroup per row, the row in registers as in sample_rows_kernel):
//               log_softmax(fp32 logits) -> RepetitionPenalty on the log-probs (the row's own sequence) -> [sampling: Temperature ->
//               TopK -> TopP with min_tokens_to_keep] = the processed row, written to `scores` (HF's output_scores); then + the row's
//               running beam score = the accumulated scores, [sampling: + Gumbel noise]; the row's K best (key desc, flat index asc)
//               go out as candidates.  The item's top K over nb * V is contained in the union of its rows' top K.
//   beam_update (one workgroup per item): the item's top K of the nb * K candidates (_get_top_k_continuations :3077; with sampling the
//               Gumbel-top-K of the accumulated scores, which is sequential sampling without replacement, in draw order), the stopping
//               marks, the running-beam choice (_get_running_beams_for_next_iteration), the finished-hypothesis merge with the length
//               penalty (_update_finished_beams :3153), the early-stop heuristic (:3007) and the loop condition (:3055).  Parents'
//               sequences, beam-index history and KV row tables are gathered in place (a workgroup owns all rows of its item).
//               ctl[0] is the loop-open flag: once a step closes it, every later launch of both kernels returns at once, so a captured
//               loop of T steps replays HF's data-dependent number of iterations exactly (ctl[1] counts them).
//   attn_decode_rows (attn_decode.hip): key t of row r is read from physical cache row kv_row[r, t].  Prompt positions of
//               every beam point at its item's single prompt row, later positions at the row that computed the token, so a reorder
//               moves no K/V bytes and no referenced slot is ever overwritten (a step writes slot `pos` of each row's own physical row).
#include "choice.h"

#define BR_THREADS CH_THREADS
#define BR_NPT CH_NPT                    // the row lives in registers: V <= 32768
#define BU_THREADS 256
#define BU_MAXC 2048                     // nb * K candidates per item
#define BU_MAXK 64                       // K = max(2, 1 + n_eos) * nb with one eos: nb <= 32
#define BEAM_NEG 1.0e9f

// ------------------------------------------------------------------------------------------------
// beam_rows
// ------------------------------------------------------------------------------------------------
struct BeamRowArgs {
    const void* logits; long long ld; int lg_div;     // logical row r reads logits row r / lg_div (step 0: the item's prefill row)
    int R, V, nb;
    float* scores; long long ld_scores;
    const int64_t* seq; long long ld_seq; int pos;   // the row's tokens [0, pos)
    float rep_penalty, temperature; int top_k; float top_p; int min_keep; int do_sample;
    const unsigned long long* rng; int draw;
    const float* run_score;
    int K; float* cand_key; float* cand_score; int* cand_tok;
    const int* ctl;
};

template <typename T>
__global__ __launch_bounds__(BR_THREADS) void beam_rows_kernel(BeamRowArgs a) {
    __shared__ float redf[CH_WAVES];
    __shared__ int redi[CH_WAVES];
    __shared__ unsigned long long red64[CH_WAVES];
    if (a.ctl && a.ctl[0] == 0) return;                            // the loop has closed: HF ran no such iteration
    const int r = blockIdx.x, tid = threadIdx.x, V = a.V;
    const T* lg = (const T*)a.logits + (long long)(r / a.lg_div) * a.ld;
    float* sc = a.scores + (long long)r * a.ld_scores;
    const float NEG_INF = -INFINITY;
    ChoiceRow<true> row;
    row.sc = sc; row.V = V;
    float (&x)[BR_NPT] = row.x;

    // ---- log_softmax in fp32 (x - max - log(sum exp(x - max)), element c = i * 1024 + tid)
    float mx = NEG_INF;
#pragma unroll
    for (int i = 0; i < BR_NPT; ++i) {
        const int c = i * BR_THREADS + tid;
        x[i] = c < V ? Cvt<T>::ld(lg + c) : NEG_INF;
        mx = fmaxf(mx, x[i]);
    }
    const float m = block_max(mx, redf);
    float zl = 0.f;
#pragma unroll
    for (int i = 0; i < BR_NPT; ++i) zl += (i * BR_THREADS + tid < V) ? expf(x[i] - m) : 0.f;
    const float lz = logf(block_sum(zl, redf));
#pragma unroll
    for (int i = 0; i < BR_NPT; ++i) x[i] = (i * BR_THREADS + tid < V) ? (x[i] - m) - lz : NEG_INF;

    // ---- repetition penalty on the log-probs, tokens seq[r, 0:pos]; recomputed from the logit so that a repeated token is penalised once
    if (a.rep_penalty != 1.0f) {
#pragma unroll
        for (int i = 0; i < BR_NPT; ++i) { const int c = i * BR_THREADS + tid; if (c < V) sc[c] = x[i]; }
        __syncthreads();
        rep_penalty_scatter(sc, V, a.seq + (long long)r * a.ld_seq, 0, a.pos, a.rep_penalty, [&](long long t) { return (Cvt<T>::ld(lg + t) - m) - lz; });
        __syncthreads();
#pragma unroll
        for (int i = 0; i < BR_NPT; ++i) { const int c = i * BR_THREADS + tid; if (c < V) x[i] = sc[c]; }
        __syncthreads();
    }

    if (a.do_sample) {
        if (a.temperature != 1.0f) {
#pragma unroll
            for (int i = 0; i < BR_NPT; ++i) if (i * BR_THREADS + tid < V) x[i] = x[i] / a.temperature;
        }
        // ---- TopK with k = max(top_k, min_keep), TopP keeping the min_keep largest keys (choice.h: the sampler's own steps)
        if (a.top_k > 0) top_k_step(row, a.top_k > a.min_keep ? a.top_k : a.min_keep, redi);
        if (a.top_p < 1.0f) {
            unsigned long long top = 0ull, keep = ~0ull;           // the largest and the min_keep-th largest key
            for (int q = 0; q < a.min_keep; ++q) {
                keep = row_max_below(row, keep, red64);
                if (q == 0) top = keep;
            }
            top_p_step(row, a.top_p, top, keep, redf);
        }
    }

    // ---- processed row out; accumulated score (+ Gumbel noise when sampling) as a 64-bit key: (value image << 32) | ~flat index
    const float rs = a.run_score[r];
    const unsigned jbase = (unsigned)(r % a.nb) * (unsigned)V;
    unsigned long long seed = 0, ctr = 0;
    if (a.do_sample) { seed = a.rng[0]; ctr = a.rng[1] + (unsigned long long)a.draw; }
    unsigned kimg[BR_NPT];                                         // value images; `taken` drops an element once it is emitted
    unsigned taken = 0u;
#pragma unroll
    for (int i = 0; i < BR_NPT; ++i) {
        const int c = i * BR_THREADS + tid;
        kimg[i] = 0u;
        if (c >= V) { taken |= 1u << i; continue; }
        sc[c] = x[i];
        float v = x[i] + rs;
        if (a.do_sample && v != NEG_INF) v += gumbel_noise((unsigned)r, (unsigned)c, seed, ctr);
        kimg[i] = f2key(v);
    }
    // ---- the row's K best: K rounds of a block arg-max; the owner of the winner emits it and drops it
    for (int j = 0; j < a.K; ++j) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int i = 0; i < BR_NPT; ++i) {
            const unsigned long long k = ((taken >> i) & 1u) ? 0ull
                : ((unsigned long long)kimg[i] << 32) | (0xFFFFFFFFu - (jbase + (unsigned)(i * BR_THREADS + tid)));
            best = k > best ? k : best;
        }
        best = block_max_u64(best, red64);
        const unsigned flat = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu);
        const int c = (int)(flat - jbase), i = c / BR_THREADS;
        if (best != 0ull && c % BR_THREADS == tid) {
            const long long o = (long long)r * a.K + j;
            a.cand_key[o] = key2f((unsigned)(best >> 32));
            a.cand_tok[o] = c;
#pragma unroll
            for (int q = 0; q < BR_NPT; ++q)
                if (q == i) { a.cand_score[o] = x[q] + rs; taken |= 1u << q; }
        }
    }
}

extern "C" int egomi_beam_rows(const void* logits, int64_t ld, int lg_div, int R, int V, int nb, float* scores, int64_t ld_scores,
                               const int64_t* seq, int64_t ld_seq, int pos, float repetition_penalty, float temperature, int top_k, float top_p,
                               int min_tokens_to_keep, int do_sample, const uint64_t* rng, int draw, const float* run_score, int K,
                               float* cand_key, float* cand_score, int32_t* cand_tok, const int32_t* ctl, int dtype, egomi_stream_t stream) {
    if (!logits || !scores || !run_score || !cand_key || !cand_score || !cand_tok) return EGOMI_E_BADARG;
    if (R <= 0 || V <= 0 || nb <= 0 || R % nb || lg_div <= 0 || ld < V || ld_scores < V || K <= 0 || K > V) return EGOMI_E_SHAPE;
    if (V > BR_THREADS * BR_NPT) return EGOMI_E_UNSUPPORTED;
    if (!(repetition_penalty > 0.f) || !(temperature > 0.f) || top_k < 0 || !(top_p > 0.f) || top_p > 1.f || min_tokens_to_keep < 1)
        return EGOMI_E_BADARG;
    if (do_sample && !rng) return EGOMI_E_BADARG;
    if (repetition_penalty != 1.0f && (!seq || pos < 0 || pos > ld_seq)) return EGOMI_E_BADARG;
    BeamRowArgs a;
    a.logits = logits; a.ld = ld; a.lg_div = lg_div; a.R = R; a.V = V; a.nb = nb; a.scores = scores; a.ld_scores = ld_scores;
    a.seq = seq; a.ld_seq = ld_seq; a.pos = pos; a.rep_penalty = repetition_penalty; a.temperature = temperature; a.top_k = top_k;
    a.top_p = top_p; a.min_keep = min_tokens_to_keep; a.do_sample = do_sample; a.rng = (const unsigned long long*)rng; a.draw = draw;
    a.run_score = run_score; a.K = K; a.cand_key = cand_key; a.cand_score = cand_score; a.cand_tok = cand_tok; a.ctl = ctl;
    EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((beam_rows_kernel<T>), dim3(R), dim3(BR_THREADS), 0, (hipStream_t)stream, a));
    return egomi_launch_status();
}

// ------------------------------------------------------------------------------------------------
// beam_update
// ------------------------------------------------------------------------------------------------
struct BeamUpdateArgs {
    int B, nb, K, V;
    const float* cand_key; const float* cand_score; const int* cand_tok;    // [B*nb, K] from beam_rows
    int S0, cur_len, max_len;                                               // prompt length, this step's position, HF's max_length
    long long eos; float length_penalty; int early_stopping;               // 0 False, 1 True, 2 "never"
    int64_t* seq; int64_t* fin_seq; long long ld_seq;                       // running / finished sequences [B*nb, >= max_len]
    int* bidx; int* fin_bidx; long long ld_bidx;                            // beam indices [B*nb, >= max_len - S0]
    int* kv_row; long long ld_kv;                                           // [B*nb, >= max_len] physical cache row of every key
    float* run_score; float* fin_score; int* fin_flag; int* heur;           // [B*nb], [B*nb], [B*nb], [B]
    int64_t* tok;                                                           // [B*nb] the token each running row feeds next
    int* ctl;                                                               // [0] open, [1] iterations, [2..4] per-step tallies, [5] ticket
};

// the item's 2*nb destination rows (0..nb-1 running, nb..2nb-1 finished) of one int array, each from its source row (src_fin: the
// finished array, else the running one) with `new_val` at column cur_col for running sources.  Column-blocked: every read of a column
// precedes (barrier) every write of it, so the gather is in place.
template <typename E>
__device__ __forceinline__ void gather_pass(int b, int nb, int ncols, int cur_col, E* run, E* fin, long long ld, const int* src_row,
                                            const int* src_fin, const E* new_val, bool with_fin) {
    constexpr int CH = 8;
    const int rows = with_fin ? 2 * nb : nb;
    const int cpc = (BU_THREADS * CH) / rows;                   // whole columns per pass
    for (int c0 = 0; c0 < ncols; c0 += cpc) {
        E v[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int e = q * BU_THREADS + threadIdx.x, vr = e % rows, col = c0 + e / rows;
            if (e >= cpc * rows || col >= ncols) continue;
            const E* from = src_fin[vr] ? fin : run;
            v[q] = (col == cur_col && !src_fin[vr]) ? new_val[vr] : from[((long long)b * nb + src_row[vr]) * ld + col];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int e = q * BU_THREADS + threadIdx.x, vr = e % rows, col = c0 + e / rows;
            if (e >= cpc * rows || col >= ncols) continue;
            E* to = vr < nb ? run : fin;
            to[((long long)b * nb + (vr < nb ? vr : vr - nb)) * ld + col] = v[q];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BU_THREADS) void beam_update_kernel(BeamUpdateArgs a) {
    __shared__ unsigned long long s_comp[BU_MAXC];
    __shared__ int s_sel[BU_MAXK];                 // the item's top K: candidate slot (row * K + j) in draw order
    __shared__ int s_src_row[64], s_src_fin[64];  // gather sources of the 2*nb destination rows
    __shared__ int64_t s_new_tok[64];
    __shared__ int s_new_bidx[64], s_new_kv[64];
    __shared__ int s_open;
    const int b = blockIdx.x, tid = threadIdx.x, nb = a.nb, K = a.K, nc = nb * K;
    if (tid == 0) s_open = a.ctl[0];
    __syncthreads();
    if (!s_open) return;
    const int* ctok = a.cand_tok + (long long)b * nc;
    const float* ckey = a.cand_key + (long long)b * nc;
    const float* cscore = a.cand_score + (long long)b * nc;
    for (int i = tid; i < nc; i += BU_THREADS) {
        const unsigned flat = (unsigned)(i / K) * (unsigned)a.V + (unsigned)ctok[i];
        s_comp[i] = ((unsigned long long)f2key(ckey[i]) << 32) | (0xFFFFFFFFu - flat);
    }
    __syncthreads();
    // the item's top K (key desc, flat index asc): rank of each candidate among the nb*K (all distinct: the flat index is in the key)
    for (int i = tid; i < nc; i += BU_THREADS) {
        int rank = 0;
        for (int q = 0; q < nc; ++q) rank += s_comp[q] > s_comp[i] ? 1 : 0;
        if (rank < K) s_sel[rank] = i;
    }
    __syncthreads();
    if (tid == 0) {
        const int row0 = b * nb;
        const bool last = a.cur_len + 1 >= a.max_len;
        float sc[BU_MAXK];
        bool hit[BU_MAXK];
        bool all_hit = true;
        for (int k = 0; k < K; ++k) {
            const int i = s_sel[k];
            sc[k] = cscore[i];
            hit[k] = last || (a.eos >= 0 && (long long)ctok[i] == a.eos);
            all_hit = all_hit && hit[k];
        }
        // running beams: top nb of score + hit * -1e9 (ties -> lower candidate position)
        float run_new[32];
        bool taken[BU_MAXK];
        for (int k = 0; k < K; ++k) taken[k] = false;
        for (int j = 0; j < nb; ++j) {
            int bk = -1; float bv = 0.f;
            for (int k = 0; k < K; ++k) {
                const float v = sc[k] + (hit[k] ? -BEAM_NEG : 0.f);
                if (!taken[k] && (bk < 0 || v > bv)) { bk = k; bv = v; }
            }
            taken[bk] = true;
            run_new[j] = bv;
            const int i = s_sel[bk];
            s_src_row[j] = i / K; s_src_fin[j] = 0;
            s_new_tok[j] = ctok[i]; s_new_bidx[j] = row0 + i / K; s_new_kv[j] = row0 + j;
        }
        // finished hypotheses: merge the item's nb finished with the K candidates (only the first nb that just hit are eligible)
        bool all_fin = true;
        for (int j = 0; j < nb; ++j) all_fin = all_fin && a.fin_flag[row0 + j] != 0;
        const bool full = all_fin && a.early_stopping == 1;
        const bool heur_open = a.heur[b] != 0;
        const float lpf = (float)pow((double)(a.cur_len + 1 - a.S0), (double)a.length_penalty);
        float ms[BU_MAXK + 32];
        for (int j = 0; j < nb; ++j) ms[j] = a.fin_score[row0 + j];
        for (int k = 0; k < K; ++k) {
            float v = sc[k] / lpf;
            v += full ? -BEAM_NEG : 0.f;
            v += heur_open ? 0.f : -BEAM_NEG;
            v += (hit[k] && k < nb) ? 0.f : -BEAM_NEG;
            ms[nb + k] = v;
        }
        bool mtaken[BU_MAXK + 32];
        for (int q = 0; q < nb + K; ++q) mtaken[q] = false;
        float fin_new[32]; int flag_new[32];
        for (int j = 0; j < nb; ++j) {
            int bq = -1; float bv = 0.f;
            for (int q = 0; q < nb + K; ++q)
                if (!mtaken[q] && (bq < 0 || ms[q] > bv)) { bq = q; bv = ms[q]; }
            mtaken[bq] = true;
            fin_new[j] = bv;
            if (bq < nb) {
                s_src_row[nb + j] = bq; s_src_fin[nb + j] = 1; flag_new[j] = a.fin_flag[row0 + bq];
                s_new_tok[nb + j] = 0; s_new_bidx[nb + j] = 0;
            } else {
                const int k = bq - nb, i = s_sel[k];
                s_src_row[nb + j] = i / K; s_src_fin[nb + j] = 0; flag_new[j] = hit[k] && k < nb;
                s_new_tok[nb + j] = ctok[i]; s_new_bidx[nb + j] = row0 + i / K;
            }
            s_new_kv[nb + j] = 0;
        }
        // early-stop heuristic with the new running / finished scores at cur_len + 1 (:3007)
        const int hyp_len = (a.early_stopping == 2 && a.length_penalty > 0.f) ? a.max_len - a.S0 : a.cur_len + 1 - a.S0;
        const float best_possible = run_new[0] / (float)pow((double)hyp_len, (double)a.length_penalty);
        float worst = fin_new[0];
        for (int j = 1; j < nb; ++j) worst = fminf(worst, fin_new[j]);
        bool improvable = false;
        bool all_fin_new = true;
        for (int j = 0; j < nb; ++j) {
            improvable = improvable || best_possible > (flag_new[j] ? worst : -BEAM_NEG);
            all_fin_new = all_fin_new && flag_new[j];
        }
        const bool heur_new = heur_open && improvable;
        for (int j = 0; j < nb; ++j) {
            a.run_score[row0 + j] = run_new[j];
            a.fin_score[row0 + j] = fin_new[j];
            a.fin_flag[row0 + j] = flag_new[j];
            a.tok[row0 + j] = s_new_tok[j];
        }
        a.heur[b] = heur_new;
        atomicAdd(a.ctl + 2, heur_new ? 1 : 0);
        atomicAdd(a.ctl + 3, all_fin_new ? 0 : 1);
        atomicAdd(a.ctl + 4, all_hit ? 0 : 1);
    }
    __syncthreads();
    // gather parents in place: sequences [0, cur_len], beam indices [0, t], KV row tables [0, cur_len] (running rows only)
    const int t = a.cur_len - a.S0;
    gather_pass<int64_t>(b, nb, a.cur_len + 1, a.cur_len, a.seq, a.fin_seq, a.ld_seq, s_src_row, s_src_fin, s_new_tok, true);
    gather_pass<int>(b, nb, t + 1, t, a.bidx, a.fin_bidx, a.ld_bidx, s_src_row, s_src_fin, s_new_bidx, true);
    gather_pass<int>(b, nb, a.cur_len + 1, a.cur_len, a.kv_row, nullptr, a.ld_kv, s_src_row, s_src_fin, s_new_kv, false);
    // the last workgroup to finish closes or keeps the loop open for the whole batch (:3055) and resets the tallies
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(a.ctl + 5, 1) == a.B - 1) {
            __threadfence();
            const int h = atomicAdd(a.ctl + 2, 0), notfin = atomicAdd(a.ctl + 3, 0), valid = atomicAdd(a.ctl + 4, 0);
            const bool open = h > 0 && !(notfin == 0 && a.early_stopping == 1) && valid > 0;
            a.ctl[1] += 1;
            a.ctl[2] = 0; a.ctl[3] = 0; a.ctl[4] = 0; a.ctl[5] = 0;
            __threadfence();
            atomicExch(a.ctl, open ? 1 : 0);
        }
    }
}

extern "C" int egomi_beam_update(int B, int nb, int K, int V, const float* cand_key, const float* cand_score, const int32_t* cand_tok, int S0,
                                 int cur_len, int max_len, int64_t eos_id, float length_penalty, int early_stopping, int64_t* seq,
                                 int64_t* fin_seq, int64_t ld_seq, int32_t* beam_idx, int32_t* fin_beam_idx, int64_t ld_bidx, int32_t* kv_row,
                                 int64_t ld_kv, float* run_score, float* fin_score, int32_t* fin_flag, int32_t* heur, int64_t* tok,
                                 int32_t* ctl, egomi_stream_t stream) {
    if (!cand_key || !cand_score || !cand_tok || !seq || !fin_seq || !beam_idx || !fin_beam_idx || !kv_row || !run_score || !fin_score ||
        !fin_flag || !heur || !tok || !ctl) return EGOMI_E_BADARG;
    if (B <= 0 || nb <= 0 || nb > 32 || K < nb || K > BU_MAXK || nb * K > BU_MAXC || V <= 0) return EGOMI_E_SHAPE;
    if (S0 < 0 || cur_len < S0 || cur_len >= max_len || ld_seq < max_len || ld_kv < max_len || ld_bidx < max_len - S0) return EGOMI_E_SHAPE;
    if (early_stopping < 0 || early_stopping > 2) return EGOMI_E_BADARG;
    BeamUpdateArgs a;
    a.B = B; a.nb = nb; a.K = K; a.V = V; a.cand_key = cand_key; a.cand_score = cand_score; a.cand_tok = cand_tok; a.S0 = S0;
    a.cur_len = cur_len; a.max_len = max_len; a.eos = eos_id; a.length_penalty = length_penalty; a.early_stopping = early_stopping;
    a.seq = seq; a.fin_seq = fin_seq; a.ld_seq = ld_seq; a.bidx = beam_idx; a.fin_bidx = fin_beam_idx; a.ld_bidx = ld_bidx;
    a.kv_row = kv_row; a.ld_kv = ld_kv; a.run_score = run_score; a.fin_score = fin_score; a.fin_flag = fin_flag; a.heur = heur; a.tok = tok;
    a.ctl = ctl;
    EGOMI_LAUNCH(beam_update_kernel, dim3(B), dim3(BU_THREADS), 0, (hipStream_t)stream, a);
    return egomi_launch_status();
}
