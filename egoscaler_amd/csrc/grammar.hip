// Constrained decoding of trajectories (A13): generate() emits only token sequences that traj_scan (csrc/traj.hip) parses.
//
// replaces transformers/generation/logits_process.py PrefixConstrainedLogitsProcessor (generate(prefix_allowed_tokens_fn=...)): HF calls a
// Python function per row and step on the host and masks the scores with what it returns.  The trajectory grammar
//     <ts> (bin x 6 <tsep>) x n <te> eos,   min_steps <= n <= max_steps,   bin = one of the nb contiguous ids p0 .. p0 + nb - 1
// is a ten-state machine, so here the state lives in device memory and one launch per decode step, directly before the token kernel, writes
// -inf over every logit the state does not allow: no callback, no host round trip, and the launch sits inside the captured token loop.
//
// State per decoder row: int32 (phase, steps).  The ONE transition table (gr_advance / gr_allowed / gr_need below; tests/grammar_ref.py
// restates it in numpy):
//     phase 9      no <ts> seen yet              allows <ts>                      <ts>   -> (0, 0)
//     phase 0      at a step boundary, `steps`   allows bins and / or <te>        bin    -> (1, steps),  <te> -> (7, steps)
//                  steps closed
//     phase 1..5   that many bins of the open    allows bins                      bin    -> (phase + 1, steps)
//                  step seen
//     phase 6      six bins seen                 allows <tsep>                    <tsep> -> (0, steps + 1)
//     phase 7      <te> seen                     allows eos                       eos    -> (8, steps)
//     phase 8      eos seen                      allows eos                       absorbs every token
//   At phase 0, with rem = the tokens the loop still emits (this one included): bins are allowed when steps < max_steps and rem >= 9 (six
//   bins, <tsep>, <te>, eos still fit); <te> is allowed when steps >= min_steps or bins are not.  A transition looks at the token alone, never
//   at rem or the step limits; any other token leaves the state as it is (nothing checks or reports that), and a phase outside 0 .. 9 allows
//   nothing and never moves.  In phase 8 egomi_sample_rows overrides the row's token with pad anyway: the row only keeps one finite logit.
//
// need(state) = the number of tokens from the state to the earliest legal close `... <te> eos` with min_steps <= n <= max_steps:
//     (8, s) 0    (7, s) 1    (0, s) 7 max(0, min_steps - s) + 2    (p, s), 1 <= p <= 6: (6 - p) + 1 + need(0, s + 1)    (9, .) 1 + need(0, 0)
//   and EGOMI_GRAMMAR_NEVER where no legal close exists: more steps closed, or about to close, than max_steps, or a <te> taken outside
//   [min_steps, max_steps].  It is used twice: egomi_traj_grammar_init reports it per row, and generate() refuses a call whose max_length is
//   below it.  A row whose need at step 0 is at most T_new is guaranteed to end `... <te> eos` with min_steps <= n <= max_steps: below
//   min_steps need >= 9 keeps bins open, every step opened at rem >= 9 leaves rem >= 2 for <te> eos, and at rem < 9 only <te> is left.
//
// egomi_traj_grammar_init: one thread per row scans the prompt (positions with mask == 0 skipped): the state comes from the last <ts>,
//   steps = the <tsep> after it, phase = the trailing run of bins after the last <tsep> or <ts> (any other token ends a run), capped at 6;
//   no <ts>: (9, 0).  Writes state[r] and need[r].
// egomi_traj_grammar_step: one 1024-thread workgroup per row, bf16 or fp32 logits, in place.  Per row, in this order:
//   1. tok_prev != NULL: the state advances by tok_prev[r] (every thread computes it; thread 0 stores it after the row pass's barriers).
//   2. m = max x, s = sum exp(x - m) over all V RAW logits: lp_row_max_sumexp, egomi_token_logprob's pass (csrc/lp_row.h).
//   3. Z = sum exp(x_a - m) over the allowed ids in float64 in a fixed order (thread i owns bin i, block_sum2_f64 as egomi_bin_stats uses
//      it; thread 0 adds the allowed special id last); mass[r, col] = (float)Z / s, the probability the model gave the legal set -- the one
//      quantity the mask destroys.  A NaN logit in the row gives NaN; every allowed logit -inf gives 0 and the row ends all -inf.
//   4. -inf over every id of [0, V) that is not allowed.  The row's bytes are walked in 16-byte ALIGNED blocks (a row of V = 32262 bf16
//      starts 12 bytes off a line on every second row): a block that lies wholly inside [row, row + V) and holds no allowed element takes
//      one 16-byte store, every other block element stores for its elements of the row that are not allowed.  Allowed elements are never
//      written, and no byte outside [row, row + V * sizeof) is: the ld - V padding columns and the neighbouring rows stay as they are.
//   No atomics; rem and col are launch constants.  m, s and Z come from loads whose order depends on V only, and the stored bits from the
//   element index only: a row's bits depend on its values, its state and (V, spec, dtype), not on R, its slot, ld or its alignment.
//
// Motion limits (egomi_traj_grammar_init_limits / egomi_traj_grammar_step_limits): the same two kernels with one template flag.  Per row a
//   table lim int32 [18] = lo[6] | hi[6] | dmax[6] in bins and a pose int32 [12] = prev[6] | cur[6]: prev = the bins of the last CLOSED step
//   (-1: unknown), cur = the bins of the open step seen so far.  The pose moves with gr_advance's transitions and adds none: a
//   bin taken at phase p sets cur[p]; <tsep> taken at phase 6 copies cur to prev; <ts> taken at phase 9 sets prev to -1; a token that does
//   not move the phase leaves the pose alone.  (The step never clears cur: cur[p] is meaningful below the phase only.  The init kernel
//   writes -1 there.)  Where the state allows bins at phase p, dimension d = p and q = prev[d], the window of bin indices is (gr_window)
//       q < 0:  [lo, hi]           else  a = max(lo, q - dmax), b = min(hi, q + dmax)
//       a > b (q lies farther than dmax outside the box): the cap wins, a = b = min(max(e, q - dmax), q + dmax) with e = q < lo ? lo : hi
//   never empty, always inside [0, nb - 1]; lo, hi, dmax and q are clamped into range on load, so a bad table cannot move the window out of
//   the bin ids.  Everything else -- need, rem >= 9, when <te> is allowed, the special ids -- is the grammar's.  mass keeps its meaning
//   (what the grammar ALONE allows); limits_mass[r, col] is the same sum over the window: the second slot of the one block_sum2_f64 call,
//   the same float64 terms in the same order, so a full-range table gives limits_mass bit-equal to mass.  Thread 0 stores the pose after
//   the last barrier, like the state.  The init kernel commits prev at a <tsep> only when the run before it held six bins (else -1).
#include "lp_row.h"                      // lp_row_max_sumexp, block_sum2_f64: shared with csrc/logprob.hip

struct GrammarSpec {
    long long p0, ts, tsep, te, eos;
    int nb, min_steps, max_steps;
};

__device__ __forceinline__ bool gr_is_bin(long long tok, const GrammarSpec& g) { return tok >= g.p0 && tok < g.p0 + g.nb; }

__device__ __forceinline__ void gr_advance(int& phase, int& steps, long long tok, const GrammarSpec& g) {
    const bool bin = gr_is_bin(tok, g);
    if (phase == 9) {
        if (tok == g.ts) { phase = 0; steps = 0; }
    } else if (phase == 0) {
        if (bin) phase = 1;
        else if (tok == g.te) phase = 7;
    } else if (phase >= 1 && phase <= 5) {
        if (bin) ++phase;
    } else if (phase == 6) {
        if (tok == g.tsep) { phase = 0; ++steps; }
    } else if (phase == 7) {
        if (tok == g.eos) phase = 8;
    }                                                                    // 8 absorbs; anything else never moves
}

// the allowed set: the whole bin window when `bins`, plus the one special id `sp` when sp >= 0
__device__ __forceinline__ void gr_allowed(int phase, int steps, int rem, const GrammarSpec& g, bool& bins, long long& sp) {
    bins = false;
    sp = -1;
    if (phase == 9) sp = g.ts;
    else if (phase == 0) {
        bins = steps < g.max_steps && rem >= 9;
        if (steps >= g.min_steps || !bins) sp = g.te;
    } else if (phase >= 1 && phase <= 5) bins = true;
    else if (phase == 6) sp = g.tsep;
    else if (phase == 7 || phase == 8) sp = g.eos;
}

__device__ __forceinline__ int gr_need(int phase, int steps, const GrammarSpec& g) {
    const long long never = EGOMI_GRAMMAR_NEVER;
    const long long mn = g.min_steps, mx = g.max_steps;
    auto from0 = [&](long long s) { return s > mx ? never : 7 * (mn > s ? mn - s : 0) + 2; };
    long long n = never;
    if (phase == 8) n = (steps >= mn && steps <= mx) ? 0 : never;
    else if (phase == 7) n = (steps >= mn && steps <= mx) ? 1 : never;
    else if (phase == 0) n = from0(steps);
    else if (phase >= 1 && phase <= 6) n = (6 - phase) + 1 + from0((long long)steps + 1);
    else if (phase == 9) n = 1 + from0(0);
    return (int)(n < never ? n : never);
}

__device__ __forceinline__ int gr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the window [wa, wb] of bin indices for a dimension with limits (lo, hi, dmax) whose last closed step chose bin q (-1: unknown)
__device__ __forceinline__ void gr_window(int lo, int hi, int dmax, int q, int nb, int& wa, int& wb) {
    lo = gr_clamp(lo, 0, nb - 1);
    hi = gr_clamp(hi, lo, nb - 1);
    dmax = gr_clamp(dmax, 0, nb - 1);
    q = gr_clamp(q, -1, nb - 1);
    wa = lo; wb = hi;
    if (q < 0) return;
    wa = max(lo, q - dmax);
    wb = min(hi, q + dmax);
    if (wa > wb) wa = wb = min(max(q < lo ? lo : hi, q - dmax), q + dmax);
}

template <bool POSE>
__global__ __launch_bounds__(64) void traj_grammar_init_kernel(const int64_t* ids, long long ld_ids, const uint8_t* mask, long long ld_mask, int R,
                                                               int S0, GrammarSpec g, int32_t* state, int32_t* need, int32_t* pose) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int64_t* row = ids + (long long)r * ld_ids;
    const uint8_t* mk = mask ? mask + (long long)r * ld_mask : nullptr;
    bool seen = false;
    int steps = 0, run = 0;
    int prev[6], cur[6];                                                 // POSE only
    if (POSE)
        for (int d = 0; d < 6; ++d) prev[d] = cur[d] = -1;
    for (int j = 0; j < S0; ++j) {
        if (mk && mk[j] == 0) continue;
        const long long t = row[j];
        const bool bin = gr_is_bin(t, g);
        if (POSE && seen) {
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                if (t == g.ts) prev[d] = -1;
                else if (t == g.tsep) prev[d] = run == 6 ? cur[d] : -1;
                if (bin && run == d) cur[d] = (int)(t - g.p0);
                else if (!bin || t == g.ts) cur[d] = -1;                 // every token that ends a run
            }
        }
        if (t == g.ts) { seen = true; steps = 0; run = 0; }
        else if (!seen) continue;
        else if (t == g.tsep) { ++steps; run = 0; }
        else if (bin) { if (run < 6) ++run; }
        else run = 0;
    }
    if (POSE)
        for (int d = 0; d < 6; ++d) { pose[12 * r + d] = prev[d]; pose[12 * r + 6 + d] = cur[d]; }
    const int phase = seen ? run : 9;
    if (!seen) steps = 0;
    state[2 * r] = phase;
    state[2 * r + 1] = steps;
    need[r] = gr_need(phase, steps, g);
}

struct GrammarStepArgs {
    void* logits; long long ld; int V;
    const int64_t* tok_prev; int32_t* state;
    GrammarSpec g; int rem;
    float* mass; long long ld_mass; int col;
    const int32_t* lim; int32_t* pose; float* limits_mass;              // the LIM kernels only
};

template <typename T> struct NegInf;
template <> struct NegInf<bf16_t> { static constexpr bf16_t one = 0xFF80u; static constexpr uint32_t word = 0xFF80FF80u; };
template <> struct NegInf<float> { static constexpr uint32_t word = 0xFF800000u; };
__device__ __forceinline__ void gr_store_ninf(bf16_t* p) { *p = NegInf<bf16_t>::one; }
__device__ __forceinline__ void gr_store_ninf(float* p) { *p = -INFINITY; }

template <typename T, bool REG, bool LIM>
__global__ __launch_bounds__(LPB_THREADS) void traj_grammar_step_kernel(GrammarStepArgs a) {
    __shared__ float red[16];
    __shared__ double red2[32];
    const int r = blockIdx.x, tid = threadIdx.x, V = a.V;
    int phase = a.state[2 * r], steps = a.state[2 * r + 1];             // read by every thread before the first barrier; stored after the last
    // LIM: the row's whole table and pose, loaded here beside the state: their addresses depend on r alone, so they travel with the state's
    // load and not, entry by entry, behind the phase it yields (three more dependent round trips in front of the row pass)
    int lm[18], ps0[12];
    if (LIM) {
#pragma unroll
        for (int i = 0; i < 18; ++i) lm[i] = a.lim[18 * (long long)r + i];
#pragma unroll
        for (int i = 0; i < 12; ++i) ps0[i] = a.pose[12 * (long long)r + i];
    }
    const int phase0 = phase;
    if (a.tok_prev) gr_advance(phase, steps, a.tok_prev[r], a.g);
    bool bins;
    long long sp;
    gr_allowed(phase, steps, a.rem, a.g, bins, sp);
    // LIM: what the token does to the pose (stored by thread 0 below), and the window [wa, wb] of bin indices under the moved pose
    const bool moved = LIM && a.tok_prev && phase != phase0;
    const bool set_cur = moved && phase0 >= 0 && phase0 <= 5 && phase == phase0 + 1;       // a bin taken at phase0
    const bool commit = moved && phase0 == 6;                                                // <tsep>: prev = cur
    const bool reset = moved && phase0 == 9;                                                 // <ts>: prev = -1
    int wa = 0, wb = a.g.nb - 1;
    if (LIM && bins) {
#pragma unroll
        for (int d = 0; d < 6; ++d)                                      // (selects: the arrays stay in registers)
            if (d == phase) gr_window(lm[d], lm[6 + d], lm[12 + d], reset ? -1 : (commit ? ps0[6 + d] : ps0[d]), a.g.nb, wa, wb);
    }
    T* lg = (T*)a.logits + (long long)r * a.ld;
    float m, s;
    lp_row_max_sumexp<T, REG>(lg, V, red, m, s);
    double Z = 0.0, Zw = 0.0;                                            // Zw: the same terms over the window (LIM; else unused)
    if (bins && tid < a.g.nb) {
        const float xi = Cvt<T>::ld(lg + a.g.p0 + tid);
        Z = (double)(xi == -INFINITY ? 0.f : expf(xi - m));
        if (LIM && tid >= wa && tid <= wb) Zw = Z;
    }
    block_sum2_f64(Z, Zw, red2);                                         // (after its barriers every load of the row pass has completed)
    if (tid == 0) {
        if (sp >= 0) {
            const float xs = Cvt<T>::ld(lg + sp);
            const double zs = (double)(xs == -INFINITY ? 0.f : expf(xs - m));
            Z += zs;
            Zw += zs;
        }
        a.mass[(long long)r * a.ld_mass + a.col] = (float)Z / s;
        if (a.tok_prev) { a.state[2 * r] = phase; a.state[2 * r + 1] = steps; }
        if (LIM) {
            a.limits_mass[(long long)r * a.ld_mass + a.col] = (float)Zw / s;
            int32_t* ps = a.pose + 12 * (long long)r;
            if (set_cur) ps[6 + phase0] = (int32_t)(a.tok_prev[r] - a.g.p0);
            if (commit || reset) {
#pragma unroll
                for (int d = 0; d < 6; ++d) ps[d] = commit ? ps0[6 + d] : -1;
            }
        }
    }
    // the mask: 16-byte aligned blocks of the row's bytes, block k at base + 16 k
    constexpr int EPB = 16 / (int)sizeof(T);
    const uintptr_t row = (uintptr_t)lg, row_end = row + (uintptr_t)V * sizeof(T), base = row & ~(uintptr_t)15;
    const long long nblk = (long long)((row_end - base + 15) >> 4);
    const long long a0 = bins ? a.g.p0 + (LIM ? wa : 0) : 0, a1 = bins ? a.g.p0 + (LIM ? wb + 1 : a.g.nb) : 0;     // the allowed window [a0, a1)
    const u32x4 ninf4 = {NegInf<T>::word, NegInf<T>::word, NegInf<T>::word, NegInf<T>::word};
    for (long long k = tid; k < nblk; k += LPB_THREADS) {
        const uintptr_t blk = base + (uintptr_t)k * 16;
        const long long e0 = ((long long)blk - (long long)row) / (long long)sizeof(T);   // its first element's index; negative in block 0 only
        const bool whole = blk >= row && blk + 16 <= row_end;
        const bool hit = (e0 < a1 && e0 + EPB > a0) || (sp >= e0 && sp < e0 + EPB);
        if (whole && !hit) {
            *reinterpret_cast<u32x4*>(blk) = ninf4;
        } else {
            for (int j = 0; j < EPB; ++j) {
                const long long e = e0 + j;
                if (e >= 0 && e < V && !(e >= a0 && e < a1) && e != sp) gr_store_ninf(lg + e);
            }
        }
    }
}

static int gr_check_spec(int64_t p0, int nb, int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, GrammarSpec& g) {
    if (nb < 1 || nb > LPB_THREADS || p0 < 0 || min_steps < 0 || min_steps > max_steps) return EGOMI_E_SHAPE;
    const int64_t sp[4] = {ts, tsep, te, eos};
    for (int i = 0; i < 4; ++i) {
        if (sp[i] < 0 || (sp[i] >= p0 && sp[i] < p0 + nb)) return EGOMI_E_SHAPE;
        for (int j = 0; j < i; ++j)
            if (sp[i] == sp[j]) return EGOMI_E_SHAPE;
    }
    g.p0 = p0; g.nb = nb; g.ts = ts; g.tsep = tsep; g.te = te; g.eos = eos; g.min_steps = min_steps; g.max_steps = max_steps;
    return EGOMI_OK;
}

template <bool POSE>
static int gr_init(const int64_t* ids, int64_t ld_ids, const uint8_t* mask, int64_t ld_mask, int R, int S0, int64_t p0, int nb, int64_t ts, int64_t tsep,
                   int64_t te, int64_t eos, int min_steps, int max_steps, int32_t* state, int32_t* need, int32_t* pose, egomi_stream_t stream) {
    if (!ids || !state || !need || (POSE && !pose)) return EGOMI_E_BADARG;
    if (R <= 0 || S0 <= 0 || ld_ids < S0 || (mask && ld_mask < S0)) return EGOMI_E_SHAPE;
    GrammarSpec g;
    const int rc = gr_check_spec(p0, nb, ts, tsep, te, eos, min_steps, max_steps, g);
    if (rc != EGOMI_OK) return rc;
    EGOMI_LAUNCH(traj_grammar_init_kernel<POSE>, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, ids, (long long)ld_ids, mask,
                 (long long)ld_mask, R, S0, g, state, need, pose);
    return egomi_launch_status();
}

extern "C" int egomi_traj_grammar_init(const int64_t* ids, int64_t ld_ids, const uint8_t* mask, int64_t ld_mask, int R, int S0, int64_t p0, int nb,
                                       int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int32_t* state,
                                       int32_t* need, egomi_stream_t stream) {
    return gr_init<false>(ids, ld_ids, mask, ld_mask, R, S0, p0, nb, ts, tsep, te, eos, min_steps, max_steps, state, need, nullptr, stream);
}

extern "C" int egomi_traj_grammar_init_limits(const int64_t* ids, int64_t ld_ids, const uint8_t* mask, int64_t ld_mask, int R, int S0, int64_t p0,
                                              int nb, int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps,
                                              int32_t* state, int32_t* need, int32_t* pose, egomi_stream_t stream) {
    return gr_init<true>(ids, ld_ids, mask, ld_mask, R, S0, p0, nb, ts, tsep, te, eos, min_steps, max_steps, state, need, pose, stream);
}

template <bool LIM>
static int gr_step(void* logits, int64_t ld, int R, int V, const int64_t* tok_prev, int32_t* state, int64_t p0, int nb, int64_t ts, int64_t tsep,
                   int64_t te, int64_t eos, int min_steps, int max_steps, int rem, float* mass, int64_t ld_mass, int col, const int32_t* lim,
                   int32_t* pose, float* limits_mass, int dtype, egomi_stream_t stream) {
    if (!logits || !state || !mass || (LIM && (!lim || !pose || !limits_mass))) return EGOMI_E_BADARG;
    if (dtype != EGOMI_F32 && dtype != EGOMI_BF16) return EGOMI_E_BADARG;
    if (R <= 0 || V <= 0 || ld < V || rem < 1 || col < 0 || ld_mass <= col) return EGOMI_E_SHAPE;
    GrammarStepArgs a;
    const int rc = gr_check_spec(p0, nb, ts, tsep, te, eos, min_steps, max_steps, a.g);
    if (rc != EGOMI_OK) return rc;
    if (p0 + nb > V || ts >= V || tsep >= V || te >= V || eos >= V) return EGOMI_E_SHAPE;
    if (((uintptr_t)logits) % (dtype == EGOMI_F32 ? 4 : 2)) return EGOMI_E_UNSUPPORTED;      // elements must be naturally aligned
    a.logits = logits; a.ld = ld; a.V = V; a.tok_prev = tok_prev; a.state = state; a.rem = rem; a.mass = mass; a.ld_mass = ld_mass; a.col = col;
    a.lim = lim; a.pose = pose; a.limits_mass = limits_mass;
    if (V <= LPB_THREADS * LPB_NPT) EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((traj_grammar_step_kernel<T, true, LIM>), dim3(R), dim3(LPB_THREADS), 0, (hipStream_t)stream, a));
    else EGOMI_DISPATCH_DTYPE(dtype, EGOMI_LAUNCH((traj_grammar_step_kernel<T, false, LIM>), dim3(R), dim3(LPB_THREADS), 0, (hipStream_t)stream, a));
    return egomi_launch_status();
}

extern "C" int egomi_traj_grammar_step(void* logits, int64_t ld, int R, int V, const int64_t* tok_prev, int32_t* state, int64_t p0, int nb, int64_t ts,
                                       int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int rem, float* mass, int64_t ld_mass,
                                       int col, int dtype, egomi_stream_t stream) {
    return gr_step<false>(logits, ld, R, V, tok_prev, state, p0, nb, ts, tsep, te, eos, min_steps, max_steps, rem, mass, ld_mass, col, nullptr, nullptr,
                          nullptr, dtype, stream);
}

extern "C" int egomi_traj_grammar_step_limits(void* logits, int64_t ld, int R, int V, const int64_t* tok_prev, int32_t* state, int64_t p0, int nb,
                                              int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int rem, float* mass,
                                              int64_t ld_mass, int col, const int32_t* lim, int32_t* pose, float* limits_mass, int dtype,
                                              egomi_stream_t stream) {
    return gr_step<true>(logits, ld, R, V, tok_prev, state, p0, nb, ts, tsep, te, eos, min_steps, max_steps, rem, mass, ld_mass, col, lim, pose,
                         limits_mass, dtype, stream);
}
