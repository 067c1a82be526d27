"""Cached greedy decoding (A13) with static buffers and optional hipGraph capture.

Reference behaviour: model_arch.py:77-108 -> HF generate: one prefill (point encoder + splice,
pointllm.py:112-171) that fills the KV cache, then single-token steps (pointllm.py:255-275).
Here the prefill is Engine.forward_hidden with a kv_sink; each later step runs
  embed -> 32 x {rmsnorm, q/k/v GEMMs, RoPE(pos), kv_append, attn_decode, o_proj, rmsnorm, SwiGLU MLP}
  -> final norm -> lm_head -> argmax
on static buffers.  Every length is a launch argument, so T steps are captured into ONE hipGraph
(BASELINE.json config 5) and replayed with a single launch; token ids never leave the device.
"""
import contextlib
import gc
import os

import torch

from . import lora, ops
from ._lib import call
from .ops import S, dt


@contextlib.contextmanager
def _capture(g):
    """Capture the block into CUDAGraph g on a side stream, with the cyclic garbage collector off.  This torch does not collect before a
    capture, so a collection could start inside one and run the finalizers of whatever unrelated objects it frees (a dropped model's
    graphs, events, memory pools); their HIP calls are illegal during a capture and abort the process (a beam-search capture aborted with
    the main thread inside such a collection).  Garbage is collected after the capture instead."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                yield
    finally:
        if enabled:
            gc.enable()
    torch.cuda.current_stream().wait_stream(side)


def kv_append(k, v, ld, kc, vc, B, Sq, H, hd, Smax, pos0):
    call("egomi_kv_append", k, v, ld, kc, vc, B, Sq, H, hd, Smax, pos0, dt(k.dtype), S())


def attn_decode(q, ld_q, kc, vc, key_mask, out, B, H, hd, Smax, T_len, scale):
    call("egomi_attn_decode", q, ld_q, kc, vc, key_mask, key_mask.stride(0) if key_mask is not None else 0, out, out.stride(0), B, H, hd, Smax, T_len,
         scale, dt(q.dtype), S())


def kv_append_fp8(k, v, ld, kc, vc, ks, vs, B, Sq, H, hd, Smax, pos0):
    """kv_append into the fp8 cache: codes kc / vc uint8 [B, H, Smax, hd], scales ks / vs fp32 [B, H, Smax] (include/egomi.h egomi_kv_append_fp8)."""
    call("egomi_kv_append_fp8", k, v, ld, kc, vc, ks, vs, B, Sq, H, hd, Smax, pos0, dt(k.dtype), S())


def attn_decode_fp8(q, ld_q, kc, vc, ks, vs, key_mask, out, B, H, hd, Smax, T_len, scale):
    """attn_decode over the fp8 cache (include/egomi.h egomi_attn_decode_fp8)."""
    call("egomi_attn_decode_fp8", q, ld_q, kc, vc, ks, vs, key_mask, key_mask.stride(0) if key_mask is not None else 0, out, out.stride(0), B, H, hd,
         Smax, T_len, scale, dt(q.dtype), S())


def kv8_quantize(x):
    """The fp8 cache's numerics restated in torch (csrc/kv8.hip header): x [..., hd] -> (codes uint8 [..., hd], scales fp32 [...]),
    s = amax / 448 (1 where amax == 0), codes = (x / s).to(float8_e4m3fn).  The kernels are bit-equal to it."""
    x = x.float()
    s = x.abs().amax(-1) / 448.0
    s = torch.where(s == 0, torch.ones_like(s), s)
    return (x / s[..., None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def kv8_dequantize(codes, scales):
    """float(code) * s, fp32."""
    return codes.view(torch.float8_e4m3fn).float() * scales[..., None]


def w8_quantize(w):
    """The fp8 decode weights' numerics restated in torch (csrc/w8.hip header): rows w [N, K] -> (codes uint8 [N, K], scales fp32 [N]),
    s_n = amax_n / 448 (1 where amax == 0), codes = (w.float() / s[:, None]).to(float8_e4m3fn).  egomi_quantize_rows_fp8 is bit-equal to it."""
    w = w.float()
    s = w.abs().amax(1) / 448.0
    s = torch.where(s == 0, torch.ones_like(s), s)
    return (w / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), s


W4_GROUP = 128                                       # columns per scale group of the int4 decode weights


def w4_quantize(w):
    """The int4 decode weights' numerics restated in torch on the host (csrc/w4.hip header): rows w [N, K], K % 32 == 0 -> (packed uint8
    [N, K / 2], scales fp32 [NG, N]).  Group g = columns [128 g, min(K, 128 g + 128)), NG = ceil(K / 128); s[g, n] = amax / 7 (1 where
    amax == 0), code = clamp(round(w / s), -7, 7) (torch.round: ties to even), stored as the nibble code + 8 in the natural order: byte b
    of a row holds column 2 b in its low nibble and column 2 b + 1 in its high nibble.
    egomi_quantize_rows_int4 is bit-equal to it (run it on the host: a device's division need not be correctly rounded)."""
    w = w.float()
    N, K = w.shape
    if K % 32:
        raise ValueError(f"w4_quantize: K = {K} is not a multiple of 32")
    NG = -(-K // W4_GROUP)
    wp = torch.zeros(N, NG * W4_GROUP, dtype=torch.float32, device=w.device)
    wp[:, :K] = w
    s = wp.view(N, NG, W4_GROUP).abs().amax(2) / 7.0
    s = torch.where(s == 0, torch.ones_like(s), s)
    codes = torch.round(wp.view(N, NG, W4_GROUP) / s[:, :, None]).clamp_(-7, 7).view(N, -1)[:, :K]
    nib = codes.to(torch.int32) + 8
    packed = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8)
    return packed.contiguous(), s.t().contiguous()


def w4_unpack(packed, K):
    """packed uint8 [N, K / 2] -> the codes int8 [N, K] (-7 .. 7; nibble - 8) in column order: w4_quantize's packing undone."""
    b = packed[:, :K // 2].to(torch.int32)
    return (torch.stack([b & 15, b >> 4], 2).view(packed.shape[0], K) - 8).to(torch.int8)


def w4_dequantize(packed, scales, K):
    """code * s[group, row], fp32 [N, K]."""
    s = scales.t().repeat_interleave(W4_GROUP, 1)[:, :K]
    return w4_unpack(packed, K).float() * s


def argmax_rows(logits, ids, seq=None, pos=0):
    B, V = logits.shape
    call("egomi_argmax_rows", logits, logits.stride(0), B, V, ids, seq, seq.stride(0) if seq is not None else 0, pos, dt(logits.dtype), S())


def sample_rows(logits, scores, seq, pos, rep_from, ids, done, repetition_penalty, temperature, top_k, top_p, do_sample, rng, draw, eos, pad):
    """One step's token choice for the whole batch (include/egomi.h egomi_sample_rows): processed scores (HF's `.scores`) + next token."""
    B, V = logits.shape
    call("egomi_sample_rows", logits, logits.stride(0), B, V, scores, scores.stride(0), seq, seq.stride(0) if seq is not None else 0, pos, rep_from,
         ids, done, repetition_penalty, temperature, int(top_k or 0), top_p, int(bool(do_sample)), rng, draw, -1 if eos is None else int(eos),
         0 if pad is None else int(pad), dt(logits.dtype), S())


def token_logprob(logits, tok, eos, live, tok_lp, col, sum_lp, n_tok):
    """The log-prob of this step's chosen token under the RAW logits, per row (include/egomi.h egomi_token_logprob): tok_lp[:, col], and the
    running sum_lp / n_tok; live (int32 [R] or None) stops a row's count after its eos."""
    R, V = logits.shape
    call("egomi_token_logprob", logits, logits.stride(0), R, V, tok, -1 if eos is None else int(eos), live, tok_lp, tok_lp.stride(0), col, sum_lp,
         n_tok, dt(logits.dtype), S())


def bin_stats_rows(logits, p0, nb, values, mass, mean, std, ent, col):
    """The step's distribution over the bin tokens p0 .. p0 + nb - 1 (values float64 [nb]) under the RAW logits, per row (include/egomi.h
    egomi_bin_stats): mass / mean / std / ent [:, col]."""
    R, V = logits.shape
    call("egomi_bin_stats", logits, logits.stride(0), R, V, p0, nb, values, mass, mean, std, ent, mass.stride(0), col, dt(logits.dtype), S())


def bin_window(bin_token_ids, V):
    """(p0, nb) of `bin_token_ids`, checked against a vocabulary of V ids (egomi_bin_stats' limits, raised before any launch)."""
    try:
        p0, nb = (int(v) for v in bin_token_ids)
    except (TypeError, ValueError):
        raise ValueError(f"`bin_token_ids` must be (first bin id, number of bins), not {bin_token_ids!r}") from None
    if not 1 <= nb <= 1024 or p0 < 0 or p0 + nb > V:
        raise ValueError(f"`bin_token_ids` = ({p0}, {nb}) is not a window of 1 .. 1024 ids inside the vocabulary of {V}")
    return p0, nb


GRAMMAR_FIELDS = ("p0", "nb", "ts", "tsep", "te", "eos", "min_steps", "max_steps")


def grammar_check(spec, V):
    """The eight integers (GRAMMAR_FIELDS) of a trajectory grammar spec (traj.grammar_spec), checked against a vocabulary of V ids
    (the limits of egomi_traj_grammar_step, raised before any launch)."""
    try:
        g = tuple(int(getattr(spec, f)) for f in GRAMMAR_FIELDS) if hasattr(spec, "p0") else tuple(int(v) for v in spec)
        p0, nb, ts, tsep, te, eos, mn, mx = g
    except (TypeError, ValueError, AttributeError):
        raise ValueError(f"a trajectory grammar is traj.grammar_spec(tok, min_steps, max_steps), not {spec!r}") from None
    if not 1 <= nb <= 1024 or p0 < 0 or p0 + nb > V:
        raise ValueError(f"grammar: the bin window ({p0}, {nb}) is not 1 .. 1024 ids inside the vocabulary of {V}")
    sp = (ts, tsep, te, eos)
    if any(not 0 <= s < V or p0 <= s < p0 + nb for s in sp) or len(set(sp)) != 4:
        raise ValueError(f"grammar: <ts>, <tsep>, <te>, eos = {sp} must be four different ids of the vocabulary of {V} outside the bin window")
    if not 0 <= mn <= mx:
        raise ValueError(f"grammar: 0 <= min_steps <= max_steps does not hold for ({mn}, {mx})")
    return g


def traj_grammar_init(ids, mask, spec, state, need):
    """The grammar state every prompt row leaves and the tokens it needs to close (include/egomi.h egomi_traj_grammar_init): ids int64
    [R, S0] and mask uint8 [R, S0] or None (views with a row stride are fine) -> state int32 [R, 2], need int32 [R]."""
    R, S0 = ids.shape
    p0, nb, ts, tsep, te, eos, mn, mx = spec
    call("egomi_traj_grammar_init", ids, ids.stride(0), mask, mask.stride(0) if mask is not None else 0, R, S0, p0, nb, ts, tsep, te, eos, mn, mx,
         state, need, S())


def traj_grammar_step(logits, tok_prev, state, spec, rem, mass, col):
    """One step of the trajectory grammar, in place on `logits` [R, V] (include/egomi.h egomi_traj_grammar_step): the state advances by
    tok_prev (None at step 0), mass[:, col] = the raw probability of the allowed set, and every other id becomes -inf.  rem = the tokens
    the loop still emits, this one included."""
    R, V = logits.shape
    p0, nb, ts, tsep, te, eos, mn, mx = spec
    call("egomi_traj_grammar_step", logits, logits.stride(0), R, V, tok_prev, state, p0, nb, ts, tsep, te, eos, mn, mx, rem, mass, mass.stride(0),
         col, dt(logits.dtype), S())


def traj_limits_check(lim, nb, rows):
    """The motion-limits table of sample() / greedy() / generate(traj_limits=...) (traj.motion_limits), checked on the host before any
    launch: `lim` is a CPU integer tensor or array [rows, 18] = lo[6] | hi[6] | dmax[6] in bins with 0 <= lo <= hi <= nb - 1 and
    0 <= dmax <= nb - 1 (include/egomi.h egomi_traj_grammar_step_limits).  -> the table as a contiguous CPU int32 tensor.  It reads no
    device memory: a table that lives on a device is refused, not fetched."""
    if isinstance(lim, torch.Tensor):
        if lim.is_cuda:
            raise ValueError("traj_limits: the table is checked on the host; pass a CPU tensor or array, not a device tensor")
        if lim.is_floating_point() or lim.dtype == torch.bool:
            raise ValueError(f"traj_limits: an integer table of bins, not {lim.dtype}")
        t = lim.detach().to(torch.int64)
    else:
        import numpy as np
        a = np.asarray(lim)
        if a.dtype.kind not in "iu":
            raise ValueError(f"traj_limits: an integer table of bins, not {a.dtype}")
        t = torch.from_numpy(a.astype(np.int64))
    if t.dim() != 2 or tuple(t.shape) != (int(rows), 18):
        raise ValueError(f"traj_limits: the table is [{int(rows)}, 18] = lo[6] | hi[6] | dmax[6] per row, not {list(t.shape)}")
    if bool(((t < 0) | (t > nb - 1)).any()):
        raise ValueError(f"traj_limits: every entry is a number of bins in [0, {nb - 1}]")
    if bool((t[:, 0:6] > t[:, 6:12]).any()):
        raise ValueError("traj_limits: lo <= hi does not hold in every row and dimension")
    return t.to(torch.int32).contiguous()


def traj_grammar_init_limits(ids, mask, spec, state, need, pose):
    """traj_grammar_init, and pose int32 [R, 12] = prev[6] | cur[6] from the prompt (include/egomi.h egomi_traj_grammar_init_limits)."""
    R, S0 = ids.shape
    p0, nb, ts, tsep, te, eos, mn, mx = spec
    call("egomi_traj_grammar_init_limits", ids, ids.stride(0), mask, mask.stride(0) if mask is not None else 0, R, S0, p0, nb, ts, tsep, te, eos,
         mn, mx, state, need, pose, S())


def traj_grammar_step_limits(logits, tok_prev, state, spec, rem, mass, col, lim, pose, limits_mass):
    """traj_grammar_step under the motion limits lim int32 [R, 18] (include/egomi.h egomi_traj_grammar_step_limits): the bin window of a
    row narrows to its limits around pose's last closed step, the pose moves with the state, and limits_mass[:, col] = the raw
    probability of what is allowed under the limits (mass[:, col] stays what the grammar alone allows).  limits_mass has mass's stride."""
    R, V = logits.shape
    p0, nb, ts, tsep, te, eos, mn, mx = spec
    assert lim.is_contiguous() and pose.is_contiguous() and limits_mass.stride(0) == mass.stride(0)
    call("egomi_traj_grammar_step_limits", logits, logits.stride(0), R, V, tok_prev, state, p0, nb, ts, tsep, te, eos, mn, mx, rem, mass,
         mass.stride(0), col, lim, pose, limits_mass, dt(logits.dtype), S())


def seq_rank(sum_lp, n_tok, B, K, length_penalty=1.0):
    """Per clip, the K rows b * K + j by descending sum_lp / n_tok ** length_penalty (include/egomi.h egomi_seq_rank):
    -> (score fp32 [B, K], order int32 [B, K])."""
    sum_lp, n_tok = sum_lp.to(torch.float32).contiguous(), n_tok.to(torch.int32).contiguous()
    if sum_lp.numel() != B * K or n_tok.numel() != B * K:
        raise ValueError(f"sum_lp / n_tok must hold B * K = {B * K} rows")
    score = torch.empty(B, K, dtype=torch.float32, device=sum_lp.device)
    order = torch.empty(B, K, dtype=torch.int32, device=sum_lp.device)
    call("egomi_seq_rank", sum_lp, n_tok, B, K, float(length_penalty), score, order, S())
    return score, order


def beam_rows(logits, lg_div, R, nb, scores, seq, pos, repetition_penalty, temperature, top_k, top_p, min_keep, do_sample, rng, draw, run_score,
              cand_key, cand_score, cand_tok, ctl):
    """One beam step's row pass (include/egomi.h egomi_beam_rows): processed log-probs (HF's `.scores`) + each row's K best candidates."""
    V = logits.shape[1]
    call("egomi_beam_rows", logits, logits.stride(0), lg_div, R, V, nb, scores, scores.stride(0), seq, seq.stride(0) if seq is not None else 0, pos,
         repetition_penalty, temperature, int(top_k or 0), top_p, min_keep, int(bool(do_sample)), rng, draw, run_score, cand_key.shape[1], cand_key,
         cand_score, cand_tok, ctl, dt(logits.dtype), S())


def beam_update(B, nb, V, cand_key, cand_score, cand_tok, S0, cur_len, max_len, eos, length_penalty, early_stopping, seq, fin_seq, bidx, fin_bidx,
                kv_row, run_score, fin_score, fin_flag, heur, tok, ctl):
    """One beam step's per-item update (include/egomi.h egomi_beam_update).  early_stopping: False / True / "never"."""
    es = 2 if early_stopping == "never" else int(bool(early_stopping))
    call("egomi_beam_update", B, nb, cand_key.shape[1], V, cand_key, cand_score, cand_tok, S0, cur_len, max_len, -1 if eos is None else int(eos),
         length_penalty, es, seq, fin_seq, seq.stride(0), bidx, fin_bidx, bidx.stride(0), kv_row, kv_row.stride(0), run_score, fin_score, fin_flag,
         heur, tok, ctl, S())


def attn_decode_rows(q, ld_q, kc, vc, kv_row, n_phys, key_mask, out, B, nb, H, hd, Smax, T_len, scale):
    """attn_decode with key t of logical row r read from physical cache row kv_row[r, t] (include/egomi.h egomi_attn_decode_rows)."""
    call("egomi_attn_decode_rows", q, ld_q, kc, vc, kv_row, kv_row.stride(0), n_phys, key_mask, key_mask.stride(0) if key_mask is not None else 0,
         out, out.stride(0), B, nb, H, hd, Smax, T_len, scale, dt(q.dtype), S())


def attn_decode_rows_fp8(q, ld_q, kc, vc, ks, vs, kv_row, n_phys, key_mask, out, B, nb, H, hd, Smax, T_len, scale):
    """attn_decode_rows over the fp8 cache (include/egomi.h egomi_attn_decode_rows_fp8)."""
    call("egomi_attn_decode_rows_fp8", q, ld_q, kc, vc, ks, vs, kv_row, kv_row.stride(0), n_phys, key_mask,
         key_mask.stride(0) if key_mask is not None else 0, out, out.stride(0), B, nb, H, hd, Smax, T_len, scale, dt(q.dtype), S())


def attn_decode_shared(q, ld_q, kp, vp, key_mask, ks, vs, out, B, K, H, hd, Sp, S0, Tmax, T_len, scale):
    """Attention of the B * K logical rows r = b * K + j over clip b's prompt cache kp / vp [B, H, Sp, hd] (keys 0 .. S0-1, key_mask
    [B, >= S0]) and the row's own suffix cache ks / vs [B*K, H, Tmax, hd] (keys 0 .. T_len-1)  (include/egomi.h egomi_attn_decode_shared)."""
    call("egomi_attn_decode_shared", q, ld_q, kp, vp, key_mask, key_mask.stride(0) if key_mask is not None else 0, ks, vs, out, out.stride(0), B, K,
         H, hd, Sp, S0, Tmax, T_len, scale, dt(q.dtype), S())


def attn_decode_shared_rows(q, ld_q, kp, vp, key_mask, ks, vs, sfx_row, n_phys, out, B, K, H, hd, Sp, S0, Tmax, T_len, scale):
    """attn_decode_shared with suffix key t of logical row r read from physical suffix row sfx_row[r, t] of ks / vs [n_phys, H, Tmax, hd]
    (beam search on the split cache; entries outside [0, n_phys) are masked keys)  (include/egomi.h egomi_attn_decode_shared_rows)."""
    call("egomi_attn_decode_shared_rows", q, ld_q, kp, vp, key_mask, key_mask.stride(0) if key_mask is not None else 0, ks, vs, sfx_row,
         sfx_row.stride(0) if sfx_row is not None else 0, n_phys, out, out.stride(0), B, K, H, hd, Sp, S0, Tmax, T_len, scale, dt(q.dtype), S())


def attn_suffix_shared(q, ld_q, kp, vp, key_mask, ks, vs, out, B, K, H, hd, Sp, S0, Tmax, T, scale):
    """The suffix pass of attn_decode_shared: the B * K * T queries (b * K + j) * T + t over clip b's prompt cache, then keys 0 .. t of
    suffix row b * K + j (causal)  (include/egomi.h egomi_attn_suffix_shared)."""
    call("egomi_attn_suffix_shared", q, ld_q, kp, vp, key_mask, key_mask.stride(0) if key_mask is not None else 0, ks, vs, out, out.stride(0), B, K,
         H, hd, Sp, S0, Tmax, T, scale, dt(q.dtype), S())


def candidate_lengths(cand, eos):
    """The tokens of every candidate that score() counts: cand [..., T] token ids (any device) -> int32 [...]: through the first `eos`
    inclusive, T where there is none, and T everywhere with eos=None (egomi_token_logprob's `live` rule, restated on whole rows)."""
    T = cand.shape[-1]
    if eos is None:
        return torch.full(cand.shape[:-1], T, dtype=torch.int32, device=cand.device)
    hit = cand == int(eos)
    first = hit.int().argmax(-1) + 1                        # (argmax: the first of equal maxima)
    return torch.where(hit.any(-1), first, torch.full_like(first, T)).to(torch.int32)


class DenseCache:
    """The KV cache of B decoder rows in the model's dtype: kc / vc [L, B, H, Smax, hd], one row of Smax keys per decoder row.

    The three cache classes are what Decoder knows about a layout.  Each owns its tensors (tensors()) and has
      G, fused_qkv          decoder rows per prompt row; whether qkv_finish() exists
      begin(S0, total_new)  a prefill of S0 prompt tokens and then total_new steps start (raises if they do not fit)
      append_prompt(l, qkv, B, Sq, row=None)   prefill: k | v of B * Sq post-RoPE q|k|v rows -> positions 0 .. Sq-1 of layer l, of prompt
                            rows 0 .. B-1 or (B = 1) of prompt row `row`
      append_step(l, qkv, pos)                 step: k | v of the B rows' q|k|v -> position pos
      qkv_finish(l, ws, n, qkv, cos, sin, pos) the fused sum of n slabs + RoPE(pos) + append_step (egomi_qkv_finish*)
      attend(l, pos, qkv, mask, out, kv_row, nb)   the B queries in qkv over keys 0 .. pos of layer l -> out; kv_row (beam mode, nb beams
                            per item): key t of row r lives in physical row kv_row[r, t]"""
    G, fused_qkv, names = 1, True, ("kc", "vc")
    _append_op, _attend_op, _attend_rows_op, _finish_op = map(staticmethod, (kv_append, attn_decode, attn_decode_rows, ops.qkv_finish))

    def __init__(self, lm, B, Smax, dtype, dev):
        self.B, self.H, self.hd, self.Smax = B, lm.num_attention_heads, lm.head_dim, Smax
        self.kc = torch.zeros(lm.num_hidden_layers, B, self.H, Smax, self.hd, dtype=dtype, device=dev)
        self.vc = torch.zeros_like(self.kc)

    def tensors(self):
        return tuple(getattr(self, n) for n in self.names)

    def begin(self, S0, total_new):
        pass

    def _append(self, sel, qkv, B, Sq, pos0):
        d = self.H * self.hd
        self._append_op(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv.stride(0), *(t[sel] for t in self.tensors()), B, Sq, self.H, self.hd, self.Smax, pos0)

    def append_prompt(self, l, qkv, B, Sq, row=None):
        self._append((l,) if row is None else (l, row), qkv, B, Sq, 0)

    def append_step(self, l, qkv, pos):
        self._append((l,), qkv, self.B, 1, pos)

    def qkv_finish(self, l, ws, n, qkv, cos, sin, pos):
        self._finish_op(ws, n, qkv, cos, sin, pos, *(t[l] for t in self.tensors()), self.B, self.H, self.hd, self.Smax)

    def attend(self, l, pos, qkv, mask, out, kv_row, nb):
        B, tail = self.B, (self.H, self.hd, self.Smax, pos + 1, self.hd ** -0.5)
        kv = tuple(t[l] for t in self.tensors())
        if kv_row is None:
            self._attend_op(qkv, qkv.stride(0), *kv, mask, out, B, *tail)
        else:
            self._attend_rows_op(qkv, qkv.stride(0), *kv, kv_row, B, mask, out, B, nb, *tail)


class Fp8Cache(DenseCache):
    """DenseCache in e4m3fn codes kc / vc uint8 [L, B, H, Smax, hd] with fp32 scales ks / vs [L, B, H, Smax], one per (layer, row, head,
    position) and tensor (csrc/kv8.hip).  The fp8 entry points take the scales right after the codes: the order of `names`."""
    names = ("kc", "vc", "ks", "vs")
    _append_op, _attend_op, _attend_rows_op, _finish_op = map(staticmethod, (kv_append_fp8, attn_decode_fp8, attn_decode_rows_fp8, ops.qkv_finish_fp8))

    def __init__(self, lm, B, Smax, dtype, dev):
        super().__init__(lm, B, Smax, torch.uint8, dev)
        self.ks = torch.zeros(lm.num_hidden_layers, B, self.H, Smax, dtype=torch.float32, device=dev)
        self.vs = torch.zeros_like(self.ks)


class SplitCache:
    """Prompt cache kp / vp [L, B / G, H, Sp, hd] (Sp = Smax - Tmax, one row per PROMPT, filled by one prefill per prompt) plus suffix
    cache ksfx / vsfx [L, B, H, Tmax, hd] (the tokens each of the B rows generated); row r = b * G + j is sample / beam j of prompt b
    (csrc/shared.hip).  A step rotates at pos = S0 + t but appends at suffix slot t; egomi_qkv_finish takes one `pos` for both, so this
    layout has no fused finish.  Interface: DenseCache."""
    fused_qkv = False

    def __init__(self, lm, B, G, Smax, Tmax, dtype, dev):
        self.B, self.G, self.H, self.hd, self.Tmax, self.Sp, self.S0 = B, G, lm.num_attention_heads, lm.head_dim, Tmax, Smax - Tmax, 0
        self.kp = torch.zeros(lm.num_hidden_layers, B // G, self.H, self.Sp, self.hd, dtype=dtype, device=dev)
        self.vp = torch.zeros_like(self.kp)
        self.ksfx = torch.zeros(lm.num_hidden_layers, B, self.H, Tmax, self.hd, dtype=dtype, device=dev)
        self.vsfx = torch.zeros_like(self.ksfx)

    def tensors(self):
        return (self.kp, self.vp, self.ksfx, self.vsfx)

    def begin(self, S0, total_new):
        if S0 > self.Sp or total_new > self.Tmax:
            raise ValueError(f"prompt length {S0} / {total_new} new tokens exceed the decoder's prompt cache ({self.Sp}) / suffix cache ({self.Tmax})")
        self.S0 = S0

    def append_prompt(self, l, qkv, B, Sq, row=None):
        d, sel = self.H * self.hd, (l,) if row is None else (l, row)
        kv_append(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv.stride(0), self.kp[sel], self.vp[sel], B, Sq, self.H, self.hd, self.Sp, 0)

    def append_step(self, l, qkv, pos):
        d = self.H * self.hd
        kv_append(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv.stride(0), self.ksfx[l], self.vsfx[l], self.B, 1, self.H, self.hd, self.Tmax, pos - self.S0)

    def attend(self, l, pos, qkv, mask, out, kv_row, nb):
        B, G, S0 = self.B, self.G, self.S0
        head = (qkv, qkv.stride(0), self.kp[l], self.vp[l], mask[::G], self.ksfx[l], self.vsfx[l])
        tail = (out, B // G, G, self.H, self.hd, self.Sp, S0, self.Tmax, pos - S0 + 1, self.hd ** -0.5)
        if kv_row is None:
            attn_decode_shared(*head, *tail)
        else:                                               # the suffix rows that kv_row[:, S0:] names (its columns below S0 are not read)
            attn_decode_shared_rows(*head, kv_row[:, S0:], B, *tail)


def _group_spec(flag, rows, G, B, kv_dtype, max_new_tokens, max_len):
    """The checks of a constructor flag that asks for the prompt / suffix cache with G decoder rows per prompt (`rows`: what G counts)."""
    if kv_dtype == "fp8":
        raise NotImplementedError(f"{flag} with an fp8 KV cache is not built")
    if B % G:
        raise ValueError(f"{B} decoder rows are not a multiple of {rows} = {G}")
    if max_new_tokens is None or not 0 < int(max_new_tokens) < max_len:
        raise ValueError(f"{flag} needs max_new_tokens (the suffix cache length) in 1 .. max_len - 1")
    return G


class Decoder:
    def __init__(self, engine, B, max_len, num_beams=1, kv_dtype=None, weight_dtype=None, samples_per_prompt=1, max_new_tokens=None,
                 split_cache=False, score_cache=False):
        """B = rows of every decode step; num_beams > 1: B = items * num_beams logical beams (beam() after prefill(nb=...)).
        self.cache is the KV cache, one object per layout (DenseCache, Fp8Cache, SplitCache above); its tensors also read as self.kc / vc /
        ks / vs / kp / vp / ksfx / vsfx, None where the layout has none.
        kv_dtype="fp8": Fp8Cache instead of DenseCache; None: the model's dtype.
        weight_dtype="fp8": step() runs the four projections of every layer (q|k|v, o_proj, gate|up, down_proj) on e4m3fn codes with one fp32
        scale per output row (W8A16, csrc/w8.hip; self.w8); lm_head, the embeddings and the norms keep the model's dtype, and prefill runs
        on the bf16 weights.  bf16 engines and B <= 512 only; None: the model's weights.
        weight_dtype="int4": the same four projections on 4-bit codes -7 .. 7 with one fp32 scale per output row and 128-column group,
        s = amax / 7 (W4A16, csrc/w4.hip; self.w4: per layer (packed uint8 [N, K / 2], scales fp32 [NG, N])): 0.53 of the fp8 bytes at
        about 4.5 times the weight error.  Same limits and the same bf16 parts as "fp8".  self.wq is the codes step() multiplies (self.w8
        or self.w4, None on the model's weights) and self.qmm = (product, slab product) their kernels.
        samples_per_prompt = K > 1 (best-of-K sampling; needs max_new_tokens = Tmax): the B rows are K samples of each of B / K prompts,
        row r = b * K + j, on a SplitCache with G = K; step() attends over prompt and suffix with egomi_attn_decode_shared.  sample() /
        greedy() are unchanged: same rows, same seed, same draws as the expanded decoder.
        split_cache=True with num_beams = nb > 1 (needs max_new_tokens = Tmax): beam search on a SplitCache with G = nb.  A beam's suffix is
        the path through its ancestors' rows, so step() appends into the row's own suffix row and attends with
        egomi_attn_decode_shared_rows through kv_row[:, S0:] (egomi_beam_update keeps that table as in the dense layout).  beam() is unchanged.
        score_cache=True (needs max_new_tokens = Tmax; num_beams == 1, model-dtype cache and weights): the decoder of score(), on the
        SplitCache with G = samples_per_prompt also when that is 1 (one given candidate per prompt: the ground truth).  Without the
        flag samples_per_prompt = 1 is the dense decoder, as ever."""
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8', not {kv_dtype!r}")
        if weight_dtype not in (None, "fp8", "int4"):
            raise ValueError(f"weight_dtype must be None, 'fp8' or 'int4', not {weight_dtype!r}")
        if weight_dtype is not None and engine.dtype != torch.bfloat16:
            raise ValueError(f"{weight_dtype} decode weights need a bf16 model, not {engine.dtype}")
        if weight_dtype is not None and B > 512:
            raise ValueError(f"{weight_dtype} decode weights support at most 512 decoder rows, not {B}")
        K, nb, G = int(samples_per_prompt), int(num_beams), 1               # G: decoder rows per prompt-cache row
        if K != 1:
            if not 1 < K <= 32:
                raise ValueError(f"samples_per_prompt must be between 1 and 32, not {samples_per_prompt}")
            if nb != 1:
                raise NotImplementedError("samples_per_prompt > 1 with num_beams > 1 is not built")
            G = _group_spec("samples_per_prompt > 1", "samples_per_prompt", K, B, kv_dtype, max_new_tokens, max_len)
        if split_cache:
            if nb <= 1:
                raise ValueError("split_cache needs num_beams > 1 (independent samples of one prompt: samples_per_prompt)")
            if nb > 32:
                raise ValueError(f"split_cache supports at most 32 beams, not {num_beams}")
            G = _group_spec("split_cache", "num_beams", nb, B, kv_dtype, max_new_tokens, max_len)
        if score_cache:
            if nb != 1 or weight_dtype is not None:
                raise ValueError("score_cache is for num_beams == 1 on the model's own weights")
            G = _group_spec("score_cache", "samples_per_prompt", K, B, kv_dtype, max_new_tokens, max_len)
        split = G > 1 or bool(score_cache)
        self.eng, self.B, self.Smax, self.nb, self.K, self.kv_dtype = engine, B, max_len, nb, K, kv_dtype
        lm = engine.dims.lm
        L, d, Fd, V = lm.num_hidden_layers, lm.hidden_size, lm.intermediate_size, lm.vocab_size
        T, dev = engine.dtype, engine.device
        self.cache = SplitCache(lm, B, G, max_len, int(max_new_tokens), T, dev) if split else \
            (Fp8Cache if kv_dtype == "fp8" else DenseCache)(lm, B, max_len, T, dev)
        z = lambda *s, dtype=T: torch.zeros(*s, dtype=dtype, device=dev)
        self.x, self.h, self.qkv, self.ao, self.x_mid, self.h2 = z(B, d), z(B, d), z(B, 3 * d), z(B, d), z(B, d), z(B, d)
        self.gu, self.act, self.hn, self.lg = z(B, 2 * Fd), z(B, Fd), z(B, d), z(B, V)
        self.tok = z(B, 1, dtype=torch.int64)
        self.gws = torch.empty(128 << 20, dtype=torch.uint8, device=dev)      # split-K slabs of the skinny decode GEMMs
        # sequences, key mask, generator state and eos flags live in STATIC buffers, so that a captured token loop can be replayed by a later
        # generate() call of the same geometry (run_validation: one capture per (prompt length, new tokens, sampling mode), not one per batch)
        self.seq_buf = z(B, max_len, dtype=torch.int64)
        self.mask_buf = torch.ones(B, max_len, dtype=torch.uint8, device=dev)
        self.rng = z(2, dtype=torch.int64)
        self.done_buf = z(B, dtype=torch.int32)
        self._graphs, self._scores = {}, {}
        self.lp_tok = self.lp_sum = self.lp_n = self.lp_live = None      # sample() / greedy() with logprobs=True: made on first use (_lp_buffers)
        self.bs_mass = self.bs_mean = self.bs_std = self.bs_ent = None   # sample() / greedy() / score() with bin_stats=(p0, nb) (_bs_buffers)
        self._bs_values = {}
        self.gr_state = self.gr_need = self.gr_mass = None               # sample() / greedy() with grammar=spec (_grammar)
        self.gr_lim = self.gr_pose = self.gr_limits_mass = None          # ... and limits=table
        self._score_act = None                              # score(): the activations of a suffix pass, made on first use (_score_buffers)
        self.kv_row = None                                  # beam mode: [B, Smax] int32, physical cache row of every key of every logical row
        if self.nb > 1:
            self._beam_buffers()
        self.seq = None
        self.mask = None
        self.pos = 0
        # inference-only resident copies: [Wq;Wk;Wv] and [Wgate;Wup] stacked so one product fills q|k|v (resp. gate|up);
        # fewer, wider launches for the weight-streaming-bound decode step (+0.28 GB per layer of HBM)
        w = engine.w
        if not engine.prepared:
            engine.prepare()
        self.wqkv = [engine.wqkv[l] if l in engine.wqkv else torch.cat([w[f"model.layers.{l}.self_attn.{n}_proj.weight"] for n in "qkv"], 0)
                     for l in range(L)]
        self.wgu = [engine.wgu[l] if l in engine.wgu else engine.stack_gate_up(w[f"model.layers.{l}.mlp.gate_proj.weight"], w[f"model.layers.{l}.mlp.up_proj.weight"])
                    for l in range(L)]                     # interleaved-32 rows when ffn % 32 == 0 (engine.gu_il): gate|up come out interleaved
        self.wo = self.wdown = None                        # LoRA: merged o_proj / down_proj copies (otherwise step() reads eng.w)
        if engine.lora is not None:
            self._merge_lora()

        # single-token step: the split-K projections leave their fp32 slabs unsummed and the NEXT kernel of the layer sums them
        # while doing its own work (qkv -> RoPE + cache append; o_proj / down_proj -> residual + RMSNorm): three launches and a
        # round trip of each product through HBM fewer per layer.  Slice counts are the library's plan for these shapes (0 =
        # it would not split: that projection keeps the plain path).  EGOMI_DECODE_FUSED=0 switches the whole thing off (A/B).
        self.fused = {"qkv": 0, "o": 0, "down": 0}
        self.w8 = self.w4 = self.wq = self.qmm = None
        if weight_dtype is not None:                        # the quantized products always leave slabs: their only path
            if weight_dtype == "fp8":
                self.wq = self.w8 = self._fp8_weights()
                self.qmm = (ops.mm_w8, ops.mm_w8_slabs)
            else:
                self.wq = self.w4 = self._int4_weights()
                self.qmm = (ops.mm_w4, ops.mm_w4_slabs)
            q, slabs = self.wq[0], self.qmm[1]
            self.fused = {"qkv": slabs(self.h, *q["qkv"], self.gws, count_only=True),
                          "o": slabs(self.ao, *q["o"], self.gws, count_only=True),
                          "down": slabs(self.act, *q["down"], self.gws, count_only=True)}
            if not all(self.fused.values()):
                raise ValueError(f"{weight_dtype} decode weights cannot run this model's projection shapes ({self.fused})")
        elif T == torch.bfloat16 and os.environ.get("EGOMI_DECODE_FUSED", "1") != "0" and B <= 512:
            self.fused["qkv"] = ops.mm_slabs(self.h, self.wqkv[0], self.qkv, self.gws, count_only=True)
            self.fused["o"] = ops.mm_slabs(self.ao, w["model.layers.0.self_attn.o_proj.weight"], self.x_mid, self.gws, count_only=True)
            self.fused["down"] = ops.mm_slabs(self.act, w["model.layers.0.mlp.down_proj.weight"], self.x, self.gws, count_only=True)
        if not self.cache.fused_qkv:                        # the q|k|v product keeps the unfused mm + rope_ + append_step path
            self.fused["qkv"] = 0

    def _lp_buffers(self):
        """Static buffers of sample(logprobs=True) / greedy(logprobs=True), made on first use: lp_tok [B, max_len] (column t = step t),
        lp_sum [B], lp_n [B], lp_live [B]."""
        if self.lp_tok is None:
            dev = self.eng.device
            self.lp_tok = torch.zeros(self.B, self.Smax, dtype=torch.float32, device=dev)
            self.lp_sum = torch.zeros(self.B, dtype=torch.float32, device=dev)
            self.lp_n = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.lp_live = torch.ones(self.B, dtype=torch.int32, device=dev)
        self.lp_sum.zero_()
        self.lp_n.zero_()
        self.lp_live.fill_(1)

    def _bs_buffers(self, bin_stats):
        """Static buffers of sample() / greedy() / score() with bin_stats=(p0, nb), made on first use: bs_mass / bs_mean / bs_std / bs_ent
        [B, max_len] (column t = step t) and the float64 bin values of nb bins.  -> (p0, nb, values, (mass, mean, std, ent))."""
        p0, nb = bin_window(bin_stats, self.lg.shape[1])
        dev = self.eng.device
        if self.bs_mass is None:
            self.bs_mass, self.bs_mean, self.bs_std, self.bs_ent = (torch.zeros(self.B, self.Smax, dtype=torch.float32, device=dev) for _ in range(4))
        if nb not in self._bs_values:
            from .traj import bin_edges
            self._bs_values[nb] = bin_edges(nb, dev)
        return p0, nb, self._bs_values[nb], (self.bs_mass, self.bs_mean, self.bs_std, self.bs_ent)

    def _grammar(self, grammar, T_new, limits=None):
        """The trajectory grammar of sample() / greedy() with grammar=spec: its static buffers, made on first use -- gr_state int32 [B, 2]
        (phase, steps per row), gr_need int32 [B] (the tokens the prompt row needs to close: a row with gr_need <= T_new ends `<te> eos`
        inside the loop, any other may not; the caller checks), gr_mass fp32 [B, max_len] (column t = the raw probability of step t's allowed
        set) -- and -> (head, mask, key).  head() queues egomi_traj_grammar_init on the prompt in self.seq / self.mask: the token loop
        starts with it, inside the captured graph, so every replay starts from the state of the prompt that is in the static buffers then,
        not from where the last replay ended.  mask(t) queues step t's egomi_traj_grammar_step on self.lg, directly before the token
        kernel.  key: what the grammar adds to a graph key (the spec with its step limits).  None: no launch, no buffer, () as key.
        limits=table (traj_limits_check; [B, 18] CPU integers): the motion limits.  Three more static buffers, made on first use -- gr_lim
        int32 [B, 18], gr_pose int32 [B, 12], gr_limits_mass fp32 [B, max_len] -- and the two launches become egomi_traj_grammar_init_limits
        / egomi_traj_grammar_step_limits.  The table is copied into gr_lim here, before the loop, on every call: the captured loop reads
        it from there, so the key gains the constant "limits" only and a replay with another table needs no re-capture."""
        if grammar is None:
            if limits is not None:
                raise ValueError("motion limits narrow the trajectory grammar's bin window: `limits` needs `grammar`")
            return (lambda: None), (lambda t: None), ()
        if self.nb > 1:
            raise ValueError("a trajectory grammar is for num_beams == 1: the beams of an item share one prefill logits row at step 0")
        spec = grammar_check(grammar, self.lg.shape[1])
        if self.gr_state is None:
            dev = self.eng.device
            self.gr_state = torch.zeros(self.B, 2, dtype=torch.int32, device=dev)
            self.gr_need = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.gr_mass = torch.zeros(self.B, self.Smax, dtype=torch.float32, device=dev)
        S0 = self.pos
        if limits is not None:
            table = traj_limits_check(limits, spec[1], self.B)
            if self.gr_lim is None:
                dev = self.eng.device
                self.gr_lim = torch.zeros(self.B, 18, dtype=torch.int32, device=dev)
                self.gr_pose = torch.zeros(self.B, 12, dtype=torch.int32, device=dev)
                self.gr_limits_mass = torch.zeros(self.B, self.Smax, dtype=torch.float32, device=dev)
            self.gr_lim.copy_(table)

            def head_l():
                traj_grammar_init_limits(self.seq_buf[:, :S0], self.mask_buf[:, :S0], spec, self.gr_state, self.gr_need, self.gr_pose)

            def mask_l(t):
                traj_grammar_step_limits(self.lg, None if t == 0 else self.tok.view(-1), self.gr_state, spec, T_new - t, self.gr_mass, t,
                                         self.gr_lim, self.gr_pose, self.gr_limits_mass)
            return head_l, mask_l, ("grammar",) + spec + ("limits",)

        def head():
            traj_grammar_init(self.seq_buf[:, :S0], self.mask_buf[:, :S0], spec, self.gr_state, self.gr_need)

        def mask(t):
            traj_grammar_step(self.lg, None if t == 0 else self.tok.view(-1), self.gr_state, spec, T_new - t, self.gr_mass, t)
        return head, mask, ("grammar",) + spec

    def _readouts(self, logprobs, bin_stats, eos):
        """The per-step readouts of sample() / greedy() / score(): prepares their buffers (_lp_buffers, _bs_buffers) and -> (emit, key).
        emit(logits, tokens, col, rows=slice(None)) issues, for decoder rows `rows`, the egomi_token_logprob launch of logprobs=True (into
        lp_tok[:, col], lp_sum, lp_n; lp_live stops a row's count after its `eos`) and then the egomi_bin_stats launch of bin_stats=(p0, nb)
        (into bs_mass / bs_mean / bs_std / bs_ent[:, col]), both on the raw `logits`.  key: what the readouts add to a graph key."""
        bs = self._bs_buffers(bin_stats) if bin_stats is not None else None
        if logprobs:
            self._lp_buffers()
        live = self.lp_live if logprobs and eos is not None else None

        def emit(logits, tokens, col, rows=slice(None)):
            if logprobs:
                token_logprob(logits, tokens, eos, None if live is None else live[rows], self.lp_tok[rows], col, self.lp_sum[rows], self.lp_n[rows])
            if bs is not None:
                bin_stats_rows(logits, *bs[:3], *(buf[rows] for buf in bs[3]), col)
        return emit, (("logprobs",) if logprobs else ()) + (("bin_stats", bs[0], bs[1]) if bs is not None else ())

    def _merge_lora(self):
        """LoRA: the decode steps multiply merged copies W + s B A of the adapted projections (one fp32 sum, rounded once; csrc/lora.hip);
        the prefill runs through the engine on the unmerged adapters.  A decoder is made for one set of adapter values: the model's decoder
        cache keys on engine.lora_key()."""
        eng = self.eng
        w, tg = eng.w, eng.lora.targets
        get = lambda l, t: eng.lora_merged(l, t) if t in tg else w[lora.base_name(l, t)]
        self.wo = [w[lora.base_name(l, "o_proj")] for l in range(len(self.wqkv))]
        self.wdown = [w[lora.base_name(l, "down_proj")] for l in range(len(self.wqkv))]
        for l in range(len(self.wqkv)):
            if any(t in tg for t in ("q_proj", "k_proj", "v_proj")):
                self.wqkv[l] = torch.cat([get(l, t) for t in ("q_proj", "k_proj", "v_proj")], 0)
            if any(t in tg for t in ("gate_proj", "up_proj")):
                self.wgu[l] = eng.stack_gate_up(get(l, "gate_proj"), get(l, "up_proj"))
            if "o_proj" in tg:
                self.wo[l] = get(l, "o_proj")
            if "down_proj" in tg:
                self.wdown[l] = get(l, "down_proj")

    def _fp8_weights(self):
        """Per layer {"qkv", "o", "gu", "down": (codes uint8 [N, K], scales fp32 [N])} of the stacked forms step() multiplies ([Wq;Wk;Wv],
        [Wgate;Wup] in its interleaved-32 order when engine.gu_il).  Frozen layers: one copy per engine and prepare_epoch, shared by every
        decoder (Engine.prepared = False drops it); trainable layers change under every optimizer step, so each decoder quantizes afresh."""
        return self._quantized("w8", ops.quantize_rows_fp8)

    def _int4_weights(self):
        """_fp8_weights for the int4 form: (packed uint8 [N, K / 2], scales fp32 [NG, N]) per projection, cached as engine.w4."""
        return self._quantized("w4", ops.quantize_rows_int4)

    def _quantized(self, attr, quantize):
        eng = self.eng
        held = getattr(eng, attr)
        if held is not None and held[0] == eng.weights_key() and not eng.any_layer_trainable:
            return held[1]
        q = [{"qkv": quantize(self.wqkv[l]), "o": quantize(self._w(l, "o")), "gu": quantize(self.wgu[l]), "down": quantize(self._w(l, "down"))}
             for l in range(len(self.wqkv))]
        if not eng.any_layer_trainable:
            setattr(eng, attr, (eng.weights_key(), q))
        return q

    def _w(self, l, name):
        """o_proj / down_proj of layer l as the decode step multiplies it: the merged LoRA copy, else the engine's weight."""
        merged = self.wo if name == "o" else self.wdown
        if merged is not None:
            return merged[l]
        return self.eng.w[f"model.layers.{l}." + ("self_attn.o_proj.weight" if name == "o" else "mlp.down_proj.weight")]

    def _slabs(self, l, name, a, out_like, weight):
        """The split-K slabs of one projection (fp8, int4 or model-dtype weights) at the start of self.gws; -> their number."""
        if self.wq is not None:
            return self.qmm[1](a, *self.wq[l][name], self.gws)
        return ops.mm_slabs(a, weight, out_like, self.gws)

    # -- prefill -------------------------------------------------------------------------------------
    def _set_inputs(self, input_ids, mask, total_new, nb=1):
        """Prompt ids and key mask into the static buffers (`seq` is a [B, S0 + total_new] view of rows that are Smax long); nb > 1: every
        prompt row serves the nb logical beams of its item."""
        B, S0 = input_ids.shape
        if S0 + total_new > self.Smax:
            raise ValueError("prompt + new tokens exceed the decoder's cache length")
        if B * nb != self.B:
            raise ValueError(f"{B} prompts x {nb} beams do not fill the decoder's {self.B} rows")
        self.cache.begin(S0, total_new)
        if nb > 1:
            input_ids, mask = input_ids.repeat_interleave(nb, 0), mask.repeat_interleave(nb, 0)
        self.mask_buf.fill_(1)
        self.mask_buf[:, :S0] = mask.to(torch.uint8)
        self.mask = self.mask_buf
        self.seq_buf.zero_()
        self.seq_buf[:, :S0] = input_ids
        self.seq = self.seq_buf[:, :S0 + total_new]

    def prefill(self, input_ids, attention_mask, point_clouds, fps_start, total_new, nb=1, chunk=None):
        """nb > 1 (beam mode): the B prompts run ONCE each; their K/V land in physical cache rows 0..B-1 and their logits in rows 0..B-1 of
        self.lg, which every beam of the item reads at step 0 (HF expands to B * nb identical rows and prefills them all).
        chunk=None: one prompt pass over the whole batch; chunk=n: prefill_chunked()."""
        B, S0 = input_ids.shape
        eng, dev = self.eng, self.eng.device
        if self.K > 1:
            nb = self.K
        mask = torch.ones(B, S0, dtype=torch.bool, device=dev) if attention_mask is None else attention_mask.to(dev).bool()
        self._set_inputs(input_ids, mask, total_new, nb)
        for b0 in range(0, B, chunk or B):
            b1 = min(B, b0 + (chunk or B))

            def sink(l, qkv, Bc, Sq, b0=b0):
                if chunk is None:                 # the whole batch: one append
                    return self.cache.append_prompt(l, qkv, Bc, Sq)
                for i in range(Bc):               # a batch slice of the [L,B,H,Smax,hd] cache is not contiguous over samples: one append each
                    self.cache.append_prompt(l, qkv[i * Sq:(i + 1) * Sq], 1, Sq, row=b0 + i)
            cut = lambda a: None if a is None else a[b0:b1]
            hn = eng.forward_hidden(input_ids[b0:b1], mask[b0:b1], cut(point_clouds), cut(fps_start), save=False, kv_sink=sink)
            last = hn.view(b1 - b0, S0, -1)[:, -1].contiguous()
            ops.mm(last, eng.w["lm_head.weight"], out=self.lg[b0:b1])
        self.pos = S0
        if self.K == 1:                                     # beams read their item's row themselves (egomi_beam_rows' lg_div)
            return self.lg[:B]
        # every sample of a prompt starts from the prompt's step-0 logits (HF prefills K identical rows)
        self.lg.copy_(self.lg[:B].repeat_interleave(self.K, 0))
        return self.lg

    def prefill_chunked(self, input_ids, attention_mask, point_clouds, fps_start, total_new, chunk=16, nb=1):
        """prefill() for large batches (config 5: bs=256): the prompt pass runs `chunk` samples at a time (its activations are
        what limits the batch, not the cache) and every chunk appends its K/V rows to its own slice of the static cache."""
        return self.prefill(input_ids, attention_mask, point_clouds, fps_start, total_new, nb, chunk)

    # -- one decode step on static buffers: consumes self.tok, leaves logits in self.lg ---------------------
    def step(self, pos):
        eng = self.eng
        w, lm = eng.w, eng.dims.lm
        B, d, Fd, H, hd, L = self.B, lm.hidden_size, lm.intermediate_size, lm.num_attention_heads, lm.head_dim, lm.num_hidden_layers
        ops.embed_splice(self.tok, w["model.embed_tokens.weight"], None, None, eng.dims.pb.point_token_len, out=self.x.view(B, 1, d))
        x = self.x
        fq, fo, fd = self.fused["qkv"], self.fused["o"], self.fused["down"]
        normed = False                                      # self.h already holds this layer's input norm (written by the previous layer's tail)
        for l in range(L):
            p = f"model.layers.{l}."
            if not normed:
                ops.rmsnorm(x, w[p + "input_layernorm.weight"], lm.rms_norm_eps, out=self.h)
            if fq:
                n = self._slabs(l, "qkv", self.h, self.qkv, self.wqkv[l])
                self.cache.qkv_finish(l, self.gws, n, self.qkv, eng.cos, eng.sin, pos)
            else:
                if self.wq is not None:                     # (prompt / suffix cache: the only unfused q|k|v product on quantized weights)
                    self.qmm[0](self.h, *self.wq[l]["qkv"], out=self.qkv, workspace=self.gws)
                else:
                    ops.mm(self.h, self.wqkv[l], out=self.qkv, workspace=self.gws)
                ops.rope_(self.qkv, eng.cos, eng.sin, B, 1, pos, 2 * H, hd, 3 * d)
                self.cache.append_step(l, self.qkv, pos)
            self.cache.attend(l, pos, self.qkv, self.mask, self.ao, self.kv_row, self.nb)
            if fo:
                n = self._slabs(l, "o", self.ao, self.x_mid, self._w(l, "o"))
                ops.slabs_rmsnorm(self.gws, n, x, w[p + "post_attention_layernorm.weight"], lm.rms_norm_eps, self.x_mid, self.h2)
            else:
                ops.mm(self.ao, self._w(l, "o"), out=self.x_mid, residual=x, workspace=self.gws)
                ops.rmsnorm(self.x_mid, w[p + "post_attention_layernorm.weight"], lm.rms_norm_eps, out=self.h2)
            if self.wq is not None:
                self.qmm[0](self.h2, *self.wq[l]["gu"], out=self.gu, workspace=self.gws)
            else:
                ops.mm(self.h2, self.wgu[l], out=self.gu, workspace=self.gws)
            if eng.gu_il:
                ops.swiglu_il(self.gu, self.act)
            else:
                ops.swiglu(self.gu[:, :Fd], self.gu[:, Fd:], self.act)
            if fd:                                          # x is not an input of this product: the tail writes the new residual stream into it
                n = self._slabs(l, "down", self.act, x, self._w(l, "down"))
                last = l + 1 == L
                ops.slabs_rmsnorm(self.gws, n, self.x_mid, w["model.norm.weight"] if last else w[f"model.layers.{l + 1}.input_layernorm.weight"],
                                  lm.rms_norm_eps, x, self.hn if last else self.h)
                normed = True
            else:
                ops.mm(self.act, self._w(l, "down"), out=x, residual=self.x_mid, workspace=self.gws)
                normed = False
        if not normed:
            ops.rmsnorm(x, w["model.norm.weight"], lm.rms_norm_eps, out=self.hn)
        ops.mm(self.hn, w["lm_head.weight"], out=self.lg)

    # -- token loops ---------------------------------------------------------------------------------
    def _run(self, steps, use_graph, key=None):
        """Runs the token loop steps(): eagerly, or as ONE hipGraph.  The captured loop depends only on what the caller puts into `key`
        (every buffer it touches is static; the seed, the eos flags and the loop-open flag are device memory), so a later call with the
        same key replays the graph kept in self._graphs; key=None captures afresh and keeps nothing."""
        if not use_graph:
            return steps()
        g = self._graphs.get(key) if key is not None else None
        if g is None:
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                steps()
            if key is not None:
                self._graphs[key] = g
        g.replay()
        self.graph = g

    def _seed(self, seed):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())            # the CPU default generator: torch.manual_seed() makes a run repeatable
        self.rng.copy_(torch.tensor([int(seed), 0], dtype=torch.int64))

    def _score_buf(self, T_new):
        """The static [T_new, B, V] fp32 buffer of the processed scores."""
        if T_new not in self._scores:
            self._scores[T_new] = torch.empty(T_new, self.B, self.lg.shape[1], dtype=torch.float32, device=self.eng.device)
        return self._scores[T_new]

    def sample(self, T_new, do_sample=True, temperature=1.0, top_k=50, top_p=0.95, repetition_penalty=1.0, eos=None, pad=None, seed=None,
               use_graph=True, logprobs=False, bin_stats=None, grammar=None, limits=None):
        """After prefill(): T_new steps of HF generate's token loop (model_arch.py:82-108 -> GenerationMixin: logits processors, warpers,
        multinomial / arg-max, eos bookkeeping), every step one egomi_sample_rows launch + one cached decode step, all of them captured
        into ONE hipGraph (the draw counter and `pos` are launch constants, seed and done flags live in device memory).
        Returns (sequences [B, S0+T_new], processed scores fp32 [T_new, B, V]); rows that emitted `eos` continue with `pad`.
        logprobs=True: every step also runs one egomi_token_logprob launch on the raw logits, after the token kernel: self.lp_tok[:, t] is
        the chosen token's log-prob (0 once the row has finished), self.lp_sum / self.lp_n the row's sum and token count (its eos counted,
        the pads not).  A graph of its own (the flag is part of the key); with False the loop has the launches it had.
        bin_stats=(p0, nb): every step also runs one egomi_bin_stats launch on the raw logits, after those: self.bs_mass / bs_mean / bs_std /
        bs_ent[:, t] describe the distribution token t was chosen from, over the bin ids p0 .. p0 + nb - 1 (values linspace(-1, 1, nb)); rows
        that have finished are computed like any other (the caller cuts at the eos).  Again a graph of its own; None: no launch, no buffer.
        grammar=spec (traj.grammar_spec; num_beams == 1): constrained decoding.  The loop starts with one egomi_traj_grammar_init launch on
        the prompt, and every step runs one egomi_traj_grammar_step launch directly before the token kernel (csrc/grammar.hip; _grammar):
        in place on self.lg, every id the row's grammar state does not allow becomes -inf, and self.gr_mass[:, t] keeps the raw probability
        the model gave the allowed set.  Everything downstream then sees the CONSTRAINED row: the returned scores are the processed scores
        of the constrained distribution, and logprobs / bin_stats describe that same renormalised distribution -- the one the token was
        drawn from, a proper distribution over valid trajectories; the raw signal survives in gr_mass alone.  A row with
        self.gr_need <= T_new ends `<te> eos` with min_steps <= n <= max_steps.  A graph of its own (the spec and its limits are part of the
        key); None: the loop has the launches it had.
        limits=table (with grammar; traj.motion_limits, [B, 18] CPU integers): per-row, per-dimension motion limits on the bins
        (_grammar): the same two launches in their *_limits form, self.gr_limits_mass[:, t] = the raw probability of what the limits
        allow beside gr_mass[:, t].  The table lives in self.gr_lim: another table replays the same graph."""
        emit, readout_key = self._readouts(logprobs, bin_stats, eos)
        gr_head, gr_mask, gr_key = self._grammar(grammar, T_new, limits)
        S0, sc_buf = self.pos, self._score_buf(T_new)
        self._seed(seed)
        self.done_buf.zero_()
        self.done = self.done_buf if eos is not None else None
        kw = dict(repetition_penalty=float(repetition_penalty or 1.0), temperature=float(temperature or 1.0), top_k=int(top_k or 0),
                  top_p=float(1.0 if top_p is None else top_p), do_sample=bool(do_sample), rng=self.rng, eos=eos, pad=pad)

        def steps():
            gr_head()
            for t in range(T_new):
                gr_mask(t)
                sample_rows(self.lg, sc_buf[t], self.seq, S0 + t, 0, self.tok.view(-1), self.done, draw=t, **kw)
                emit(self.lg, self.tok.view(-1), t)
                if t + 1 < T_new:
                    self.step(S0 + t)
        key = (S0, T_new, kw["repetition_penalty"], kw["temperature"], kw["top_k"], kw["top_p"], kw["do_sample"], eos, pad)
        self._run(steps, use_graph, key + readout_key + gr_key)
        self.pos = S0 + T_new
        return self.seq, sc_buf

    def greedy(self, T_new, use_graph=True, keep_scores=True, logprobs=False, bin_stats=None, grammar=None, limits=None):
        """After prefill(): T_new greedy tokens.  Returns (sequences [B,S0+T], scores list or None).  logprobs=True: one egomi_token_logprob
        launch per step after the arg-max, into self.lp_tok / lp_sum / lp_n as in sample() (no eos here: every row counts every step).
        bin_stats=(p0, nb): one egomi_bin_stats launch per step after those, into self.bs_mass / bs_mean / bs_std / bs_ent as in sample().
        grammar=spec: as in sample(): the init launch before the loop and one egomi_traj_grammar_step launch per step before the scores
        are kept and the arg-max runs, so scores, logprobs and bin_stats are those of the constrained row; self.gr_mass / gr_need as there.
        limits=table: as in sample()."""
        emit, _ = self._readouts(logprobs, bin_stats, None)
        gr_head, gr_mask, _ = self._grammar(grammar, T_new, limits)
        S0 = self.pos
        scores = None                                       # eager: fp32 clones; captured: views of one buffer the graph writes
        if keep_scores:
            scores = list(torch.zeros(T_new, self.B, self.lg.shape[1], dtype=torch.float32, device=self.eng.device)) if use_graph else []

        def steps():
            gr_head()
            for t in range(T_new):
                gr_mask(t)
                if keep_scores and use_graph:
                    ops.cast(self.lg, torch.float32, out=scores[t])
                elif keep_scores:
                    scores.append(self.lg.float().clone())
                argmax_rows(self.lg, self.tok.view(-1), self.seq, S0 + t)
                emit(self.lg, self.tok.view(-1), t)
                if t + 1 < T_new:
                    self.step(S0 + t)
        self._run(steps, use_graph)                         # a fresh capture per call
        self.pos = S0 + T_new
        return self.seq, scores

    # -- teacher-forced scoring of given candidates ------------------------------------------------------
    def _score_buffers(self, rows):
        """The activations of one suffix pass of `rows` token rows, made on first use and kept while they are large enough."""
        held = self._score_act
        if held is None or held["x"].shape[0] < rows:
            lm, T, dev = self.eng.dims.lm, self.eng.dtype, self.eng.device
            d, Fd, V = lm.hidden_size, lm.intermediate_size, lm.vocab_size
            self._score_act = held = None                   # the smaller set goes before the larger one comes
            z = lambda *s: torch.zeros(*s, dtype=T, device=dev)
            held = self._score_act = {"x": z(rows, d), "h": z(rows, d), "qkv": z(rows, 3 * d), "ao": z(rows, d), "x_mid": z(rows, d),
                                      "gu": z(rows, 2 * Fd), "act": z(rows, Fd), "lg": z(rows, V)}
        return {n: t[:rows] for n, t in held.items()}

    def _suffix_pass(self, tokens, b0, b1):
        """step() widened to Tq tokens per row: tokens int64 [(b1 - b0) * K, Tq] are suffix tokens 0 .. Tq-1 of the candidates of clips
        b0 .. b1-1; their k | v go to suffix slots 0 .. Tq-1 and row (r, t) attends over its clip's prompt and its own keys 0 .. t
        (egomi_attn_suffix_shared).  The unfused products on the weights step() reads (never the quantized ones).
        -> logits [(b1 - b0) * K * Tq, V], row (r, t) = the distribution of suffix token t + 1."""
        eng, c = self.eng, self.cache
        w, lm = eng.w, eng.dims.lm
        d, Fd, H, hd, L = lm.hidden_size, lm.intermediate_size, lm.num_attention_heads, lm.head_dim, lm.num_hidden_layers
        K, S0 = c.G, c.S0
        Rg, Tq = tokens.shape
        M, r0, r1 = Rg * Tq, b0 * K, b1 * K
        a = self._score_buffers(M)
        x, h, qkv, ao, x_mid, gu, act, lg = (a[n] for n in ("x", "h", "qkv", "ao", "x_mid", "gu", "act", "lg"))
        ops.embed_splice(tokens, w["model.embed_tokens.weight"], None, None, eng.dims.pb.point_token_len, out=x.view(Rg, Tq, d))
        mask = self.mask[::K][b0:b1]
        for l in range(L):
            p = f"model.layers.{l}."
            ops.rmsnorm(x, w[p + "input_layernorm.weight"], lm.rms_norm_eps, out=h)
            ops.mm(h, self.wqkv[l], out=qkv, workspace=self.gws)
            ops.rope_(qkv, eng.cos, eng.sin, M, Tq, S0, 2 * H, hd, 3 * d)
            ks, vs = c.ksfx[l][r0:r1], c.vsfx[l][r0:r1]
            kv_append(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv.stride(0), ks, vs, Rg, Tq, H, hd, c.Tmax, 0)
            attn_suffix_shared(qkv, qkv.stride(0), c.kp[l][b0:b1], c.vp[l][b0:b1], mask, ks, vs, ao, b1 - b0, K, H, hd, c.Sp, S0, c.Tmax, Tq,
                               hd ** -0.5)
            ops.mm(ao, self._w(l, "o"), out=x_mid, residual=x, workspace=self.gws)
            ops.rmsnorm(x_mid, w[p + "post_attention_layernorm.weight"], lm.rms_norm_eps, out=h)
            ops.mm(h, self.wgu[l], out=gu, workspace=self.gws)
            if eng.gu_il:
                ops.swiglu_il(gu, act)
            else:
                ops.swiglu(gu[:, :Fd], gu[:, Fd:], act)
            ops.mm(act, self._w(l, "down"), out=x, residual=x_mid, workspace=self.gws)
        ops.rmsnorm(x, w["model.norm.weight"], lm.rms_norm_eps, out=h)
        ops.mm(h, w["lm_head.weight"], out=lg)
        return lg

    def score(self, cand, eos, keep_logits=False, row_budget=16384, bin_stats=None):
        """After prefill() on a score_cache decoder: the log-probs of GIVEN suffix tokens cand int64 [B, T] (row r = b * K + j, candidate j
        of clip b) under teacher forcing, on the model's own weights.  Column 0 is read from the prefill logits; columns 1 .. T-1 come
        from ONE suffix pass over tokens 0 .. T-2 of every row (_suffix_pass), clips in groups of at most `row_budget` token rows (at
        least one clip), then one egomi_token_logprob launch per column on that pass's logits (row stride Tq * V) with the buffers, the
        eos rule and the column order of sample(logprobs=True): self.lp_tok[:, :T] (0 after a row's eos), self.lp_sum, self.lp_n.
        Columns past the longest candidate (candidate_lengths) are zero for every row: the pass and the launches stop there.
        keep_logits: -> the pass's logits [B, Tq, V] (Tq = longest candidate - 1; row (r, t) scores token t + 1), else None.
        bin_stats=(p0, nb): one egomi_bin_stats launch beside every egomi_token_logprob launch, on the same logits: self.bs_mass / bs_mean /
        bs_std / bs_ent[:, :T], column t = the distribution candidate token t is scored under; 0 at and after a row's length, like lp_tok."""
        if not self.split or self.nb != 1:
            raise ValueError("score() needs a Decoder(score_cache=True)")
        emit, _ = self._readouts(True, bin_stats, eos)
        bs_bufs = (self.bs_mass, self.bs_mean, self.bs_std, self.bs_ent) if bin_stats is not None else ()
        K, S0, dev = self.cache.G, self.pos, self.eng.device
        R, T = cand.shape
        if R != self.B or T < 1 or T > self.cache.Tmax:
            raise ValueError(f"score(): candidates [{R}, {T}] do not fit the decoder's {self.B} rows / {self.cache.Tmax} suffix tokens")
        cand = cand.to(dev, torch.int64)
        lens = candidate_lengths(cand, eos)
        Tn = int(lens.max())                                # columns >= Tn count for no row
        toks = cand.t().contiguous()                        # [T, R]: a column's tokens are contiguous
        for buf in (self.lp_tok, *bs_bufs):
            buf[:, :T].zero_()
        emit(self.lg, toks[0], 0)
        Tq, V, kept = Tn - 1, self.lg.shape[1], None
        if Tq > 0:
            per = max(1, int(row_budget) // (K * Tq))       # clips per pass
            if keep_logits:
                kept = torch.empty(R, Tq, V, dtype=self.lg.dtype, device=dev)
            for b0 in range(0, R // K, per):
                b1 = min(R // K, b0 + per)
                r0, r1 = b0 * K, b1 * K
                lg = self._suffix_pass(cand[r0:r1, :Tq].contiguous(), b0, b1).view(r1 - r0, Tq, V)
                for t in range(1, Tn):
                    emit(lg[:, t - 1], toks[t, r0:r1], t, slice(r0, r1))
                if keep_logits:
                    kept[r0:r1] = lg
        if bs_bufs:                                         # the launches know no eos: cut every row at its length
            past = torch.arange(T, device=dev)[None, :] >= lens[:, None]
            for buf in bs_bufs:
                buf[:, :T].masked_fill_(past, 0.0)
        return kept

    # -- beam search / beam sampling ---------------------------------------------------------------
    def _beam_buffers(self):
        R, Smax, dev = self.B, self.Smax, self.eng.device
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=dev)
        self.kv_row = z(R, Smax, dtype=torch.int32)
        self.fin_seq = z(R, Smax, dtype=torch.int64)
        self.bidx = z(R, Smax, dtype=torch.int32)             # HF's running_beam_indices / beam_indices (columns 0 .. new tokens - 1)
        self.fin_bidx = z(R, Smax, dtype=torch.int32)
        self.run_score, self.fin_score = z(R, dtype=torch.float32), z(R, dtype=torch.float32)
        self.fin_flag, self.heur = z(R, dtype=torch.int32), z(R // self.nb, dtype=torch.int32)
        self.ctl = z(8, dtype=torch.int32)                    # [0] loop open, [1] iterations run, [2..5] per-step tallies (egomi_beam_update)
        self._cands = {}

    def beam(self, T_new, num_return_sequences=1, length_penalty=1.0, early_stopping=False, do_sample=False, temperature=1.0, top_k=50,
             top_p=1.0, repetition_penalty=1.0, eos=None, pad=None, seed=None, use_graph=True, grammar=None, limits=None):
        """After prefill(nb=self.nb): HF _beam_search (generation/utils.py:3208-3560) for T_new steps, every step one egomi_beam_rows + one
        egomi_beam_update launch + one cached decode step over the B * nb logical beams, all captured into ONE hipGraph (no host sync per
        step: the loop-open flag lives in device memory and closes the remaining steps when HF would have left its loop).
        Returns (sequences [B*nrs, S0 + Lgen], sequences_scores [B*nrs], scores [iterations, B*nb, V] fp32, beam_indices [B*nrs, Lgen])."""
        if grammar is not None:
            raise ValueError("beam() takes no trajectory grammar: the beams of an item share one prefill logits row at step 0")
        if limits is not None:
            raise ValueError("beam() takes no motion limits: they narrow the trajectory grammar's bin window, and beam() takes no grammar")
        nb, R, S0, dev = self.nb, self.B, self.pos, self.eng.device
        Bi, V = R // nb, self.lg.shape[1]
        n_eos = 0 if eos is None else 1
        K = max(2, 1 + n_eos) * nb                                            # beams_to_keep
        max_len = S0 + T_new
        fill = (pad or eos) if eos is not None else -1                         # HF's output_fill_value
        sc_buf = self._score_buf(T_new)
        cands = self._cands.get(K)
        if cands is None:
            cands = self._cands[K] = (torch.empty(R, K, dtype=torch.float32, device=dev), torch.empty(R, K, dtype=torch.float32, device=dev),
                                      torch.empty(R, K, dtype=torch.int32, device=dev))
        # initial state (:3290-3320): running scores [0, -1e9, ...] per item, finished scores -1e9, beam indices -1, sequences filled
        self.seq_buf[:, S0:] = fill
        self.fin_seq.copy_(self.seq_buf)
        self.bidx.fill_(-1)
        self.fin_bidx.fill_(-1)
        self.run_score.view(Bi, nb).fill_(-1e9)
        self.run_score.view(Bi, nb)[:, 0] = 0
        self.fin_score.fill_(-1e9)
        self.fin_flag.zero_()
        self.heur.fill_(1)
        self.ctl.zero_()
        self.ctl[0] = 1
        self.kv_row.zero_()
        self.kv_row[:, :S0] = (torch.arange(R, device=dev, dtype=torch.int32) // nb)[:, None]     # every beam reads its item's prompt row
        self._seed(seed)
        if not do_sample:                                                      # HF applies the warpers in sampling mode only
            temperature, top_k, top_p = 1.0, 0, 1.0
        kw = dict(repetition_penalty=float(repetition_penalty or 1.0), temperature=float(temperature or 1.0), top_k=int(top_k or 0),
                  top_p=float(1.0 if top_p is None else top_p), min_keep=max(2, n_eos + 1), do_sample=bool(do_sample))  # :1299-1305
        es = early_stopping if early_stopping == "never" else bool(early_stopping)

        def steps():
            for t in range(T_new):
                beam_rows(self.lg, nb if t == 0 else 1, R, nb, sc_buf[t], self.seq_buf, S0 + t, rng=self.rng, draw=t, run_score=self.run_score,
                          cand_key=cands[0], cand_score=cands[1], cand_tok=cands[2], ctl=self.ctl, **kw)
                beam_update(Bi, nb, V, cands[0], cands[1], cands[2], S0, S0 + t, max_len, eos, float(length_penalty), es, self.seq_buf,
                            self.fin_seq, self.bidx, self.fin_bidx, self.kv_row, self.run_score, self.fin_score, self.fin_flag, self.heur,
                            self.tok.view(-1), self.ctl)
                if t + 1 < T_new:
                    self.step(S0 + t)
        self._run(steps, use_graph, ("beam", S0, T_new, nb, float(length_penalty), es, eos, pad, tuple(sorted(kw.items()))))
        self.pos = S0 + T_new
        n_iter = int(self.ctl[1])
        nrs = int(num_return_sequences)
        rows = (torch.arange(Bi, device=dev)[:, None] * nb + torch.arange(nrs, device=dev)[None, :]).reshape(-1)
        bidx = self.fin_bidx[rows, :T_new]
        lgen = int((bidx >= 0).sum(1).max()) if T_new > 0 else 0              # :3520, the longest returned hypothesis
        return (self.fin_seq[rows, :S0 + lgen].clone(), self.fin_score[rows].clone(), sc_buf[:n_iter].clone(), bidx[:, :lgen].long())


Decoder.split = property(lambda self: isinstance(self.cache, SplitCache), doc="prompt cache + suffix cache instead of the dense one")
for _n in ("kc", "vc", "ks", "vs", "kp", "vp", "ksfx", "vsfx"):           # the cache's tensors under their names; None where the layout has none
    setattr(Decoder, _n, property(lambda self, _n=_n: getattr(self.cache, _n, None)))
