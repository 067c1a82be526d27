#!/usr/bin/env python3
"""Scoring given trajectories at 7B in the evaluate.py shape: 8 clips, a 540-token prompt (synth_batch(dims, 8, text_len=16, num_steps=20,
max_traj_token=160), as tools/bench_best_of_k.py), K candidates of T = 64 tokens per clip.  Three arms per K, alternated round by round on
one device (A B C, A B C, ...) after a warm-up round, every call timed with device events around it:
  A  model.score(): one prefill per clip + ONE suffix pass over the B*K candidates (egomi_attn_suffix_shared)
  B  the same log-probs from the API that predates score(): model.forward() on the B*K expanded rows of S0 + T tokens, in clip chunks
     that fit (--fwd_clips), then log_softmax and a gather at the candidates
  C  the generate(num_return_sequences=K, share_prompt=True, output_logprobs=True) call that produced the candidates (what rescoring is
     added to)
Reports per arm the median, the min and the arm's own spread (max - min) / median over the rounds, A/B and A/C on the medians, the worst
|A - B| log-prob difference, the row counts of A and B, and a kernel-only timing of egomi_attn_suffix_shared on one layer's buffers (us
per launch, the bytes it models: q, out, the clip's prompt K/V once per query tile, the suffix K/V once per candidate).  The clock state is
recorded around the run as tools/clock_probe.py does.  Prints one JSON line.  Per-kernel times of the pass: run it under
`rocprofv3 --kernel-trace --stats` separately with --arms A (no counters in the same run).
GPU box only:  python tools/bench_score.py [--K 4,16] [--layers N] [--T 64] [--rounds 3] [--arms ABC]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egoscaler_amd import decode, synth
from tools.bench_best_of_k import clocks, model_7b


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def forward_logprobs(m, ids, mask, pcs, st, cand, clips):
    """Arm B: teacher forcing through model.forward() on the expanded rows, `clips` clips at a time -> fp32 [B*K, T]."""
    B, K, T = cand.shape
    S0, out = ids.shape[1], []
    rep = lambda x: x.repeat_interleave(K, 0)
    for b0 in range(0, B, clips):
        sl = slice(b0, b0 + clips)
        c = cand[sl].reshape(-1, T)
        seq = torch.cat([rep(ids[sl]), c], 1)
        am = torch.cat([rep(mask[sl]), torch.ones_like(c, dtype=mask.dtype)], 1)
        lg = m(input_ids=seq, attention_mask=am, point_clouds=rep(pcs[sl]), fps_start=rep(st[sl])).logits[:, S0 - 1:S0 - 1 + T].float()
        out.append(torch.log_softmax(lg, -1).gather(2, c[:, :, None]).squeeze(2))
        del lg
    return torch.cat(out)


def kernel_only(m, B, K, T, reps=20):
    """egomi_attn_suffix_shared alone on the last layer's buffers of the scorer decoder that just ran (q|k|v of the pass, both caches)."""
    dec = list(m._scorers.values())[-1]
    c, lm = dec.cache, m.dims.lm
    H, hd, d, Tq = lm.num_attention_heads, lm.head_dim, lm.hidden_size, T - 1
    a = dec._score_buffers(B * K * Tq)
    l = lm.num_hidden_layers - 1
    run = lambda: decode.attn_suffix_shared(a["qkv"], a["qkv"].stride(0), c.kp[l], c.vp[l], dec.mask[::K], c.ksfx[l], c.vsfx[l], a["ao"], B, K, H,
                                            hd, c.Sp, c.S0, c.Tmax, Tq, hd ** -0.5)
    run()
    torch.cuda.synchronize()
    ms, _ = event_ms(lambda: [run() for _ in range(reps)])
    es, tiles = a["qkv"].element_size(), -(-K * Tq // 32)
    rows = B * K * Tq
    model = {"q_and_out": 2 * rows * d * es, "prompt_kv_per_tile": B * H * tiles * 2 * c.S0 * hd * es, "prompt_kv_once": B * H * 2 * c.S0 * hd * es,
             "suffix_kv": B * K * H * 2 * Tq * hd * es}
    return {"us_per_layer": round(ms / reps * 1e3, 1), "workgroups": B * H * tiles, "modelled_bytes": model}


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", default="4,16")
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default="ABC")
    ap.add_argument("--fwd_clips", type=int, default=2, help="arm B: clips per model.forward() call")
    a = ap.parse_args()
    m, dims = model_7b(a.layers)
    B, T = a.batch, a.T
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = {"prompt_len": Lp, "T": T, "clips": B, "layers": dims.lm.num_hidden_layers, "rounds": a.rounds, "clocks_before": clocks(), "K": {}}
    for K in [int(k) for k in a.K.split(",")]:
        gkw = dict(input_ids=ids, attention_mask=mask, point_clouds=pcs, fps_start=st, max_length=T, num_return_sequences=K, eos_token_id=None,
                   seed=5, share_prompt=True, output_logprobs=True)
        gen = m.generate(**gkw)                                       # (captures the loop: arm C's warm-up)
        cand = gen.sequences[:, Lp:].reshape(B, K, T)
        arms = {"A": lambda: m.score(ids, mask, pcs, cand, fps_start=st, eos_token_id=None).token_logprobs,
                "B": lambda: forward_logprobs(m, ids, mask, pcs, st, cand, a.fwd_clips),
                "C": lambda: m.generate(**gkw).token_logprobs}
        arms = {n: f for n, f in arms.items() if n in a.arms}
        last = {n: f() for n, f in arms.items()}                      # warm-up round: every shape of the timed window
        ms = {n: [] for n in arms}
        for _ in range(a.rounds):
            for n, f in arms.items():
                t, last[n] = event_ms(f)
                ms[n].append(t)
        rec = {n: {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2),
                   "spread": round((max(v) - min(v)) / statistics.median(v), 4), "runs_ms": [round(x, 2) for x in v]} for n, v in ms.items()}
        med = {n: statistics.median(v) for n, v in ms.items()}
        if "A" in med and "B" in med:
            rec["A_over_B"] = round(med["A"] / med["B"], 4)
            rec["max_abs_A_minus_B"] = float((last["A"] - last["B"]).abs().max())
        if "A" in med and "C" in med:
            rec["A_over_C"] = round(med["A"] / med["C"], 4)
            rec["max_abs_A_minus_C"] = float((last["A"] - last["C"]).abs().max())
        rec["token_rows"] = {"A": B * Lp + B * K * (T - 1), "B": B * K * (Lp + T)}
        if "A" in arms:
            rec["attn_suffix_shared"] = kernel_only(m, B, K, T)
        out["K"][str(K)] = rec
        m._decoders.clear()
        m._scorers.clear()
        torch.cuda.empty_cache()
    out["clocks_after"] = clocks()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
