#!/usr/bin/env python3
"""What generate(output_logprobs=True) costs at 7B in the best-of-K shape of tools/bench_best_of_k.py: 8 clips x K = 16 samples, a
540-token prompt, 64 new tokens, share_prompt=True, do_sample with the reference's top_k / top_p.
  --mode parent   generate(num_return_sequences=K, share_prompt=True) and nothing newer: this file also runs from a checkout of the parent
                  commit (the A/B's parent arm; it imports that checkout's package and tools/bench_best_of_k.py)
  --mode off      the same call on this tree (output_logprobs left False): must time like the parent
  --mode on       output_logprobs=True: one egomi_token_logprob launch per step inside the captured loop + egomi_seq_rank after it
Per mode: ms per decode step (replay of the captured token loop, best of 2 after a warm-up, / (steps - 1)) and the whole generate() call.
--mode on also times the three new kernels alone, each as 64 launches captured into one hipGraph (replay / 64, best of 3):
egomi_token_logprob on the decoder's own logits buffer [8 * K, V] bf16 (bytes read = rows * V * 2), egomi_seq_rank and egomi_traj_medoid
(B = 8, Tmax = 20, D = 6) at K = 16 and 32.  Prints one JSON line.  Alternate the arms on one box in one session; the spread between two
runs of the same arm is the resolution of the comparison.
GPU box only:  python tools/bench_select.py --mode on [--K 16] [--layers N] [--steps 64]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench_best_of_k import clocks, model_7b, timed
from egoscaler_amd import synth


def graph_us(fn, n=64, reps=3):
    """fn() launched n times inside one captured graph: microseconds per launch, best of `reps` replays after a warm-up."""
    from egoscaler_amd.decode import _capture
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        for _ in range(n):
            fn()
    return timed(g.replay, reps) * 1e3 / n


def kernels(dec, K, V):
    from egoscaler_amd import decode, traj
    R = dec.B
    tok = torch.randint(0, V, (R,), device="cuda")
    dec._lp_buffers()
    out = {"rows": R, "V": V, "bytes_read": R * V * dec.lg.element_size()}
    us = graph_us(lambda: decode.token_logprob(dec.lg, tok, None, None, dec.lp_tok, 0, dec.lp_sum, dec.lp_n))
    out["token_logprob_us"] = round(us, 2)
    out["token_logprob_GBps"] = round(out["bytes_read"] / (us * 1e-6) / 1e9, 1)
    g = torch.Generator(device="cuda").manual_seed(3)
    for k in (16, 32):
        s = -torch.rand(8 * k, device="cuda", generator=g) * 60
        n = torch.randint(1, 65, (8 * k,), device="cuda", generator=g).to(torch.int32)
        score = torch.empty(8, k, dtype=torch.float32, device="cuda")
        order = torch.empty(8, k, dtype=torch.int32, device="cuda")
        from egoscaler_amd._lib import c_f, c_i, call
        from egoscaler_amd.ops import P, S
        out[f"seq_rank_K{k}_us"] = round(graph_us(lambda: call("egomi_seq_rank", P(s), P(n), c_i(8), c_i(k), c_f(1.0), P(score), P(order), S())), 2)
        gen = torch.randn(8, k, 20, 6, device="cuda", generator=g)
        ng = torch.randint(1, 21, (8, k), device="cuda", generator=g).to(torch.int32)
        cost = torch.empty(8, k, dtype=torch.float64, device="cuda")
        pick = torch.empty(8, dtype=torch.int32, device="cuda")
        out[f"traj_medoid_K{k}_us"] = round(graph_us(lambda: call("egomi_traj_medoid", P(gen), P(ng), c_i(8), c_i(k), c_i(20), c_i(6), P(cost), P(pick), S())), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("parent", "off", "on"), required=True)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    m, dims = model_7b(a.layers)
    B, T, K = a.batch, a.steps, a.K
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    kw = dict(input_ids=ids, attention_mask=mask, point_clouds=pcs, fps_start=st, max_length=T, num_return_sequences=K, eos_token_id=None, seed=5,
              share_prompt=True)
    if a.mode == "on":
        kw["output_logprobs"] = True
    out = {"mode": a.mode, "prompt_len": Lp, "new_tokens": T, "clips": B, "K": K, "layers": dims.lm.num_hidden_layers, "clocks_before": clocks()}
    res = []
    ms_gen = timed(lambda: res.append(m.generate(**kw)))              # the first call captures the loop, the timed ones replay it
    dec = list(m._decoders.values())[-1]
    loops = [timed(dec.graph.replay, 1) for _ in range(2)]
    out.update({"ms_per_step": round(min(loops) / max(1, T - 1), 4), "ms_per_step_runs": [round(x / max(1, T - 1), 4) for x in loops],
                "generate_s": round(ms_gen * 1e-3, 4), "graphs": len(dec._graphs)})
    if a.mode == "on":
        o = res[-1]
        out["finite"] = bool(torch.isfinite(o.token_logprobs).all()) and bool((o.sequences_lengths == T).all())
        out["mean_token_logprob"] = round(float(o.token_logprobs.mean()), 4)
        out["kernels"] = kernels(dec, K, dims.lm.vocab_size)
    out["clocks_after"] = clocks()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
