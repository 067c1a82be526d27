#!/usr/bin/env python3
"""The fp8 (e4m3fn) KV cache against the bf16 one at BASELINE.json config 5: inference-only greedy decode, bs=256, prefill S0~=540 once,
then 32 single-token steps captured into ONE hipGraph, seeded weights (tools/bench_decode.py's setup).  Both arms live in one process
and their graphs are replayed alternately.  Per arm: ms/step, tokens/s, algorithmic bytes (weights + K/V codes or bf16 rows + scales +
key mask, per step) and the fraction of 8 TB/s.  Also the teacher-forced logit error of the fp8 cache (both decoders step on the bf16
arm's tokens; relative Frobenius norm over all steps).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` separately.
GPU box only:  python tools/bench_decode_kv8.py [--batch 256] [--steps 32] [--layers N] [--reps 5]"""
import argparse, json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egoscaler_amd import synth
from egoscaler_amd.config import dims_7b
from egoscaler_amd.decode import Decoder, argmax_rows
from egoscaler_amd.pointllm import TrajPointLLMForCausalLM


def model_7b(layers=None):
    """bf16 7B-width model (optionally fewer layers) with tools/bench_decode.py's seeded weights."""
    dims = dims_7b()
    if layers:
        dims.lm.num_hidden_layers = layers
    dev = torch.device("cuda")
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=256, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device=dev, dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        for n, p in list(m.named_parameters()) + list(m.named_buffers()):
            leaf = n.rsplit(".", 1)[-1]
            if leaf == "num_batches_tracked":
                continue
            if leaf == "running_var" or (leaf == "weight" and p.dim() == 1):
                p.fill_(1.0)
            elif leaf == "running_mean":
                p.zero_()
            else:
                fan = p[0].numel() if p.dim() > 1 else p.numel()
                for r0 in range(0, p.shape[0], 8192):
                    blk = p[r0:r0 + 8192]
                    blk.copy_(torch.empty(blk.shape, dtype=torch.float32, device=dev).normal_(0, 0.02 if fan >= 1024 else min(0.35, fan ** -0.5), generator=g))
    return m.eval(), dims


def inputs(dims, B, distinct=1):
    """B prompt rows (`distinct` different prompts / clouds, repeated), their clouds and FPS starts."""
    dev = torch.device("cuda")
    toks, _, Lp = synth.synth_batch(dims, distinct, text_len=16, num_steps=20, max_traj_token=160)
    reps = -(-B // distinct)
    ids = toks[:, :Lp].repeat(reps, 1)[:B].to(dev)
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(distinct)]).repeat(reps, 1, 1)[:B].to(dev)
    return ids, pcs, torch.zeros(B, dtype=torch.int32, device=dev)


@torch.no_grad()
def teacher_forced_error(m, dims, B=8, steps=16, distinct=8):
    """Relative Frobenius error of the fp8 cache's logits against the bf16 cache's, over `steps` single-token steps on the bf16 run's greedy
    tokens (both decoders read the same tokens, so the error does not compound through diverging sequences)."""
    ids, pcs, st = inputs(dims, B, distinct)
    S0 = ids.shape[1]
    d16, d8 = Decoder(m.engine, B, S0 + steps + 1), Decoder(m.engine, B, S0 + steps + 1, kv_dtype="fp8")
    for dec in (d16, d8):
        dec.prefill(ids, None, pcs, st, steps + 1)
    num = den = 0.0
    for t in range(steps):
        argmax_rows(d16.lg, d16.tok.view(-1))
        d8.tok.copy_(d16.tok)
        d16.step(S0 + t)
        d8.step(S0 + t)
        a, b = d16.lg.float(), d8.lg.float()
        num += float((b - a).pow(2).sum())
        den += float(a.pow(2).sum())
    return (num / den) ** 0.5


def run(batch=256, steps=32, layers=None, reps=5, prefill_chunk=16, err_batch=8):
    m, dims = model_7b(layers)
    lm = dims.lm
    B, T = batch, steps
    ids, pcs, st = inputs(dims, B)
    S0 = ids.shape[1]
    arms = {}
    for kv in (None, "fp8"):
        dec = Decoder(m.engine, B, S0 + T, kv_dtype=kv)
        dec.prefill_chunked(ids, None, pcs, st, T, chunk=prefill_chunk)
        lg0 = dec.lg.clone()
        dec.greedy(T, use_graph=True, keep_scores=False)               # capture + first replay
        torch.cuda.synchronize()
        arms[kv] = dict(dec=dec, lg0=lg0, seq0=dec.seq.clone(), ms=[])
    for _ in range(reps):                                              # alternate the arms
        for kv, a in arms.items():
            dec = a["dec"]
            dec.lg.copy_(a["lg0"])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dec.graph.replay()
            e1.record()
            torch.cuda.synchronize()
            a["ms"].append(e0.elapsed_time(e1))
    p_llm = sum(p.numel() for n, p in m.named_parameters() if n.startswith(("model.layers.", "lm_head", "model.norm"))) * 2
    out = {"metric": "decode ms/step, fp8 vs bf16 KV cache (bs=%d, %d steps, hipGraph, greedy)" % (B, T), "prompt_len": S0, "layers": lm.num_hidden_layers,
           "reps": reps}
    for kv, a in arms.items():
        ms = sorted(a["ms"])[len(a["ms"]) // 2]
        # per step t (positions 0 .. S0 + t): weights once, K and V of every key of every layer, scales (fp8), the key mask row
        per_key = 2 * lm.hidden_size * (1 if kv == "fp8" else 2) + (2 * lm.num_attention_heads * 4 if kv == "fp8" else 0)
        kv_bytes = sum(B * (S0 + t + 1) * per_key * lm.num_hidden_layers for t in range(T - 1))
        mask_bytes = sum(B * (S0 + t + 1) * lm.num_attention_heads * lm.num_hidden_layers for t in range(T - 1))
        alg = (T - 1) * p_llm + kv_bytes + mask_bytes
        out["fp8" if kv else "bf16"] = {"ms_per_step": round(ms / (T - 1), 3), "tokens_per_s": round(B * T / (ms * 1e-3), 1),
                                        "algorithmic_GB": round(alg / 1e9, 2), "kv_GB": round(kv_bytes / 1e9, 2),
                                        "frac_8TBs": round(alg / (ms * 1e-3) / 8e12, 4), "ms_all": [round(x, 2) for x in a["ms"]],
                                        "deterministic_replay": bool(torch.equal(a["seq0"], a["dec"].seq)),
                                        "cache_GB": round(sum(t.numel() * t.element_size() for t in a["dec"].cache.tensors()) / 1e9, 2)}
        del a["dec"]
    torch.cuda.empty_cache()
    if err_batch:
        out["teacher_forced_rel_err"] = {"batch": err_batch, "steps": 16, "value": round(teacher_forced_error(m, dims, err_batch, 16), 5)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--err_batch", type=int, default=8, help="batch of the teacher-forced error run (0: skip)")
    a = ap.parse_args()
    print(json.dumps(run(a.batch, a.steps, a.layers, a.reps, err_batch=a.err_batch)))
