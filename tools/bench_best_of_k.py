#!/usr/bin/env python3
"""Best-of-K sampling at 7B in the evaluate.py shape: 8 clips, a 540-token prompt (synth_batch(dims, 8, text_len=16, num_steps=20,
max_traj_token=160), as tools/bench_beam.py), 64 new tokens, K samples per clip, do_sample with the reference's top_k / top_p.
  --mode expanded   generate(num_return_sequences=K): HF's expansion, B*K prefills and B*K cached prompts.  Uses nothing newer than that
                    call, so this file also runs on a checkout that predates share_prompt (the A/B's parent arm).
  --mode shared     generate(num_return_sequences=K, share_prompt=True): one prefill and one cached prompt per clip.
Per K: prefill ms (Decoder.prefill on the mode's rows), ms per decode step (replay of the captured token loop, all steps in one hipGraph;
one warm-up replay, best of 2 as tools/bench_beam.py), the whole generate() call, cache bytes, the step's modelled bytes.  The clock
state is recorded around the run as tools/clock_probe.py does.  Prints one JSON line.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` separately (no counters in the same run).
GPU box only:  python tools/bench_best_of_k.py --mode shared [--K 4,16] [--layers N] [--steps 64]"""
import argparse, json, os, subprocess, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egoscaler_amd import synth
from egoscaler_amd.config import dims_7b
from egoscaler_amd.pointllm import TrajPointLLMForCausalLM


def model_7b(layers=None):
    dims = dims_7b()
    if layers:
        dims.lm.num_hidden_layers = layers
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=256, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(7)
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
                    blk.copy_(torch.empty(blk.shape, dtype=torch.float32, device="cuda").normal_(0, 0.02 if fan >= 1024 else min(0.35, fan ** -0.5), generator=g))
    return m.eval(), dims


def clocks():
    """sclk / mclk lines of rocm-smi --showclocks (a read-only query, as tools/clock_probe.py; empty where the tool is missing)."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in out.splitlines() if "sclk" in l or "mclk" in l][:4]
    except Exception as e:                                            # noqa: BLE001
        return [type(e).__name__]


def timed(fn, reps=2):
    fn()                                                              # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("expanded", "shared"), required=True)
    ap.add_argument("--K", default="4,16")
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    m, dims = model_7b(a.layers)
    lm = dims.lm
    B, T = a.batch, a.steps
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = {"mode": a.mode, "prompt_len": Lp, "new_tokens": T, "clips": B, "layers": lm.num_hidden_layers, "clocks_before": clocks(), "K": {}}
    p_llm = sum(p.numel() for n, p in m.named_parameters() if n.startswith(("model.layers.", "lm_head", "model.norm"))) * 2
    row_kv = 2 * lm.hidden_size * 2 * lm.num_hidden_layers                       # K and V bytes of one position, all layers
    extra = {"share_prompt": True} if a.mode == "shared" else {}
    for K in [int(k) for k in a.K.split(",")]:
        kw = dict(input_ids=ids, attention_mask=mask, point_clouds=pcs, fps_start=st, max_length=T, num_return_sequences=K, eos_token_id=None,
                  seed=5, **extra)
        gen = lambda: m.generate(**kw)
        ms_gen = timed(gen)                                           # the first call captures the loop, the timed ones replay it
        dec = list(m._decoders.values())[-1]
        ms_loop = timed(dec.graph.replay)
        if a.mode == "shared":
            pre = lambda: dec.prefill(ids, mask, pcs, st, T)
        else:
            rep = lambda x: x.repeat_interleave(K, 0)
            pre = lambda: dec.prefill(rep(ids), rep(mask), rep(pcs), rep(st), T)
        ms_pre = timed(pre)
        mid = T // 2
        if a.mode == "shared":
            kv_step = B * Lp * row_kv + B * K * mid * row_kv
        else:
            kv_step = B * K * (Lp + mid) * row_kv
        out["K"][str(K)] = {"prefill_ms": round(ms_pre, 2), "ms_per_step": round(ms_loop / max(1, T - 1), 4), "loop_ms": round(ms_loop, 2),
                            "generate_ms": round(ms_gen, 2), "tokens_per_s": round(B * K * T / (ms_gen * 1e-3), 1),
                            "cache_GB": round(sum(t.numel() * t.element_size() for t in dec.cache.tensors()) / 1e9, 3),
                            "modelled_GB_per_step_mid": {"weights": round(p_llm / 1e9, 2), "kv": round(kv_step / 1e9, 3)},
                            "modelled_GBps": round((p_llm + kv_step) / (ms_loop / max(1, T - 1) * 1e-3) / 1e9, 1)}
        del dec
        m._decoders.clear()
        torch.cuda.empty_cache()
    out["clocks_after"] = clocks()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
