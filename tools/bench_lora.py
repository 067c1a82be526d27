"""LoRA training-step cost at the bench geometry (7B, bf16, bs 8, the bench's synthetic batch): frozen LLM against LoRA r=16 on q_proj,v_proj
and on all seven projections, in ONE process with the arms alternating round by round (box drift hits every arm alike).  One step =
loss_and_backward + EgoAdamW.step(overlap=True), as bench.py's frozen step.  Prints one JSON line: ms/step (median over rounds) and peak
memory per arm, the ratios to the frozen arm and the adapter parameter counts.

  python tools/bench_lora.py [--layers 32] [--rounds 5] [--steps 5] [--arms frozen,qv,all7]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = {"frozen": None, "qv": "q_proj,v_proj", "all7": "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"}


def build(dims, targets, r, dev):
    from egoscaler_amd.optim import EgoAdamW
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    margs = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=256, model_name=None,
                                  lora_r=r if targets else 0, lora_alpha=16, lora_target_modules=targets)
    model = TrajPointLLMForCausalLM(margs, dims, None, device=dev, dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for n, p in list(model.named_parameters()) + list(model.named_buffers()):
            leaf = n.rsplit(".", 1)[-1]
            if leaf == "num_batches_tracked" or ".lora_A." in n:
                continue
            if leaf == "running_var" or (leaf == "weight" and p.dim() == 1):
                p.fill_(1.0)
            elif leaf == "running_mean":
                p.zero_()
            else:
                fan_in = p[0].numel() if p.dim() > 1 else p.numel()
                std = 0.02 if fan_in >= 1024 else min(0.35, fan_in ** -0.5)
                for r0 in range(0, p.shape[0], 4096):
                    blk = p[r0:r0 + 4096]
                    blk.copy_(torch.empty(blk.shape, dtype=torch.float32, device=dev).normal_(0, std, generator=g))
    model.engine.prepared = False
    model.train()
    return model, EgoAdamW(model, lr=2e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arms", default="frozen,qv,all7")
    a = ap.parse_args()
    from egoscaler_amd import synth
    from egoscaler_amd.config import dims_7b
    dev = torch.device("cuda", 0)
    dims = dims_7b()
    dims.lm.num_hidden_layers = a.layers
    B = a.batch
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    toks, masks = toks.to(dev), masks.to(dev)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).to(dev)
    start = torch.zeros(B, dtype=torch.long)
    arms = a.arms.split(",")
    models, peak, times = {}, {}, {k: [] for k in arms}
    for k in arms:
        models[k] = build(dims, ARMS[k], a.r, dev)

    def step(k):
        m, opt = models[k]
        m.loss_and_backward(toks, masks, pts, Lp, dims.tok.pad, fps_start=start)
        opt.step(overlap=True)

    for k in arms:                                            # warm-up and peak memory of one arm alone
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(a.warmup):
            step(k)
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    for _ in range(a.rounds):
        for k in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(k)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    n_ad = {k: sum(p.numel() for n, p in models[k][0].named_parameters() if ".lora_" in n) for k in arms}
    res = {"layers": a.layers, "batch": B, "seq": int(toks.shape[1]), "r": a.r, "ms_per_step": med,
           "ms_all_rounds": times, "step_activation_peak_gib": peak, "adapter_params": n_ad}
    if "frozen" in med:
        res["ratio_to_frozen"] = {k: med[k] / med["frozen"] for k in arms}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
