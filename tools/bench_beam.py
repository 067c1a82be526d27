#!/usr/bin/env python3
"""Beam search at 7B in the evaluate.py shape: 8 clips, a 540-token prompt (synth_batch(dims, 8, text_len=16, num_steps=20,
max_traj_token=160), as tools/debug/validation_throughput.py), 152 new tokens, num_beams 4; against greedy at B=8 and greedy at B=32
(the same 32 rows as 8 x 4 beams, but 32 unshared prompts).  Each loop is one hipGraph; the time is the replay of all 152 steps.
Prints one JSON line: ms per step and tokens/s of each, and the step's modelled bytes (weights + K/V read; the beam step reads each
prompt's K/V once per item).  --kv_cache_layout split: the beam decoder on the prompt / suffix cache (Decoder(split_cache=True));
both: the dense and the split decoder side by side, their loops timed alternately (--reps rounds), with each arm's cache bytes.
GPU box only:  python tools/bench_beam.py [--layers N] [--steps 152] [--kv_cache_layout dense|split|both]"""
import argparse, json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egoscaler_amd import synth
from egoscaler_amd.config import dims_7b
from egoscaler_amd.decode import Decoder
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


def timed(fn, reps=2):
    fn()                                                              # capture + first replay
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


def timed_once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=152)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kv_cache_layout", default="dense", choices=["dense", "split", "both"])
    ap.add_argument("--reps", type=int, default=2, help="timed replays per arm (both: alternating rounds)")
    ap.add_argument("--no_greedy", action="store_true", help="skip the greedy arms")
    a = ap.parse_args()
    m, dims = model_7b(a.layers)
    eng, lm = m.engine, dims.lm
    B, nb, T = a.batch, a.beams, a.steps
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = {"prompt_len": Lp, "new_tokens": T, "batch": B, "num_beams": nb, "layers": lm.num_hidden_layers}

    arms = {}
    for layout in (("dense", "split") if a.kv_cache_layout == "both" else (a.kv_cache_layout,)):
        dec = Decoder(eng, B * nb, Lp + T, num_beams=nb, **(dict(split_cache=True, max_new_tokens=T) if layout == "split" else {}))
        dec.prefill(ids, mask, pcs, st, T, nb=nb)
        lg0 = dec.lg.clone()

        def beam(dec=dec, lg0=lg0):
            dec.lg.copy_(lg0)
            dec.pos = Lp
            return dec.beam(T, length_penalty=1.0, eos=None, pad=dims.tok.pad)
        arms[layout] = (dec, beam, sum(c.numel() * c.element_size() for c in dec.cache.tensors()))
    for _, beam, _ in arms.values():                                      # capture + first replay of every arm
        beam()
    torch.cuda.synchronize()
    runs = {k: [] for k in arms}
    for _ in range(a.reps):                                               # the arms alternate: one replay each per round
        for k, (_, beam, _) in arms.items():
            runs[k].append(timed_once(beam))
    for k, (dec, _, cache_bytes) in arms.items():
        ms_beam = min(runs[k])
        name = "beam" if k == a.kv_cache_layout or (a.kv_cache_layout == "both" and k == "dense") else "beam_" + k
        out[name] = {"layout": k, "ms_per_step": round(ms_beam / T, 3), "tokens_per_s": round(B * nb * T / (ms_beam * 1e-3), 1),
                     "ms_total": round(ms_beam, 1), "ms_per_step_runs": [round(x / T, 3) for x in runs[k]], "iterations": int(dec.ctl[1]),
                     "cache_GB": round(cache_bytes / 1e9, 3)}
    if "split" in arms and "dense" in arms:
        out["split_over_dense"] = round(out["beam_split"]["ms_per_step"] / out["beam"]["ms_per_step"], 4)
    del arms, dec, beam
    for Bg in (() if a.no_greedy else (B, B * nb)):
        rep = Bg // B
        d2 = Decoder(eng, Bg, Lp + T)
        d2.prefill(ids.repeat(rep, 1), mask.repeat(rep, 1), pcs.repeat(rep, 1, 1), st.repeat(rep), T)
        lg1 = d2.lg.clone()

        def greedy():
            d2.lg.copy_(lg1)
            d2.pos = Lp
            if getattr(d2, "graph", None) is None:
                d2.greedy(T, use_graph=True, keep_scores=False)
            else:
                d2.graph.replay()
        ms = timed(greedy)
        out[f"greedy_b{Bg}"] = {"ms_per_step": round(ms / T, 3), "tokens_per_s": round(Bg * T / (ms * 1e-3), 1), "ms_total": round(ms, 1)}
        del d2
    p_llm = sum(p.numel() for n, p in m.named_parameters() if n.startswith(("model.layers.", "lm_head", "model.norm"))) * 2
    row_kv = 2 * lm.hidden_size * 2 * lm.num_hidden_layers                       # K and V bytes of one position, all layers
    mid = Lp + T // 2
    out["modelled_GB_per_step_mid"] = {
        "weights": round(p_llm / 1e9, 2),
        "beam": round((p_llm + B * Lp * row_kv + B * nb * (mid - Lp) * row_kv) / 1e9, 3),
        "greedy_b%d" % B: round((p_llm + B * mid * row_kv) / 1e9, 3),
        "greedy_b%d" % (B * nb): round((p_llm + B * nb * mid * row_kv) / 1e9, 3)}
    if not a.no_greedy:
        for name in ("beam", "beam_split"):
            if name in out:
                out[name + "_over_greedy_b%d" % B] = round(out[name]["ms_per_step"] / out[f"greedy_b{B}"]["ms_per_step"], 3)
                out[name + "_over_greedy_b%d" % (B * nb)] = round(out[name]["ms_per_step"] / out[f"greedy_b{B * nb}"]["ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
