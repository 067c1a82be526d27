#!/usr/bin/env python3
"""FP8 (e4m3fn) weights of the decode-step projections against bf16 weights, 7B shapes, seeded weights (tools/bench_decode_kv8.py's model),
both arms in one process, graph replays alternated:
  (a) bs 8, S0 ~= 540, 152 sampled tokens, as generate() runs in validation: seconds per generate() call, ms per step (replay of the
      captured token loop);
  (b) 8 clips x 4 beams, 152 steps (tools/bench_beam.py's shape): seconds per call, ms per step;
  (c) BASELINE.json config 5: bs 256, 32 greedy steps, with kv_cache_dtype auto and fp8: ms per step.
Per arm: algorithmic bytes per step (weights once, K/V of every key, scales, key mask) and the fraction of 8 TB/s.  Also the teacher-forced
logit error of fp8 weights against bf16 weights (relative Frobenius norm over the steps) at 2 and 32 layers.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` separately.
GPU box only:  python tools/bench_decode_w8.py [--layers N] [--reps 3] [--shapes abc] [--err 1]"""
import argparse, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch
from bench_decode_kv8 import inputs, model_7b
from egoscaler_amd.decode import Decoder, argmax_rows


def weight_bytes(m, wd):
    """Bytes of weights one decode step reads: the four projections (codes + one fp32 scale per row with fp8), norms, lm_head."""
    lm = m.dims.lm
    proj = lm.num_hidden_layers * (4 * lm.hidden_size ** 2 + 3 * lm.hidden_size * lm.intermediate_size)
    rows = lm.num_hidden_layers * (4 * lm.hidden_size + 2 * lm.intermediate_size + lm.hidden_size)    # q|k|v, o, gate|up, down
    rest = (lm.vocab_size * lm.hidden_size + (2 * lm.num_hidden_layers + 1) * lm.hidden_size) * 2
    return (proj + 4 * rows if wd == "fp8" else 2 * proj) + rest


def kv_bytes(m, rows, S0, T, kv):
    """K / V bytes (codes + scales with fp8) and key-mask bytes every step reads, summed over steps 1 .. T-1."""
    lm = m.dims.lm
    per_key = 2 * lm.hidden_size * (1 if kv == "fp8" else 2) + (2 * lm.num_attention_heads * 4 if kv == "fp8" else 0) + lm.num_attention_heads
    return sum(rows * (S0 + t + 1) * per_key * lm.num_hidden_layers for t in range(T - 1))


def arm_stats(m, ms_step, rows, S0, T, kv, wd):
    alg = weight_bytes(m, wd) + kv_bytes(m, rows, S0, T, kv) / (T - 1)
    return {"ms_per_step": round(ms_step, 3), "GB_per_step": round(alg / 1e9, 3), "frac_8TBs": round(alg / (ms_step * 1e-3) / 8e12, 4)}


def _replay_ms(dec, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dec.graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _dec(m, wd):
    decs = [d for d in m._decoders.values() if (d.w8 is not None) == (wd == "fp8")]
    assert len(decs) == 1
    return decs[0]


@torch.no_grad()
def generate_shape(m, dims, B, T, reps, beams=1):
    """(a) / (b): generate() per call (prefill + captured loop) and ms per step of the loop's replay, arms alternated."""
    ids, pcs, st = inputs(dims, B, distinct=B)
    S0 = ids.shape[1]
    kw = dict(input_ids=ids, point_clouds=pcs, fps_start=st, max_length=T, eos_token_id=None)
    kw.update(dict(num_beams=beams, do_sample=False) if beams > 1 else dict(do_sample=True, seed=5))
    arms = {None: {"s": [], "ms": []}, "fp8": {"s": [], "ms": []}}
    for wd in arms:                                                    # capture both loops first
        m.generate(**kw, decode_weight_dtype=wd)
    torch.cuda.synchronize()
    for _ in range(reps):
        for wd, a in arms.items():
            t0 = time.perf_counter()
            m.generate(**kw, decode_weight_dtype=wd)
            torch.cuda.synchronize()
            a["s"].append(time.perf_counter() - t0)
            a["ms"].append(_replay_ms(_dec(m, wd)) / (T - 1))
    out = {"rows": B * beams, "prompt_len": S0, "new_tokens": T}
    for wd, a in arms.items():
        ms = sorted(a["ms"])[len(a["ms"]) // 2]
        r = arm_stats(m, ms, B * beams, S0, T, None, wd)
        r["s_per_call"] = round(sorted(a["s"])[len(a["s"]) // 2], 4)
        r["ms_all"] = [round(x, 3) for x in a["ms"]]
        out["fp8" if wd else "bf16"] = r
    m.__dict__.pop("_decoders", None)
    torch.cuda.empty_cache()
    return out


@torch.no_grad()
def config5(m, dims, B, T, reps, kv, prefill_chunk=16):
    """(c): greedy decode on static buffers (tools/bench_decode_kv8.py's loop), bf16 and fp8 weights over one KV dtype."""
    ids, pcs, st = inputs(dims, B)
    S0 = ids.shape[1]
    arms = {}
    for wd in (None, "fp8"):
        dec = Decoder(m.engine, B, S0 + T, kv_dtype=kv, weight_dtype=wd)
        dec.prefill_chunked(ids, None, pcs, st, T, chunk=prefill_chunk)
        lg0 = dec.lg.clone()
        dec.greedy(T, use_graph=True, keep_scores=False)
        torch.cuda.synchronize()
        arms[wd] = dict(dec=dec, lg0=lg0, ms=[])
    for _ in range(reps):
        for wd, a in arms.items():
            a["dec"].lg.copy_(a["lg0"])
            a["ms"].append(_replay_ms(a["dec"]) / (T - 1))
    out = {"rows": B, "prompt_len": S0, "steps": T, "kv_cache_dtype": kv or "auto"}
    for wd, a in arms.items():
        r = arm_stats(m, sorted(a["ms"])[len(a["ms"]) // 2], B, S0, T, kv, wd)
        r["ms_all"] = [round(x, 3) for x in a["ms"]]
        out["fp8" if wd else "bf16"] = r
        del a["dec"]
    torch.cuda.empty_cache()
    return out


@torch.no_grad()
def teacher_forced_error(m, dims, B=8, steps=16, distinct=8):
    """Relative Frobenius error of the fp8-weight logits against the bf16-weight logits over `steps` single-token steps on the bf16 run's
    greedy tokens (both decoders read the same tokens and start from the same prefill, so the error does not compound through diverging
    sequences)."""
    ids, pcs, st = inputs(dims, B, distinct)
    S0 = ids.shape[1]
    d16, d8 = Decoder(m.engine, B, S0 + steps + 1), Decoder(m.engine, B, S0 + steps + 1, weight_dtype="fp8")
    d16.prefill(ids, None, pcs, st, steps + 1)
    for n in ("kc", "vc", "lg", "seq_buf", "mask_buf"):                # one prefill: the fp8 arm starts from the bf16 arm's state
        getattr(d8, n).copy_(getattr(d16, n))
    d8.mask, d8.seq, d8.pos = d8.mask_buf, d8.seq_buf[:, :d16.seq.shape[1]], d16.pos
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


def run(layers=None, reps=3, shapes="abc", err=True, steps=152):
    m, dims = model_7b(layers)
    out = {"metric": "decode with fp8 (e4m3fn) vs bf16 projection weights, 7B shapes, seeded weights", "layers": dims.lm.num_hidden_layers,
           "reps": reps}
    if "a" in shapes:
        out["a_bs8_sampled"] = generate_shape(m, dims, 8, steps, reps)
    if "b" in shapes:
        out["b_8x4_beams"] = generate_shape(m, dims, 8, steps, reps, beams=4)
    if "c" in shapes:
        out["c_config5"] = [config5(m, dims, 256, 32, reps, kv) for kv in (None, "fp8")]
    if err:
        out["teacher_forced_rel_err"] = {f"{dims.lm.num_hidden_layers}_layers_bs8": round(teacher_forced_error(m, dims, 8, 16), 5)}
        if dims.lm.num_hidden_layers != 2:
            del m
            torch.cuda.empty_cache()
            m2, dims2 = model_7b(2)
            out["teacher_forced_rel_err"]["2_layers_bs8"] = round(teacher_forced_error(m2, dims2, 8, 16), 5)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--steps", type=int, default=152, help="new tokens of shapes (a) and (b)")
    ap.add_argument("--err", type=int, default=1, help="teacher-forced logit error at this model's depth and at 2 layers (0: skip)")
    a = ap.parse_args()
    print(json.dumps(run(a.layers, a.reps, a.shapes, bool(a.err), a.steps)))
