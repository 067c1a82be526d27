#!/usr/bin/env python3
"""Int4 (group-scaled, csrc/w4.hip) against fp8 (csrc/w8.hip) and bf16 weights of the decode-step projections, 7B shapes, seeded weights
(tools/bench_decode_kv8.py's model), the three arms in one process, graph replays alternated:
  (1) bs 1 greedy, 152 tokens; (a) bs 8 greedy, 152 tokens; (b) 8 clips x 4 beams, 152 steps: seconds per generate() call and ms per step
      (replay of the captured token loop);
  (c) bs 256, 32 greedy steps on static buffers: ms per step.
Per arm: bytes of projection weights per step, resident decode-weight bytes, algorithmic bytes per step and the fraction of 8 TB/s.  Also
the teacher-forced logit error of each quantized arm against bf16 weights.  --gemv 1: the four 7B projections alone, M = 1 / 8, fp8 and int4
kernels in a loop (for a `rocprofv3 --kernel-trace --stats` pass of its own).
GPU box only:  python tools/bench_decode_w4.py [--layers N] [--reps 3] [--shapes 1abc] [--err 1] [--gemv 0]"""
import argparse, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch
from bench_decode_kv8 import inputs, model_7b
from bench_decode_w8 import _replay_ms, kv_bytes
from egoscaler_amd import ops
from egoscaler_amd.decode import Decoder, argmax_rows

ARMS = (None, "fp8", "int4")
NAME = {None: "bf16", "fp8": "fp8", "int4": "int4"}


def proj_bytes(m, wd):
    """Bytes of the four projections' weights one decode step reads: bf16 elements, fp8 codes + one fp32 scale per row, or int4 codes +
    one fp32 scale per row and 128-column group."""
    lm = m.dims.lm
    d, f, L = lm.hidden_size, lm.intermediate_size, lm.num_hidden_layers
    elems = L * (4 * d * d + 3 * d * f)
    if wd is None:
        return 2 * elems
    if wd == "fp8":
        return elems + 4 * L * (4 * d + 2 * f + d)
    ng = lambda k: -(-k // 128)
    return elems // 2 + 4 * L * ((4 * d + 2 * f) * ng(d) + d * ng(f))


def resident_bytes(dec):
    """Bytes of the decoder's quantized projection copies (0 on the model's weights)."""
    return sum(t.numel() * t.element_size() for lay in (dec.wq or []) for pair in lay.values() for t in pair)


def arm_stats(m, ms_step, rows, S0, T, kv, wd):
    lm = m.dims.lm
    rest = (lm.vocab_size * lm.hidden_size + (2 * lm.num_hidden_layers + 1) * lm.hidden_size) * 2
    alg = proj_bytes(m, wd) + rest + kv_bytes(m, rows, S0, T, kv) / (T - 1)
    return {"ms_per_step": round(ms_step, 3), "proj_GB_per_step": round(proj_bytes(m, wd) / 1e9, 3), "GB_per_step": round(alg / 1e9, 3),
            "frac_8TBs": round(alg / (ms_step * 1e-3) / 8e12, 4)}


def _dec(m, wd):
    fmt = lambda d: "fp8" if d.w8 is not None else "int4" if d.w4 is not None else None
    decs = [d for d in m._decoders.values() if fmt(d) == wd]
    assert len(decs) == 1
    return decs[0]


@torch.no_grad()
def generate_shape(m, dims, B, T, reps, beams=1):
    """generate() per call (prefill + captured loop) and ms per step of the loop's replay, one arm after the other within a repetition.
    The model keeps two decoders, so each arm's call re-captures when a third arm pushed it out: s_per_call is taken on the second of two
    consecutive calls of the arm."""
    ids, pcs, st = inputs(dims, B, distinct=B)
    S0 = ids.shape[1]
    kw = dict(input_ids=ids, point_clouds=pcs, fps_start=st, max_length=T, eos_token_id=None, do_sample=False)
    if beams > 1:
        kw.update(num_beams=beams)
    arms = {wd: {"s": [], "ms": []} for wd in ARMS}
    out = {"rows": B * beams, "prompt_len": S0, "new_tokens": T}
    for _ in range(reps):
        for wd, a in arms.items():
            m.generate(**kw, decode_weight_dtype=wd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(**kw, decode_weight_dtype=wd)
            torch.cuda.synchronize()
            a["s"].append(time.perf_counter() - t0)
            dec = _dec(m, wd)
            a["ms"].append(_replay_ms(dec) / (T - 1))
            a["resident"] = resident_bytes(dec)
    for wd, a in arms.items():
        r = arm_stats(m, sorted(a["ms"])[len(a["ms"]) // 2], B * beams, S0, T, None, wd)
        r["s_per_call"] = round(sorted(a["s"])[len(a["s"]) // 2], 4)
        r["resident_decode_weight_GB"] = round(a["resident"] / 1e9, 3)
        r["ms_all"] = [round(x, 3) for x in a["ms"]]
        out[NAME[wd]] = r
    m.__dict__.pop("_decoders", None)
    torch.cuda.empty_cache()
    return out


@torch.no_grad()
def config5(m, dims, B, T, reps, kv=None, prefill_chunk=16):
    """(c): greedy decode on static buffers (tools/bench_decode_kv8.py's loop), the three weight formats over one KV dtype."""
    ids, pcs, st = inputs(dims, B)
    S0 = ids.shape[1]
    arms = {}
    for wd in ARMS:
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
        out[NAME[wd]] = r
        del a["dec"]
    torch.cuda.empty_cache()
    return out


@torch.no_grad()
def teacher_forced_error(m, dims, B=8, steps=16, distinct=8, weight_dtype="int4"):
    """Relative Frobenius error of the quantized-weight logits against the bf16-weight logits over `steps` single-token steps on the bf16
    run's greedy tokens (both decoders read the same tokens and start from the same prefill, so the error does not compound through
    diverging sequences)."""
    ids, pcs, st = inputs(dims, B, distinct)
    S0 = ids.shape[1]
    d16, dq = Decoder(m.engine, B, S0 + steps + 1), Decoder(m.engine, B, S0 + steps + 1, weight_dtype=weight_dtype)
    d16.prefill(ids, None, pcs, st, steps + 1)
    for n in ("kc", "vc", "lg", "seq_buf", "mask_buf"):                # one prefill: the quantized arm starts from the bf16 arm's state
        getattr(dq, n).copy_(getattr(d16, n))
    dq.mask, dq.seq, dq.pos = dq.mask_buf, dq.seq_buf[:, :d16.seq.shape[1]], d16.pos
    num = den = 0.0
    for t in range(steps):
        argmax_rows(d16.lg, d16.tok.view(-1))
        dq.tok.copy_(d16.tok)
        d16.step(S0 + t)
        dq.step(S0 + t)
        a, b = d16.lg.float(), dq.lg.float()
        num += float((b - a).pow(2).sum())
        den += float(a.pow(2).sum())
    return (num / den) ** 0.5


@torch.no_grad()
def gemv(iters=50):
    """The four 7B projections alone at M = 1 and 8, fp8 and int4 slab products back to back: event times and achieved TB/s of the weight
    bytes (codes + scales); under rocprofv3 --kernel-trace --stats the per-kernel times."""
    out = {}
    ws = torch.empty(128 << 20, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (N, K) in {"qkv": (12288, 4096), "o": (4096, 4096), "gu": (22016, 4096), "down": (4096, 11008)}.items():
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
        q8, q4 = ops.quantize_rows_fp8(w), ops.quantize_rows_int4(w)
        for M in (1, 8):
            x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
            for fmt, q, mm in (("fp8", q8, ops.mm_w8_slabs), ("int4", q4, ops.mm_w4_slabs)):
                for _ in range(5):
                    mm(x, *q, ws)
                graph = torch.cuda.CUDAGraph()                            # one graph of `iters` launches: no launch gaps in the timed window
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                    for _ in range(iters):
                        mm(x, *q, ws)
                torch.cuda.current_stream().wait_stream(side)
                graph.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / iters * 1e3
                nbytes = sum(t.numel() * t.element_size() for t in q)
                out[f"{name}_M{M}_{fmt}"] = {"us": round(us, 2), "TBs": round(nbytes / us / 1e6, 3)}
    return out


def run(layers=None, reps=3, shapes="1abc", err=True, steps=152):
    m, dims = model_7b(layers)
    out = {"metric": "decode with int4 vs fp8 vs bf16 projection weights, 7B shapes, seeded weights", "layers": dims.lm.num_hidden_layers,
           "reps": reps}
    if "1" in shapes:
        out["bs1_greedy"] = generate_shape(m, dims, 1, steps, reps)
    if "a" in shapes:
        out["a_bs8_greedy"] = generate_shape(m, dims, 8, steps, reps)
    if "b" in shapes:
        out["b_8x4_beams"] = generate_shape(m, dims, 8, steps, reps, beams=4)
    if "c" in shapes:
        out["c_bs256"] = config5(m, dims, 256, 32, reps)
    if err:
        out["teacher_forced_rel_err"] = {f"{dims.lm.num_hidden_layers}_layers_bs8_{wd}": round(teacher_forced_error(m, dims, 8, 16, weight_dtype=wd), 5)
                                         for wd in ("fp8", "int4")}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="1abc")
    ap.add_argument("--steps", type=int, default=152, help="new tokens of the generate() shapes")
    ap.add_argument("--err", type=int, default=1, help="teacher-forced logit error of fp8 and int4 weights at this model's depth (0: skip)")
    ap.add_argument("--gemv", type=int, default=0, help="1: only the four projections' kernels in a loop")
    a = ap.parse_args()
    print(json.dumps(gemv() if a.gemv else run(a.layers, a.reps, a.shapes, bool(a.err), a.steps)))
