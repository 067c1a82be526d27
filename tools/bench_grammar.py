#!/usr/bin/env python3
"""What generate(traj_grammar=...) costs: the kernel alone, and a 7B decode step with it.
  kernel           egomi_traj_grammar_step (csrc/grammar.hip) beside egomi_token_logprob (csrc/logprob.hip), one process, the same shape: 128
                   rows x V = 32262 bf16, the 7B tokenizer's layout (bins p0 = 32006, nb = 256; <ts> <tsep> <te> just below; eos 2), every
                   row at a step boundary that allows the bins and <te>.  The grammar kernel reads the 8.26 MB once and writes all of them
                   but the allowed ids.  LAUNCHES launches captured into one hipGraph, microseconds per launch = replay / LAUNCHES, best of
                   REPS replays after a warm-up; ROUNDS rounds with the arms alternated.  A launch in place on the rows it masked before
                   skips the expf of every -inf, so the kernel is also timed on fresh logits: a copy of the raw rows before every launch,
                   minus the copy timed alone.  The mass of a launch on fresh logits is checked against a float64 softmax, and its rows
                   against the mask.  Prints one JSON line.
  arm --mode M     one generate() arm at 7B in the best-of-K shape of tools/bench_binstats.py: 8 clips x K = 16, a 540-token prompt, 64 new
                   tokens, share_prompt=True, do_sample with the reference's top_k / top_p, eos = the tokenizer's.  parent: the call and
                   nothing newer (this file also runs from a checkout of the parent commit, whose package it then imports); off: the same
                   call on this tree; on: traj_grammar=grammar_spec(tok, 1, 20).  ms per decode step = replay of the captured token loop /
                   (steps - 1), best of 3 after a warm-up.  Prints one JSON line; run the three arms alternated, one process each.
  report           kernel line + arm lines (files of JSON lines) -> the table (default profiles/traj_grammar.txt) and the lines beside it as
                   .json: medians over the rounds, and each arm's own spread next to every difference.  Needs no GPU.
GPU box:  python tools/bench_grammar.py kernel > k.json;  python tools/bench_grammar.py arm --mode on >> arms.jsonl;  ...
          python tools/bench_grammar.py report --kernel k.json --arms arms.jsonl"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAUNCHES, REPS, ROUNDS = 256, 5, 5
ROWS, V, NB = 128, 32262, 256
YARDSTICK_US = 8.79                                                    # egomi_token_logprob on the same bytes, profiles/bin_stats.txt


def graph_us(fn):
    import torch
    from bench_best_of_k import timed
    from egoscaler_amd.decode import _capture
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        for _ in range(LAUNCHES):
            fn()
    return timed(g.replay, REPS) * 1e3 / LAUNCHES


def kernel():
    import torch
    from bench_best_of_k import clocks
    from egoscaler_amd import decode
    spec = (V - NB, NB, V - NB - 3, V - NB - 2, V - NB - 1, 2, 1, 20)    # p0, nb, <ts>, <tsep>, <te>, eos, min_steps, max_steps
    p0, te = spec[0], spec[4]
    g = torch.Generator(device="cuda").manual_seed(3)
    raw = (3 * torch.randn(ROWS, V, device="cuda", generator=g)).to(torch.bfloat16)
    lg = raw.clone()
    tok = torch.randint(0, V, (ROWS,), device="cuda", generator=g)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    lp_tok, lp_sum, lp_n = f32(ROWS, 1), f32(ROWS), torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    state = torch.tensor([[0, 3]] * ROWS, dtype=torch.int32, device="cuda")      # a step boundary, 3 steps closed: the bins and <te>
    mass = f32(ROWS, 1)
    decode.traj_grammar_step(lg, None, state, spec, 50, mass, 0)                 # on fresh logits: what is timed computes what it should
    want = torch.softmax(raw.double(), 1)
    out = {"rows": ROWS, "V": V, "nb": NB, "p0": p0, "dtype": "bf16", "bytes_read": ROWS * V * 2, "launches_per_graph": LAUNCHES, "reps": REPS,
           "mass_err": float((mass[:, 0].double() - (want[:, p0:].sum(1) + want[:, te])).abs().max())}
    keep = torch.zeros(V, dtype=torch.bool, device="cuda")
    keep[p0:] = True
    keep[te] = True
    assert out["mass_err"] < 1e-6, out["mass_err"]
    assert torch.equal(lg[:, keep], raw[:, keep]) and bool(torch.isneginf(lg[:, ~keep]).all())
    fns = {"token_logprob": lambda: decode.token_logprob(raw, tok, None, None, lp_tok, 0, lp_sum, lp_n),
           "traj_grammar_step": lambda: decode.traj_grammar_step(lg, None, state, spec, 50, mass, 0),     # (on the rows it masked before)
           "row_copy": lambda: lg.copy_(raw),
           "copy_then_grammar": lambda: (lg.copy_(raw), decode.traj_grammar_step(lg, None, state, spec, 50, mass, 0))}  # on fresh logits
    out.update({"clocks_before": clocks(), "us": {n: [] for n in fns}})
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            out["us"][n].append(round(graph_us(fn), 2))
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def arm(a):
    import torch
    from bench_best_of_k import clocks, model_7b, timed
    from egoscaler_amd import synth
    m, dims = model_7b(a.layers)
    B, T, K = a.batch, a.steps, a.K
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    kw = dict(input_ids=ids, attention_mask=mask, point_clouds=pcs, fps_start=st, max_length=T, num_return_sequences=K, eos_token_id=dims.tok.eos,
              seed=5, share_prompt=True)
    if a.mode == "on":
        from egoscaler_amd import traj
        kw.update(traj_grammar=traj.grammar_spec(dims.tok, 1, 20))
    out = {"mode": a.mode, "prompt_len": Lp, "new_tokens": T, "clips": B, "K": K, "layers": dims.lm.num_hidden_layers, "clocks_before": clocks()}
    res = []
    ms_gen = timed(lambda: res.append(m.generate(**kw)))              # the first call captures the loop, the timed ones replay it
    dec = list(m._decoders.values())[-1]
    loop = timed(dec.graph.replay, 3)
    out.update({"ms_per_step": round(loop / max(1, T - 1), 4), "generate_s": round(ms_gen * 1e-3, 4), "graphs": len(dec._graphs)})
    if a.mode == "on":
        o = res[-1]
        live = o.grammar_mass > 0
        out["mean_grammar_mass"] = round(float(o.grammar_mass[live].mean()), 5)
        out["rows_closed"] = int((o.sequences[:, Lp:] == dims.tok.eos).any(1).sum())
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.lstrip().startswith("{")]


def render(k, arms, note=None):
    """The lines of profiles/traj_grammar.txt for one kernel line and the arm lines; note: one more header line about the arm runs."""
    us = k["us"]
    med = {n: statistics.median(v) for n, v in us.items()}
    lines = [f"# egomi_traj_grammar_step beside egomi_token_logprob: us per launch, {k['rows']} rows x V = {k['V']} {k['dtype']} (reads rows * V * 2 = "
             f"{k['bytes_read'] / 1e6:.2f} MB and writes all of it but the allowed ids), bins p0 = {k['p0']}, nb = {k['nb']}, every row allowing the bins and <te>.",
             f"# tools/bench_grammar.py kernel; one MI355X, one process; {k['launches_per_graph']} launches captured into one hipGraph, replay / "
             f"{k['launches_per_graph']}, best of {k['reps']}; {len(us['traj_grammar_step'])} rounds with the two arms alternated.",
             f"# sclk / mclk before: {'; '.join(k['clocks_before'])}; after: {'; '.join(k['clocks_after'])}.", ""]
    for n in ("token_logprob", "traj_grammar_step", "row_copy", "copy_then_grammar"):
        lines.append(f"{'egomi_' + n:28s}" + " / ".join(f"{v:.2f}" for v in us[n]) + f"    median {med[n]:.2f} us, spread {max(us[n]) - min(us[n]):.2f} us")
    fresh = med["copy_then_grammar"] - med["row_copy"]
    ratio = fresh / med["token_logprob"]
    lines += ["", f"On fresh logits (copy_then_grammar - row_copy) egomi_traj_grammar_step takes {fresh:.2f} us, on rows it masked before {med['traj_grammar_step']:.2f} us:",
              f"{ratio:.2f}x egomi_token_logprob's time ({fresh:.2f} against {med['token_logprob']:.2f} us; that "
              f"kernel's recorded figure, profiles/bin_stats.txt: {YARDSTICK_US} us).  " +
              ("The expectation (the same latency-bound regime) holds." if ratio < 3 else "The expectation (the same latency-bound regime) is MISSED."),
              f"Worst |mass - float64 softmax mass of the allowed ids| of a launch on fresh logits: {k['mass_err']:.1e}.", ""]
    if arms:
        a0 = arms[0]
        by = {m: [a["ms_per_step"] for a in arms if a["mode"] == m] for m in ("parent", "off", "on")}
        gen = {m: [a["generate_s"] for a in arms if a["mode"] == m] for m in by}
        lines += [f"# generate() at 7B bf16 ({a0['layers']} layers): {a0['clips']} clips x K = {a0['K']} ({a0['clips'] * a0['K']} rows), S0 = {a0['prompt_len']}, "
                  f"{a0['new_tokens']} new tokens, share_prompt=True, do_sample with the reference's top_k 50 / top_p 0.95, eos = the tokenizer's.",
                  "# tools/bench_grammar.py arm; the parent commit's generate() (parent) against this tree with the option off (off) and on (on); one process per",
                  f"# run, the arms alternated in the order of the list below; ms per decode step = graph replay of all steps / {a0['new_tokens'] - 1}, best of 3.",
                  "# order: " + " ".join(a["mode"] for a in arms)] + ([f"# {note}"] if note else []) + [""]
        for m, v in by.items():
            if v:
                lines.append(f"{m:8s} ms per step  " + " / ".join(f"{x:.3f}" for x in v) + f"    median {statistics.median(v):.3f}, spread {max(v) - min(v):.3f}")
        for m, v in gen.items():
            if v:
                lines.append(f"{m:8s} generate() s " + " / ".join(f"{x:.4f}" for x in v) + f"    median {statistics.median(v):.4f}")
        if all(by.values()):
            spread = max(max(v) - min(v) for v in by.values())
            lines += ["", f"Arm-to-arm spread: one arm moved by up to {spread:.3f} ms/step between its rounds; that is the resolution of this comparison."]
            for x, y in (("off", "parent"), ("on", "off")):
                d = statistics.median(by[x]) - statistics.median(by[y])
                lines.append(f"  {x} against {y}: {d:+.3f} ms/step (medians): " + ("unresolved, inside the spread." if abs(d) <= spread else "outside the spread."))
            lines.append(f"  expected cost of the option: one launch of {fresh:.2f} us per step, {fresh * 1e-3 / statistics.median(by['off']) * 100:.2f} % of a step.")
        on = [a for a in arms if a["mode"] == "on"]
        if on:
            lines.append(f"  option on: graphs held by the decoder {on[-1]['graphs']}, rows that closed with <te> eos {on[-1]['rows_closed']} of "
                         f"{on[-1]['clips'] * on[-1]['K']}, mean raw mass of the allowed ids {on[-1]['mean_grammar_mass']}.")
        lines.append("")
    lines += ["# What this file does not say",
              "Whether the constraint changes accuracy.  The model here has seeded Gaussian weights: the raw mass of the allowed ids above is that of noise, and the",
              "ADE of constrained samples of such a model means nothing.  That needs a trained checkpoint (driver --constrain_traj reports grammar_mass_mean /",
              "grammar_mass_min next to ADE / FDE for that purpose); none was used here."]
    return lines


def report(a):
    k = _lines(a.kernel)[-1]
    arms = _lines(a.arms) if a.arms else []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(render(k, arms, a.note)) + "\n")
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:        # the raw lines beside the table
        f.write("\n".join(json.dumps(x) for x in [k] + arms) + "\n")
    print("\n".join(render(k, arms, a.note)))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("kernel")
    p = sub.add_parser("arm")
    p.add_argument("--mode", choices=("parent", "off", "on"), required=True)
    p.add_argument("--K", type=int, default=16)
    p.add_argument("--layers", type=int, default=None)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p = sub.add_parser("report")
    p.add_argument("--kernel", required=True)
    p.add_argument("--arms", default=None)
    p.add_argument("--note", default=None, help="one more header line about the arm runs, e.g. that they span two visits")
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "traj_grammar.txt"))
    a = ap.parse_args()
    {"kernel": kernel, "arm": lambda: arm(a), "report": lambda: report(a)}[a.cmd]()


if __name__ == "__main__":
    main()
