#!/usr/bin/env python3
"""What generate(output_bin_stats=True) costs: the kernel alone, and a 7B decode step with it.
  kernel           egomi_bin_stats beside egomi_token_logprob (csrc/logprob.hip), one process, the same logits buffer: 128 rows x V = 32262
                   bf16, the window of the 7B tokenizer (p0 = 32006, nb = 256).  LAUNCHES launches captured into one hipGraph, microseconds
                   per launch = replay / LAUNCHES, best of REPS replays after a warm-up; ROUNDS rounds with the two arms alternated.  The
                   timed launch's mass is checked against a float64 softmax.  Prints one JSON line.
  arm --mode M     one generate() arm at 7B in the best-of-K shape of tools/bench_select.py: 8 clips x K = 16, a 540-token prompt, 64 new
                   tokens, share_prompt=True, do_sample with the reference's top_k / top_p.  parent: the call and nothing newer (this file
                   also runs from a checkout of the parent commit, whose package it then imports); off: the same call on this tree; on:
                   output_bin_stats=True.  ms per decode step = replay of the captured token loop / (steps - 1), best of 3 after a
                   warm-up.  Prints one JSON line; run the three arms alternated, one process each, at least five rounds.
  report           kernel line + arm lines (files of JSON lines) -> the table (default profiles/bin_stats.txt) and the lines beside it as
                   .json: medians over the rounds, and each arm's own spread next to every difference.  Needs no GPU.
GPU box:  python tools/bench_binstats.py kernel > k.json;  python tools/bench_binstats.py arm --mode on >> arms.jsonl;  ...
          python tools/bench_binstats.py report --kernel k.json --arms arms.jsonl"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAUNCHES, REPS, ROUNDS = 256, 5, 5
ROWS, V, NB = 128, 32262, 256
YARDSTICK_US = 9.15                                                    # egomi_token_logprob on the same bytes, profiles/select_of_k.txt


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
    from egoscaler_amd import decode, traj
    p0 = V - NB
    g = torch.Generator(device="cuda").manual_seed(3)
    lg = (3 * torch.randn(ROWS, V, device="cuda", generator=g)).to(torch.bfloat16)
    tok = torch.randint(0, V, (ROWS,), device="cuda", generator=g)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    lp_tok, lp_sum, lp_n = f32(ROWS, 1), f32(ROWS), torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    stats = [f32(ROWS, 1) for _ in range(4)]
    values = traj.bin_edges(NB, "cuda")
    fns = {"token_logprob": lambda: decode.token_logprob(lg, tok, None, None, lp_tok, 0, lp_sum, lp_n),
           "bin_stats": lambda: decode.bin_stats_rows(lg, p0, NB, values, *stats, 0)}
    out = {"rows": ROWS, "V": V, "nb": NB, "p0": p0, "dtype": "bf16", "bytes_read": ROWS * V * 2, "launches_per_graph": LAUNCHES, "reps": REPS,
           "clocks_before": clocks(), "us": {n: [] for n in fns}}
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            out["us"][n].append(round(graph_us(fn), 2))
    mass = torch.softmax(lg.double(), 1)[:, p0:].sum(1)                # what was timed computes what it should
    out["mass_err"] = float((stats[0][:, 0].double() - mass).abs().max())
    assert out["mass_err"] < 1e-6, out["mass_err"]
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
    kw = dict(input_ids=ids, attention_mask=mask, point_clouds=pcs, fps_start=st, max_length=T, num_return_sequences=K, eos_token_id=None, seed=5,
              share_prompt=True)
    if a.mode == "on":
        kw.update(output_bin_stats=True, bin_token_ids=(dims.tok.p0, dims.tok.num_bins))
    out = {"mode": a.mode, "prompt_len": Lp, "new_tokens": T, "clips": B, "K": K, "layers": dims.lm.num_hidden_layers, "clocks_before": clocks()}
    res = []
    ms_gen = timed(lambda: res.append(m.generate(**kw)))              # the first call captures the loop, the timed ones replay it
    dec = list(m._decoders.values())[-1]
    loop = timed(dec.graph.replay, 3)
    out.update({"ms_per_step": round(loop / max(1, T - 1), 4), "generate_s": round(ms_gen * 1e-3, 4), "graphs": len(dec._graphs)})
    if a.mode == "on":
        o = res[-1]
        out["finite"] = all(bool(torch.isfinite(t).all()) for t in (o.bin_mass, o.bin_mean, o.bin_std, o.bin_entropy))
        out["mean_bin_mass"], out["mean_bin_std"] = round(float(o.bin_mass.mean()), 5), round(float(o.bin_std.mean()), 4)
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.lstrip().startswith("{")]


def render(k, arms):
    """The lines of profiles/bin_stats.txt for one kernel line and the arm lines."""
    us = k["us"]
    med = {n: statistics.median(v) for n, v in us.items()}
    lines = [f"# egomi_bin_stats beside egomi_token_logprob: us per launch, {k['rows']} rows x V = {k['V']} {k['dtype']} (reads rows * V * 2 = "
             f"{k['bytes_read'] / 1e6:.2f} MB), window p0 = {k['p0']}, nb = {k['nb']}.",
             f"# tools/bench_binstats.py kernel; one MI355X, one process; {k['launches_per_graph']} launches captured into one hipGraph, replay / "
             f"{k['launches_per_graph']}, best of {k['reps']}; {len(us['bin_stats'])} rounds with the two arms alternated.",
             f"# sclk / mclk before: {'; '.join(k['clocks_before'])}; after: {'; '.join(k['clocks_after'])}.", ""]
    for n in ("token_logprob", "bin_stats"):
        lines.append(f"{'egomi_' + n:22s}" + " / ".join(f"{v:.2f}" for v in us[n]) + f"    median {med[n]:.2f} us, spread {max(us[n]) - min(us[n]):.2f} us")
    ratio = med["bin_stats"] / med["token_logprob"]
    lines += ["", f"egomi_bin_stats takes {ratio:.2f}x egomi_token_logprob's time on the same bytes ({med['bin_stats']:.2f} against {med['token_logprob']:.2f} us; that "
              f"kernel's recorded figure, profiles/select_of_k.txt: {YARDSTICK_US} us).  " +
              ("The expectation (the same order) holds." if ratio < 3 else "The expectation (the same order) is MISSED."),
              f"Worst |mass - float64 softmax mass| of the timed launch: {k['mass_err']:.1e}.", ""]
    if arms:
        a0 = arms[0]
        by = {m: [a["ms_per_step"] for a in arms if a["mode"] == m] for m in ("parent", "off", "on")}
        gen = {m: [a["generate_s"] for a in arms if a["mode"] == m] for m in by}
        lines += [f"# generate() at 7B bf16 ({a0['layers']} layers): {a0['clips']} clips x K = {a0['K']} ({a0['clips'] * a0['K']} rows), S0 = {a0['prompt_len']}, "
                  f"{a0['new_tokens']} new tokens, share_prompt=True, do_sample with the reference's top_k 50 / top_p 0.95.",
                  "# tools/bench_binstats.py arm; the parent commit's generate() (parent) against this tree with the option off (off) and on (on); one process per",
                  f"# run, the arms alternated in the order of the list below; ms per decode step = graph replay of all steps / {a0['new_tokens'] - 1}, best of 3.",
                  "# order: " + " ".join(a["mode"] for a in arms), ""]
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
            lines.append(f"  expected cost of the option: one launch of {med['bin_stats']:.2f} us per step, {med['bin_stats'] * 1e-3 / statistics.median(by['off']) * 100:.2f} % "
                         "of a step.")
        on = [a for a in arms if a["mode"] == "on"]
        if on:
            lines.append(f"  option on: graphs held by the decoder {on[-1]['graphs']}, every statistic finite: {on[-1]['finite']}, mean bin mass "
                         f"{on[-1]['mean_bin_mass']}, mean bin std {on[-1]['mean_bin_std']}.")
        lines.append("")
    lines += ["# What this file does not say",
              "Whether the soft decode helps accuracy.  The model here has seeded Gaussian weights: every step's distribution over the bins is noise (the mean",
              "bin mass and std above are those of noise), and ADE_soft against ADE of such a model means nothing.  That needs a trained checkpoint (driver",
              "--soft_decode reports ADE_soft / FDE_soft / sigma_mean / bin_mass_min next to ADE / FDE for that purpose); none was used here."]
    return lines


def report(a):
    k = _lines(a.kernel)[-1]
    arms = _lines(a.arms) if a.arms else []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(render(k, arms)) + "\n")
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:        # the raw lines beside the table
        f.write("\n".join(json.dumps(x) for x in [k] + arms) + "\n")
    print("\n".join(render(k, arms)))


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
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bin_stats.txt"))
    a = ap.parse_args()
    {"kernel": kernel, "arm": lambda: arm(a), "report": lambda: report(a)}[a.cmd]()


if __name__ == "__main__":
    main()
