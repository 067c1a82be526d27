#!/usr/bin/env python3
"""What generate(traj_limits=...) costs beside generate(traj_grammar=...): the kernel alone, and a 7B decode step with it.
  kernel           egomi_traj_grammar_step_limits beside egomi_traj_grammar_step (csrc/grammar.hip; one kernel body, one template flag), one
                   process, the shape of tools/bench_grammar.py: 128 rows x V = 32262 bf16, the 7B tokenizer's layout, every row at a step
                   boundary that allows the bins and <te>.  The limits form reads 30 more int32 per row (18 of the table, 12 of the pose, in
                   one batch beside the state) and nothing else.  Three limits arms: the full-range table (the same window: bit-equal
                   output, checked), dmax = 8 around the row's last bin (a 17-bin window), and a width-1 window.  LAUNCHES launches captured
                   into one hipGraph, microseconds per launch = replay / LAUNCHES, best of REPS after a warm-up, ROUNDS rounds with the arms
                   alternated, each on the rows it masked before.  Those arms pass no tok_prev, so the pose never moves in them; the walk
                   arms do what the loop does at steps t >= 1: a copy of the raw rows, then a launch whose tok_prev moves state and pose --
                   six bins (cur[p] stored each) and a <tsep> (cur copied to prev: 6 loads, 6 stores by thread 0), a 7-launch cycle that
                   repeats for ever -- with dmax = 8, beside the grammar step on the same walk and the copy alone (fresh logits: subtract it).
  arm --mode M     one generate() arm at 7B in the best-of-K shape of tools/bench_grammar.py: 8 clips x K = 16, a 540-token prompt, 64 new
                   tokens, share_prompt=True.  parent: traj_grammar alone on a checkout of the parent commit (this file runs from there and
                   imports that package); off: the same call on this tree; on: traj_limits = dmax 8 bins in every dimension.  ms per decode
                   step = replay of the captured token loop / (steps - 1), best of 3 after a warm-up.  One JSON line per run.
  report           kernel line + arm lines -> the table (default profiles/traj_limits.txt) and the raw lines beside it as .json; --mass: the
                   worst mass ratio tests/test_gpu_limits_kernel.py printed.  Needs no GPU."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 5
ROWS, V, NB = 128, 32262, 256


WALK_LAUNCHES = 252                                                       # 36 cycles of 7: every replay starts where the cycle starts


def walk_us(fn):
    """graph_us of tools/bench_grammar.py for a launch that walks a 7-launch cycle: one cycle eagerly, whole cycles in the graph."""
    import torch
    from bench_best_of_k import timed
    from bench_grammar import REPS
    from egoscaler_amd.decode import _capture
    for _ in range(7):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        for _ in range(WALK_LAUNCHES):
            fn()
    return timed(g.replay, REPS) * 1e3 / WALK_LAUNCHES


def kernel():
    import torch
    from bench_best_of_k import clocks
    from bench_grammar import LAUNCHES, REPS, graph_us
    from egoscaler_amd import decode
    spec = (V - NB, NB, V - NB - 3, V - NB - 2, V - NB - 1, 2, 1, 20)
    g = torch.Generator(device="cuda").manual_seed(3)
    raw = (3 * torch.randn(ROWS, V, device="cuda", generator=g)).to(torch.bfloat16)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    state = torch.tensor([[0, 3]] * ROWS, dtype=torch.int32, device="cuda")
    pose = torch.randint(0, NB, (ROWS, 12), device="cuda", generator=g).to(torch.int32)
    table = lambda lo, hi, d: torch.tensor([[lo] * 6 + [hi] * 6 + [d] * 6] * ROWS, dtype=torch.int32, device="cuda")
    tabs = {"limits_full_range": table(0, NB - 1, NB - 1), "limits_dmax8": table(0, NB - 1, 8), "limits_width1": table(0, NB - 1, 0)}
    bufs = {n: (raw.clone(), f32(ROWS, 1), f32(ROWS, 1)) for n in ("grammar",) + tuple(tabs)}
    fns = {"grammar": lambda: decode.traj_grammar_step(bufs["grammar"][0], None, state, spec, 50, bufs["grammar"][1], 0)}
    for n, t in tabs.items():
        fns[n] = lambda n=n, t=t: decode.traj_grammar_step_limits(bufs[n][0], None, state, spec, 50, bufs[n][1], 0, t, pose, bufs[n][2])
    a, b = bufs["grammar"], bufs["limits_full_range"]
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1]) and torch.equal(b[1], b[2])
    kept = {n: int(torch.isfinite(bufs[n][0][0]).sum()) for n in bufs}
    assert kept["limits_dmax8"] <= 17 + 1 and kept["limits_width1"] == 1 + 1, kept
    # the walk: every launch takes the token of the one before it, <tsep> at phase 6 and a bin elsewhere; steps has no ceiling here
    wspec = spec[:7] + (1 << 20,)
    toks = [torch.full((ROWS,), wspec[3], dtype=torch.int64, device="cuda")] + [torch.full((ROWS,), wspec[0] + 100 + 3 * p, dtype=torch.int64, device="cuda")
                                                                               for p in range(6)]          # index = the phase the token leads to
    walk = {n: {"lg": raw.clone(), "state": torch.tensor([[6, 0]] * ROWS, dtype=torch.int32, device="cuda"), "pose": pose.clone(), "i": 0,
                "mass": f32(ROWS, 1), "lmass": f32(ROWS, 1)} for n in ("copy_then_grammar_walk", "copy_then_limits_walk")}

    def walk_fn(n):
        w = walk[n]

        def fn():
            tok = toks[w["i"] % 7]
            w["i"] += 1
            w["lg"].copy_(raw)
            if n == "copy_then_grammar_walk":
                decode.traj_grammar_step(w["lg"], tok, w["state"], wspec, 50, w["mass"], 0)
            else:
                decode.traj_grammar_step_limits(w["lg"], tok, w["state"], wspec, 50, w["mass"], 0, tabs["limits_dmax8"], w["pose"], w["lmass"])
        return fn
    scratch = raw.clone()
    fns["row_copy"] = lambda: scratch.copy_(raw)
    for n in walk:
        fns[n] = walk_fn(n)
    for _ in range(14):                                                  # two cycles eagerly: the pose follows the tokens
        fns["copy_then_limits_walk"]()
    torch.cuda.synchronize()
    w = walk["copy_then_limits_walk"]
    assert w["state"].tolist() == [[6, 2]] * ROWS and w["pose"][0].tolist() == [100 + 3 * p for p in range(6)] * 2, (w["state"][0], w["pose"][0])
    out = {"rows": ROWS, "V": V, "nb": NB, "dtype": "bf16", "launches_per_graph": LAUNCHES, "walk_launches_per_graph": WALK_LAUNCHES, "reps": REPS,
           "finite_ids_row0": kept,
           "clocks_before": clocks(), "us": {n: [] for n in fns}}
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            out["us"][n].append(round(walk_us(fn) if n in walk else graph_us(fn), 2))
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def arm(a):
    import torch
    from bench_best_of_k import clocks, model_7b, timed
    from egoscaler_amd import synth, traj
    m, dims = model_7b(a.layers)
    B, T, K = a.batch, a.steps, a.K
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    kw = dict(input_ids=toks[:, :Lp].cuda(), attention_mask=masks[:, :Lp].cuda(), point_clouds=pcs, fps_start=torch.zeros(B, dtype=torch.int32, device="cuda"),
              max_length=T, num_return_sequences=K, eos_token_id=dims.tok.eos, seed=5, share_prompt=True, traj_grammar=traj.grammar_spec(dims.tok, 1, 20))
    if a.mode == "on":
        kw.update(traj_limits=traj.motion_limits_bins(dmax=8, nb=dims.tok.num_bins, rows=B))
    out = {"mode": a.mode, "prompt_len": Lp, "new_tokens": T, "clips": B, "K": K, "layers": dims.lm.num_hidden_layers, "clocks_before": clocks()}
    res = []
    ms_gen = timed(lambda: res.append(m.generate(**kw)))              # the first call captures the loop, the timed ones replay it
    dec = list(m._decoders.values())[-1]
    loop = timed(dec.graph.replay, 3)
    out.update({"ms_per_step": round(loop / max(1, T - 1), 4), "generate_s": round(ms_gen * 1e-3, 4), "graphs": len(dec._graphs)})
    if a.mode == "on":
        o = res[-1]
        live = o.grammar_mass > 0
        out["mean_limits_over_grammar_mass"] = round(float((o.limits_mass[live] / o.grammar_mass[live]).mean()), 5)
        out["n_limit_viol"] = int(traj.limits_violations(o.sequences, dims.tok, kw["traj_limits"].repeat_interleave(K, 0), start=Lp).sum())
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.lstrip().startswith("{")]


def render(k, arms, mass=None, note=None):
    us = k["us"]
    med = {n: statistics.median(v) for n, v in us.items()}
    spread = max(max(v) - min(v) for v in us.values())
    lines = [f"# egomi_traj_grammar_step_limits beside egomi_traj_grammar_step: us per launch, {k['rows']} rows x V = {k['V']} {k['dtype']}, nb = {k['nb']}, every row",
             "# allowing the bins and <te>, each arm in place on the rows it masked before.  tools/bench_limits.py kernel; one MI355X, one process;",
             f"# {k['launches_per_graph']} launches captured into one hipGraph, replay / {k['launches_per_graph']}, best of {k['reps']}; {len(us['grammar'])} rounds, the arms alternated.",
             f"# sclk / mclk before: {'; '.join(k['clocks_before'])}; after: {'; '.join(k['clocks_after'])}.",
             f"# finite ids left in row 0: {k['finite_ids_row0']}; the full-range arm's logits and mass are bit-equal to the grammar step's, limits_mass to mass.", ""]
    for n, v in us.items():
        lines.append(f"{n:26s}" + " / ".join(f"{x:.2f}" for x in v) + f"    median {med[n]:.2f} us, spread {max(v) - min(v):.2f} us")
    lines += ["", f"Arm-to-arm spread: one arm moved by up to {spread:.2f} us between its rounds; that is the resolution of this comparison."]
    verdict = lambda d: "unresolved, inside the spread." if abs(d) <= spread else "outside the spread."
    for n in us:
        if n.startswith("limits_"):
            lines.append(f"  {n} against grammar: {med[n] - med['grammar']:+.2f} us (medians): " + verdict(med[n] - med["grammar"]))
    gw = lw = 0.0
    if "copy_then_limits_walk" in us:
        gw, lw = med["copy_then_grammar_walk"] - med["row_copy"], med["copy_then_limits_walk"] - med["row_copy"]
        lines += [f"  the walk (tok_prev moves state and pose in every launch: six bins, then <tsep>; fresh logits = copy_then_* - row_copy; "
                  f"{k['walk_launches_per_graph']} launches per graph):",
                  f"    grammar step {gw:.2f} us, limits step {lw:.2f} us: {lw - gw:+.2f} us (medians): " + verdict(lw - gw)]
    lines += ["  Why the limits form is slower where the window is the same (full range): what its compiled code adds, per workgroup of 1024 threads, is",
              "  the second live slot of the float64 block sum -- the grammar step's slot is a constant 0 and the compiler drops it: 12 more ds_bpermute",
              "  (6 rounds x 2 halves of a double), 23 more v_add_f64, 8 more LDS reads per thread between the same barriers --, one more division and",
              "  store by thread 0, and 30 int32 of table and pose loaded beside the state (one batch of scalar loads, one wait; DESIGN.md has what",
              "  loading them entry by entry behind the phase cost).  Which of these carries how much of the difference has NOT been measured.", ""]
    if mass:
        lines += [f"mass / limits_mass against float64, worst |got - ref| / (1 + |ref|) over every case of tests/test_gpu_limits_kernel.py: {mass}", ""]
    if arms:
        a0 = arms[0]
        by = {m: [a["ms_per_step"] for a in arms if a["mode"] == m] for m in ("parent", "off", "on")}
        lines += [f"# generate(traj_grammar=...) at 7B bf16 ({a0['layers']} layers): {a0['clips']} clips x K = {a0['K']}, S0 = {a0['prompt_len']}, {a0['new_tokens']} new tokens,",
                  "# share_prompt=True.  parent = the parent commit; off = this tree without traj_limits; on = traj_limits dmax 8 bins.  One process per run,",
                  f"# ms per decode step = graph replay of all steps / {a0['new_tokens'] - 1}, best of 3.  order: " + " ".join(a["mode"] for a in arms)]
        lines += ([f"# {note}"] if note else []) + [""]
        for m, v in by.items():
            if v:
                lines.append(f"{m:8s} ms per step  " + " / ".join(f"{x:.3f}" for x in v) + f"    median {statistics.median(v):.3f}, spread {max(v) - min(v):.3f}")
        got = {m: v for m, v in by.items() if v}
        if len(got) > 1:
            sp = max(max(v) - min(v) for v in got.values())
            lines += ["", f"Arm-to-arm spread: one arm moved by up to {sp:.3f} ms/step between its rounds; that is the resolution of this comparison."]
            for x, y in (("off", "parent"), ("on", "off")):
                if x in got and y in got:
                    d = statistics.median(got[x]) - statistics.median(got[y])
                    lines.append(f"  {x} against {y}: {d:+.3f} ms/step (medians): " + ("unresolved, inside the spread." if abs(d) <= sp else "outside the spread."))
            if "off" in got and "copy_then_limits_walk" in us:
                lines.append(f"  expected from the kernel figures: {lw - gw:+.2f} us per step, {(lw - gw) * 1e-3 / statistics.median(got['off']) * 100:.3f} % of a step.")
        on = [a for a in arms if a["mode"] == "on"]
        if on:
            lines.append(f"  option on: n_limit_viol {on[-1]['n_limit_viol']}, mean limits_mass / grammar_mass {on[-1]['mean_limits_over_grammar_mass']}, graphs {on[-1]['graphs']}.")
        lines.append("")
    lines += ["# What this file does not say",
              "Whether the limits change accuracy.  The model here has seeded Gaussian weights: limits_mass / grammar_mass above is that of noise, and the ADE of",
              "limited samples of such a model means nothing.  That needs a trained checkpoint (driver --traj_max_step / --traj_workspace report n_limit_viol and",
              "limits_mass_min next to ADE / FDE for that purpose); none was used here."]
    return lines


def report(a):
    k = _lines(a.kernel)[-1]
    arms = _lines(a.arms) if a.arms else []
    text = "\n".join(render(k, arms, a.mass, a.note)) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
        f.write("\n".join(json.dumps(x) for x in [k] + arms) + "\n")
    print(text, end="")


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
    p.add_argument("--mass", default=None, help="the worst mass ratio the kernel tests printed")
    p.add_argument("--note", default=None)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "traj_limits.txt"))
    a = ap.parse_args()
    {"kernel": kernel, "arm": lambda: arm(a), "report": lambda: report(a)}[a.cmd]()


if __name__ == "__main__":
    main()
