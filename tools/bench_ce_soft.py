#!/usr/bin/env python3
"""What the bin-aware training loss (loss_and_backward(bin_soft=...), driver --bin_sigma) costs: the kernel alone, and the 7B frozen step.
  kernel   egomi_ce_soft_fwd_bwd beside egomi_ce_fwd_bwd (csrc/elementwise.hip), one process: 1280 rows x V = 32262 bf16, ld = 32320, in place
           (the training step's use: 8 clips x 160 target rows, the padded logits buffer), the 7B tokenizer's window (p0 = 32006, nb = 256),
           sigma 1, radius 3.  Each entry point's launches (the row kernel plus its one or two ordered sums) LAUNCHES times in one captured
           hipGraph, microseconds per call = replay / LAUNCHES, best of REPS replays after a warm-up; ROUNDS rounds with the two arms
           alternated.  One out-of-place call on the fresh logits is checked against a float64 soft cross-entropy.  Prints one JSON line.
  step     the 7B frozen training step at bs 8 (bench.py's geometry: loss_and_backward + EgoAdamW.step(overlap=True)), one model, one process,
           bin_soft off against on alternated round by round.  Prints one JSON line: ms per step of every round, medians, spread.
  report   kernel line + step line (files of JSON lines) -> the table (default profiles/ce_soft.txt).  Needs no GPU.
GPU box:  python tools/bench_ce_soft.py kernel > k.json;  python tools/bench_ce_soft.py step > s.json
          python tools/bench_ce_soft.py report --kernel k.json --step s.json"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAUNCHES, REPS, ROUNDS = 64, 5, 5
ROWS, V, LD, NB = 1280, 32262, 32320, 256
SIGMA, RADIUS = 1.0, 3


def kernel():
    import torch
    from bench_best_of_k import clocks, timed
    from egoscaler_amd._lib import call
    from egoscaler_amd.decode import _capture
    from egoscaler_amd.ops import S, dt
    p0 = V - NB
    g = torch.Generator(device="cuda").manual_seed(3)
    fresh = torch.zeros(ROWS, LD, dtype=torch.bfloat16, device="cuda")
    fresh[:, :V] = (3 * torch.randn(ROWS, V, device="cuda", generator=g)).to(torch.bfloat16)
    tg = torch.randint(p0, V, (ROWS,), device="cuda", generator=g)
    tg[::7] = p0 - 2                                                     # <tsep>-like rows: the one-hot path
    tg[5::160] = 0                                                       # ignored rows
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("egomi_ce_count", tg, ROWS, 0, cnt, S())
    sums, rows = torch.zeros(2, dtype=torch.float32, device="cuda"), torch.empty(2, ROWS, dtype=torch.float32, device="cuda")
    bufs = {"ce_fwd_bwd": fresh.clone(), "ce_soft_fwd_bwd": fresh.clone()}
    hard = lambda lg, dl: call("egomi_ce_fwd_bwd", lg, LD, tg, ROWS, V, 0, cnt, sums[0:1], rows[0], dl, LD, 1.0, dt(lg.dtype), S())
    soft = lambda lg, dl: call("egomi_ce_soft_fwd_bwd", lg, LD, tg, ROWS, V, 0, cnt, p0, NB, SIGMA, RADIUS, sums[0:1], sums[1:2], rows[0], rows[1], dl, LD,
                               1.0, dt(lg.dtype), S())
    fns = {"ce_fwd_bwd": lambda: hard(bufs["ce_fwd_bwd"][:, :V], bufs["ce_fwd_bwd"][:, :V]),
           "ce_soft_fwd_bwd": lambda: soft(bufs["ce_soft_fwd_bwd"][:, :V], bufs["ce_soft_fwd_bwd"][:, :V])}
    # what is timed computes what it should: one out-of-place call on the fresh logits against float64
    dl = torch.zeros(ROWS, LD, dtype=torch.bfloat16, device="cuda")[:, :V]   # the entry points below are given LD as the gradient's row stride too
    sums.zero_()
    soft(fresh[:, :V], dl)
    x = fresh[:, :V].double()
    lp = torch.log_softmax(x, 1)
    j = torch.arange(V, device="cuda")[None, :]
    w = torch.exp(-((j - tg[:, None]).double() ** 2) / (2 * SIGMA ** 2)) * ((j - tg[:, None]).abs() <= RADIUS) * (j >= p0)
    q = torch.where(((tg >= p0) & (tg != 0))[:, None], w / w.sum(1, keepdim=True).clamp_min(1e-300), torch.nn.functional.one_hot(tg, V).double())
    q = q * (tg != 0)[:, None]
    ref_loss = -(q * lp).sum()
    ref_grad = (torch.softmax(x, 1) * (tg != 0)[:, None] - q) / int(cnt)
    out = {"rows": ROWS, "V": V, "ld": LD, "nb": NB, "p0": p0, "sigma": SIGMA, "radius": RADIUS, "dtype": "bf16", "bytes_per_call": 2 * ROWS * V * 2,
           "launches_per_graph": LAUNCHES, "reps": REPS, "loss_rel_err": float((sums[0].double() - ref_loss).abs() / ref_loss),
           "grad_max_err_over_max": float((dl.double() - ref_grad).abs().max() / ref_grad.abs().max()), "pad_columns_zero": not bool(fresh[:, V:].any()),
           "clocks_before": clocks(), "us": {n: [] for n in fns}}
    assert out["loss_rel_err"] < 1e-5 and out["grad_max_err_over_max"] < 2 ** -8, out
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with _capture(gr):
                for _ in range(LAUNCHES):
                    fn()
            out["us"][n].append(round(timed(gr.replay, REPS) * 1e3 / LAUNCHES, 2))
    out["pad_columns_zero"] = out["pad_columns_zero"] and not any(bool(b[:, V:].any()) for b in bufs.values())
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def step(a):
    import torch
    from bench_best_of_k import clocks
    from bench_lora import build
    from egoscaler_amd import synth, traj
    from egoscaler_amd.config import dims_7b
    dev = torch.device("cuda", 0)
    dims = dims_7b()
    dims.lm.num_hidden_layers = a.layers
    B = a.batch
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    toks, masks = toks.to(dev), masks.to(dev)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).to(dev)
    start = torch.zeros(B, dtype=torch.long)
    m, opt = build(dims, None, 0, dev)
    spec = traj.soft_target_spec(dims.tok, SIGMA, RADIUS)
    kw = {"off": {}, "on": {"bin_soft": spec}}
    last = {}

    def one(k):
        last[k] = m.loss_and_backward(toks, masks, pts, Lp, dims.tok.pad, fps_start=start, **kw[k])
        opt.step(overlap=True)
    out = {"layers": a.layers, "batch": B, "seq": int(toks.shape[1]), "loss_rows": int(B * (toks.shape[1] - Lp)), "steps_per_round": a.steps, "sigma": SIGMA,
           "radius": RADIUS, "clocks_before": clocks(), "ms": {k: [] for k in kw}}
    for k in kw:
        for _ in range(a.warmup):
            one(k)
    for _ in range(a.rounds):
        for k in kw:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                one(k)
            torch.cuda.synchronize()
            out["ms"][k].append(round((time.perf_counter() - t0) * 1e3 / a.steps, 3))
    out["last_loss"] = {k: float(v) for k, v in last.items()}
    out["last_nll_on"] = float(m.last_nll)
    out["clocks_after"] = clocks()
    print(json.dumps(out))


def _lines(path):
    with open(path) as f:
        return [json.loads(l) for l in f if l.lstrip().startswith("{")]


def render(k, s):
    lines = []
    if k:
        us = k["us"]
        med = {n: statistics.median(v) for n, v in us.items()}
        lines += [f"# egomi_ce_soft_fwd_bwd beside egomi_ce_fwd_bwd: us per call (the row kernel and its ordered sums), {k['rows']} rows x V = {k['V']} {k['dtype']}, "
                  f"ld = {k['ld']}, in place (reads and writes rows * V * 2 bytes each: {k['bytes_per_call'] / 1e6:.1f} MB per call), window p0 = {k['p0']}, "
                  f"nb = {k['nb']}, sigma {k['sigma']}, radius {k['radius']}.",
                  f"# tools/bench_ce_soft.py kernel; one MI355X, one process; {k['launches_per_graph']} calls captured into one hipGraph, replay / "
                  f"{k['launches_per_graph']}, best of {k['reps']}; {len(us['ce_soft_fwd_bwd'])} rounds with the two arms alternated.",
                  f"# sclk / mclk before: {'; '.join(k['clocks_before'])}; after: {'; '.join(k['clocks_after'])}.", ""]
        for n in ("ce_fwd_bwd", "ce_soft_fwd_bwd"):
            lines.append(f"{'egomi_' + n:26s}" + " / ".join(f"{v:.2f}" for v in us[n]) + f"    median {med[n]:.2f} us, spread {max(us[n]) - min(us[n]):.2f} us")
        lines += ["", f"egomi_ce_soft_fwd_bwd takes {med['ce_soft_fwd_bwd'] / med['ce_fwd_bwd']:.2f}x egomi_ce_fwd_bwd's time on the same bytes "
                  f"({med['ce_soft_fwd_bwd']:.2f} against {med['ce_fwd_bwd']:.2f} us; {k['bytes_per_call'] / med['ce_soft_fwd_bwd'] * 1e-6:.2f} TB/s of row traffic).  No target ratio was set.",
                  f"The checked call (out of place, fresh logits): loss against float64 {k['loss_rel_err']:.1e} relative, worst gradient error "
                  f"{k['grad_max_err_over_max']:.1e} of the largest gradient (bf16 output); pad columns still zero after every launch: {k['pad_columns_zero']}.", ""]
    if s:
        ms = s["ms"]
        med = {n: statistics.median(v) for n, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        d = med["on"] - med["off"]
        lines += [f"# The 7B frozen training step, bf16, {s['layers']} layers, bs {s['batch']}, S = {s['seq']} ({s['loss_rows']} loss rows): loss_and_backward + "
                  "EgoAdamW.step(overlap=True), one model in one process,",
                  f"# bin_soft off against on (sigma {s['sigma']}, radius {s['radius']}) alternated round by round; ms per step = wall time of {s['steps_per_round']} steps / "
                  f"{s['steps_per_round']}; tools/bench_ce_soft.py step.",
                  f"# sclk / mclk before: {'; '.join(s['clocks_before'])}; after: {'; '.join(s['clocks_after'])}.", ""]
        for n in ("off", "on"):
            lines.append(f"{n:4s} ms per step  " + " / ".join(f"{x:.2f}" for x in ms[n]) + f"    median {med[n]:.2f}, spread {max(ms[n]) - min(ms[n]):.2f}")
        lines += ["", f"Arm-to-arm spread: one arm moved by up to {spread:.2f} ms/step between its rounds; that is the resolution of this comparison.",
                  f"  on against off: {d:+.2f} ms/step (medians, {d / med['off'] * 100:+.3f} %): " + ("unresolved, inside the spread." if abs(d) <= spread else "outside the spread."),
                  f"  last losses: off {s['last_loss']['off']:.4f} (hard), on {s['last_loss']['on']:.4f} (soft) with last_nll {s['last_nll_on']:.4f}.",
                  "  The off arm is the parent's step launch for launch (tests/test_gpu_train_trace.py); it is not timed against the parent.", ""]
    lines += ["# What this file does not say",
              "Whether the loss helps accuracy.  The model here has seeded Gaussian weights; the ADE or ADE_soft of a model trained this way on such weights",
              "means nothing.  Whether training with --bin_sigma improves ADE or ADE_soft on a real checkpoint is not measured."]
    return lines


def report(a):
    k = _lines(a.kernel)[-1] if a.kernel else None
    s = _lines(a.step)[-1] if a.step else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(render(k, s)) + "\n")
    print("\n".join(render(k, s)))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("kernel")
    p = sub.add_parser("step")
    p.add_argument("--layers", type=int, default=32)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=2)
    p = sub.add_parser("report")
    p.add_argument("--kernel", default=None)
    p.add_argument("--step", default=None)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ce_soft.txt"))
    a = ap.parse_args()
    {"kernel": kernel, "step": lambda: step(a), "report": lambda: report(a)}[a.cmd]()


if __name__ == "__main__":
    main()
