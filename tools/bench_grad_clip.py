"""Timing of gradient-norm clipping (EgoAdamW(max_grad_norm=...), include/egomi.h egomi_grad_sumsq / egomi_clip_scale) on one MI355X.

  python tools/bench_grad_clip.py [--tables frozen,lora,unfrozen] [--reps 7] [--step-modes frozen,unfrozen] [--rounds 3]
                                  [--steps 10] [--warmup 3] [--parent-root DIR] [--bench-rounds 3] [--out profiles/grad_clip.txt]

1. The norm pass alone — grad_sumsq + clip_scale, three launches — over the gradient table of the three training set-ups at 7B
   (LLM frozen; plus LoRA r = 16 on all seven projections; LLM unfrozen, decoder-layer gradients in bf16 as the step holds them), and
   egomi_adamw / egomi_adamw_g16 over the same tensors in the same process: both stream, the norm pass 4 (2) of AdamW's 30 (28) bytes
   per parameter.  Device events around each repetition; median, bytes, us, TB/s.
2. The whole training step at the bench geometry (bs 8, bench.py's step) with clipping off and on (max_grad_norm = inf: same
   launches as a finite threshold), and — with --parent-root, a built checkout of the parent commit — the parent's step: one fresh
   process per arm and round, arms alternating round by round, median and (max - min) / median per arm.
3. With --parent-root: `python bench.py --gpus 1 --steps 20 --warmup 5 --no-extras --no-cpu-baseline` itself in the parent's tree and
   in this one, alternating, --bench-rounds times each.
The step of part 2 restates bench.py's (bench.py keeps it inside main() and has no option for the optimizer); part 3 is the check that
the restatement and the yardstick agree on parent against branch.
A path that finds no GPU fails; nothing here falls back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the tables
def table_shapes(kind):
    """[(numel, is_decoder_layer)] of the tensors EgoAdamW holds in the set-up `kind` at 7B (the rules of
    TrajPointLLMForCausalLM._configure_trainable_parameters: embedding, projector, final norm and lm_head always train)."""
    from egoscaler_amd import synth
    from egoscaler_amd.config import dims_7b
    dims = dims_7b()
    out = []
    for n, s in synth.param_shapes(dims):
        if n.startswith("model.point_backbone.") or len(s) == 0:
            continue
        layer = n.startswith("model.layers.")
        numel = 1
        for d in s:
            numel *= d
        if not layer or kind == "unfrozen":
            out.append((numel, layer))
    if kind == "lora":
        d, f, r = dims.lm.hidden_size, dims.lm.intermediate_size, 16
        for _ in range(dims.lm.num_hidden_layers):
            for i, o in [(d, d)] * 4 + [(d, f), (d, f), (f, d)]:
                out += [(r * i, False), (o * r, False)]
    return out


def run_tables(kinds, reps):
    import torch
    from egoscaler_amd import ops
    assert torch.cuda.is_available(), "bench_grad_clip needs a GPU"
    rows = []
    for kind in kinds:
        shapes = table_shapes(kind)
        grads = [torch.empty(n, dtype=torch.bfloat16 if layer else torch.float32, device="cuda").normal_(0, 1e-3) for n, layer in shapes]
        table = ops.GradTable(grads)
        out, stats = torch.zeros(3, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda")
        st = [(torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.bfloat16, device="cuda"), torch.zeros(n, device="cuda"),
               torch.zeros(n, device="cuda")) for n, _ in shapes]

        def norm_pass():
            ops.grad_sumsq(table)
            ops.clip_scale(table.total, 1.0, 1.0, out, stats)

        def adamw_pass():
            for g, (master, copy, m, v) in zip(grads, st):
                ops.adamw(master, copy, g, m, v, 2e-5, 0.9, 0.999, 1e-8, 0.01, 1, 1.0)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            return statistics.median(ts), min(ts), max(ts)
        n_el = sum(n for n, _ in shapes)
        g_bytes = sum(n * (2 if layer else 4) for n, layer in shapes)
        a_bytes = g_bytes + 26 * n_el                              # master, m, v read and written (24 B), the bf16 copy written (2 B)
        tn, ta = timed(norm_pass), timed(adamw_pass)
        rows.append({"table": kind, "segments": len(shapes), "chunks": table.n_chunks, "elements": n_el, "norm_bytes": g_bytes, "norm_us": tn,
                     "norm_TBps": g_bytes / tn[0] / 1e6, "adamw_bytes": a_bytes, "adamw_us": ta, "adamw_TBps": a_bytes / ta[0] / 1e6,
                     "norm_us_at_adamw_rate": g_bytes / (a_bytes / ta[0])})
        del grads, table, st
        torch.cuda.empty_cache()
    return rows


# ---------------------------------------------------------------------------------------------------------------- the step
def child_step(root, mode, clip, steps, warmup):
    """One process, one arm: bench.py's training step (bs 8, 7B bf16) from the tree `root`; prints one JSON line of per-step ms."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from egoscaler_amd import ops, synth
    from egoscaler_amd.config import dims_7b
    from egoscaler_amd.dp import GradSync
    from egoscaler_amd.optim import EgoAdamW
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    assert torch.cuda.is_available(), "bench_grad_clip needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dims = dims_7b()
    B, T, H, W = 8, 8, 224, 224
    margs = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=(mode == "unfrozen"), num_bins=256, model_name=None)
    model = TrajPointLLMForCausalLM(margs, dims, None, device=dev, dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for n, p in list(model.named_parameters()) + list(model.named_buffers()):
            leaf = n.rsplit(".", 1)[-1]
            if leaf == "num_batches_tracked":
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
    opt = EgoAdamW(model, lr=2e-5) if clip is None else EgoAdamW(model, lr=2e-5, max_grad_norm=clip)
    sync = GradSync(wire_dtype=torch.bfloat16, resident=True, local=True) if mode == "unfrozen" else None
    model.engine.grad_sync = sync
    torch.manual_seed(0)
    clips = [synth.synth_clip(i, T, H, W) for i in range(B)]
    rgb = torch.from_numpy(np.stack([c[0] for c in clips])).to(dev)
    depth = torch.from_numpy(np.stack([c[1] for c in clips])).to(dev)
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160, first_id=0)
    toks, masks = toks.to(dev), masks.to(dev)
    fx, pp = synth.clip_intrinsics(H)
    fps_start = torch.zeros(B, dtype=torch.int32, device=dev)
    overlap = model.engine.any_layer_trainable

    def step():
        pts, col, _ = ops.unproject_gather(rgb, depth, pp, fx, fx, synth.DEPTH_THRESHOLD, n_out=dims.pb.npoints)
        pc = ops.pc_norm(pts, col)
        if overlap and (sync is None or sync.local):
            opt.arm(grad_scale=1.0)
        loss = model.loss_and_backward(toks, masks, pc, Lp, dims.tok.pad, fps_start=fps_start)
        if sync is not None:
            sync.finish()
        opt.step(grad_scale=sync.grad_scale if sync is not None else 1.0, overlap=overlap)
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        loss = step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    rec = {"ms_per_step": sum(per) / steps, "median_ms": statistics.median(per), "loss": float(loss)}
    if clip is not None:
        rec["grad_norm"] = float(opt.last_grad_norm)
    print("RESULT " + json.dumps(rec), flush=True)


def run_steps(modes, rounds, steps, warmup, parent_root):
    arms = ([("parent", parent_root, "off")] if parent_root else []) + [("clip off", ROOT, "off"), ("clip on", ROOT, "inf")]
    res = {}
    for mode in modes:
        got = {a[0]: [] for a in arms}
        for _ in range(rounds):
            for name, root, clip in arms:                          # arms alternate round by round; a fresh process each
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, mode, clip, str(steps), str(warmup)],
                                   capture_output=True, text=True, cwd=root, timeout=400)   # (a child that hangs or faults ends the tool)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    raise SystemExit(f"arm '{name}' ({mode}) failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                got[name].append(json.loads(line[-1][7:]))
                print(f"[{mode}] {name}: {got[name][-1]['ms_per_step']:.3f} ms per step", file=sys.stderr, flush=True)
        res[mode] = got
    return res


def run_bench(parent_root, rounds):
    """bench.py's headline measurement, parent tree and this one alternating; -> {arm: [(clips/s, ms per step)]}."""
    got = {"parent": [], "branch": []}
    for _ in range(rounds):
        for name, root in (("parent", parent_root), ("branch", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-extras", "--no-cpu-baseline"],
                               capture_output=True, text=True, cwd=root, timeout=400)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise SystemExit(f"bench.py in the {name} tree failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            d = json.loads(line[-1])
            got[name].append((d["value"], d["ms_per_step"]))
            print(f"[bench.py] {name}: {d['value']:.3f} clips/s", file=sys.stderr, flush=True)
    return got


# ---------------------------------------------------------------------------------------------------------------- the report
def report(tables, steps, bench, a):
    argv = " ".join("<parent checkout>" if a.parent_root and x == a.parent_root else x for x in sys.argv[1:] if x != a.out and x != "--out")
    L = ["# Gradient-norm clipping on one MI355X: tools/bench_grad_clip.py " + argv]
    if tables is not None:
        L += ["", f"# The norm pass alone (grad_sumsq + clip_scale, 3 launches) and egomi_adamw over the same tensors, same process; {a.reps} repetitions "
                  "after one warm-up, device events around each; median (min .. max)",
              "table      segments  chunks    elements       norm bytes   norm us                    TB/s   adamw bytes   adamw us                   TB/s   norm us at adamw's rate"]
        for r in tables:
            L.append(f"{r['table']:<10} {r['segments']:>8}  {r['chunks']:>6}  {r['elements']:>13,}  {r['norm_bytes'] / 1e9:>8.3f} GB   "
                     f"{r['norm_us'][0]:>8.1f} ({r['norm_us'][1]:.1f} .. {r['norm_us'][2]:.1f})  {r['norm_TBps']:>5.2f}   {r['adamw_bytes'] / 1e9:>8.3f} GB   "
                     f"{r['adamw_us'][0]:>8.1f} ({r['adamw_us'][1]:.1f} .. {r['adamw_us'][2]:.1f})  {r['adamw_TBps']:>5.2f}   {r['norm_us_at_adamw_rate']:>8.1f}")
    else:
        L += ["", "# The norm pass alone: not measured"]
    if steps is not None:
        L += ["", f"# The whole step, bench geometry (7B bf16, bs 8), {a.warmup} warm-up + {a.steps} timed steps per process, one fresh process per arm and "
                  f"round, {a.rounds} rounds, arms alternating; ms per step"]
        for mode, got in steps.items():
            for name, recs in got.items():
                ms = [r["ms_per_step"] for r in recs]
                med = statistics.median(ms)
                L.append(f"{mode:<9} {name:<9} median {med:8.3f}   (max - min) / median {100 * (max(ms) - min(ms)) / med:5.2f} %   runs " +
                         " ".join(f"{x:.3f}" for x in ms) + (f"   grad_norm {recs[-1]['grad_norm']:.4g}" if "grad_norm" in recs[-1] else ""))
            if "parent" not in got:
                L.append(f"{mode:<9} parent    not measured (no --parent-root)")
    else:
        L += ["", "# The whole step: not measured"]
    if bench is not None:
        L += ["", f"# python bench.py --gpus 1 --steps 20 --warmup 5 --no-extras --no-cpu-baseline in the parent's tree and in this one, one fresh process "
                  f"each, alternating, {a.bench_rounds} rounds; clips/s (ms per step)"]
        for name, runs in bench.items():
            v = [x for x, _ in runs]
            med = statistics.median(v)
            L.append(f"{name:<7} median {med:7.3f} clips/s   (max - min) / median {100 * (max(v) - min(v)) / med:5.2f} %   runs " +
                     " ".join(f"{x:.3f} ({ms:.3f})" for x, ms in runs))
    else:
        L += ["", "# bench.py, parent against branch: not measured (no --parent-root)"]
    return "\n".join(L) + "\n"


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        root, mode, clip, steps, warmup = sys.argv[2:7]
        child_step(root, mode, None if clip == "off" else float(clip), int(steps), int(warmup))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="frozen,lora,unfrozen", help="comma list of frozen, lora, unfrozen; 'none' skips the kernel timings")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-modes", default="frozen,unfrozen", help="comma list of frozen, unfrozen; 'none' skips the step timings")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its step is timed as a third arm")
    ap.add_argument("--bench-rounds", type=int, default=3, help="with --parent-root: bench.py itself in both trees, this many times each (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    steps = None if a.step_modes == "none" else run_steps(a.step_modes.split(","), a.rounds, a.steps, a.warmup, a.parent_root)   # children first: this
    bench = run_bench(a.parent_root, a.bench_rounds) if a.parent_root and a.bench_rounds > 0 else None
    tables = None if a.tables == "none" else run_tables(a.tables.split(","), a.reps)                                            # process holds no GPU yet
    text = report(tables, steps, bench, a)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
