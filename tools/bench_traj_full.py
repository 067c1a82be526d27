#!/usr/bin/env python3
"""What egomi_traj_metrics_full (csrc/traj_full.hip) costs per launch beside egomi_traj_metrics_min (csrc/traj.hip), the kernel whose two
columns it repeats, in one process on the same inputs: B = 8 clips x K = 16 and 64 samples, Tmax = 20, D = 6, ragged lengths; and what the
host loop it replaces costs at the same shape: traj.anglar_distance (two scipy Rotation objects per step) once per sample.
Every device figure is LAUNCHES launches captured into one hipGraph, microseconds per launch = replay / LAUNCHES, best of REPS replays
after a warm-up; the arms are timed in ROUNDS rounds, alternated (tools/bench_modes.py's method).  The full kernel is also timed with every
n_gen = 1 (a DTW walk of n_gt = 20 steps per sample) and every n_gen = 20 (39 steps), which shows what a step of the walk costs.  The
timed calls are checked against each other first (columns 0, 1 and arg 0 of the minima are metrics_min's, bit for bit).
Prints one JSON line and writes the table to --out (default profiles/traj_full.txt) and that line beside it as .json.
GPU box only:  python tools/bench_traj_full.py [--out FILE]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench_best_of_k import clocks
from bench_modes import graph_us, LAUNCHES, REPS
from egoscaler_amd import traj
from egoscaler_amd._lib import call
from egoscaler_amd.ops import S

ROUNDS = 2
B, TMAX, D = 8, 20, 6
KS = (16, 64)
NAMES = ["metrics_min", "metrics_full", "metrics_full_no_minima", "metrics_full_one_step", "metrics_full_all_steps"]
WAVES = 8                                                             # wavefronts per clip in csrc/traj_full.hip: a wavefront runs K / 8 samples


def arms(k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gen = torch.randn(B, k, TMAX, D, device="cuda", generator=g)
    gt = torch.randn(B, TMAX, D, device="cuda", generator=g)
    ng = torch.randint(1, TMAX + 1, (B, k), device="cuda", generator=g).to(torch.int32)
    one, allt = torch.ones_like(ng), torch.full_like(ng, TMAX)
    made, mfde = (torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(2))
    best = torch.empty(B, dtype=torch.int32, device="cuda")
    out = torch.empty(B, k, 5, dtype=torch.float64, device="cuda")
    mins = torch.empty(B, 5, dtype=torch.float64, device="cuda")
    args = torch.empty(B, 5, dtype=torch.int32, device="cuda")
    full = lambda n, mn, ar: (lambda: call("egomi_traj_metrics_full", gen, n, gt, None, B, k, TMAX, D, 3, out, mn, ar, S()))
    m = traj.metrics_full(gen, ng, gt)
    a, f, bi = traj.metrics_best_of(gen, ng, gt)
    assert torch.equal(m.mins[:, 0], a) and torch.equal(m.mins[:, 1], f) and torch.equal(m.args[:, 0], bi)
    fns = {"metrics_min": lambda: call("egomi_traj_metrics_min", gen, ng, gt, None, B, k, TMAX, D, made, mfde, best, S()),
           "metrics_full": full(ng, mins, args), "metrics_full_no_minima": full(ng, None, None), "metrics_full_one_step": full(one, mins, args),
           "metrics_full_all_steps": full(allt, mins, args)}
    return fns, (gen.cpu().numpy().astype("float64"), ng.cpu().numpy(), gt.cpu().numpy().astype("float64"), m.gd.cpu().numpy())


def host_gd_ms(gen, ng, gt, dev_gd):
    """The loop the kernel replaces, for all B x K samples: traj.anglar_distance per sample.  Checked against the device's column."""
    traj.anglar_distance(gen[0, 0, :, 3:6], gt[0, :, 3:6])            # (scipy's import is not part of the loop)
    t0 = time.perf_counter()
    gd = [[traj.anglar_distance(gen[b, j, :ng[b, j], 3:6], gt[b, :, 3:6]) for j in range(gen.shape[1])] for b in range(gen.shape[0])]
    ms = (time.perf_counter() - t0) * 1e3
    assert abs(np.array(gd) - dev_gd).max() < 1e-6
    return ms


def render(out):
    """The lines of profiles/traj_full.txt for one run's JSON."""
    lines = [f"# egomi_traj_metrics_full beside egomi_traj_metrics_min: us per launch, B = {B}, Tmax = {TMAX}, D = {D}, ragged lengths 1 .. {TMAX}.",
             f"# tools/bench_traj_full.py; one MI355X, one process; {LAUNCHES} launches captured into one hipGraph, replay / {LAUNCHES}, best of {REPS};",
             f"# {ROUNDS} rounds with the arms alternated (first / second round).  sclk / mclk before: {'; '.join(out['clocks_before'])}; after: {'; '.join(out['clocks_after'])}.",
             f"# metrics_full_no_minima: mins = args = NULL.  metrics_full_one_step / _all_steps: every n_gen = 1 / = {TMAX}, a DTW walk of {TMAX} / {2 * TMAX - 1} steps.",
             "", f"{'':26s}" + "".join(f"{'K = ' + k[1:]:>22s}" for k in out["us"])]
    for n in NAMES:
        lines.append(f"{n:26s}" + "".join(f"{' / '.join(f'{v:.2f}' for v in out['us'][k][n]):>22s}" for k in out["us"]))
    lines.append(f"{'host GD loop (scipy), ms':26s}" + "".join(f"{out['host_gd_ms'][k]:>22.1f}" for k in out["us"]))
    lines.append("")
    for k, r in out["us"].items():
        full, mn, one, allt = (min(r[n]) for n in ("metrics_full", "metrics_min", "metrics_full_one_step", "metrics_full_all_steps"))
        per_step = (allt - one) * 1e3 / ((TMAX - 1) * -(-int(k[1:]) // WAVES))
        spread = max(max(v) - min(v) for v in r.values())
        lines.append(f"{k}: all five metrics of {B} x {k[1:]} samples take {full:.2f} us per launch against {mn:.2f} us for minADE / minFDE alone "
                     f"({full / mn:.1f}x) and {out['host_gd_ms'][k]:.1f} ms for the host GD loop alone ({out['host_gd_ms'][k] * 1e3 / full:.0f}x); "
                     f"{TMAX - 1} more steps of the DTW walk in each of a wavefront's {-(-int(k[1:]) // WAVES)} samples cost {allt - one:.2f} us, "
                     f"{per_step:.0f} ns per step; an arm moved by at most {spread:.2f} us between the rounds.")
    lines += ["", "# What bounds it",
              f"A sample is one wavefront's work and a clip one workgroup of {WAVES} wavefronts, so B = 8 clips keep 8 of the 256 CUs busy and a wavefront",
              f"runs K / {WAVES} samples one after the other.  Per sample the DTW walk is n_gen + n_gt - 1 dependent steps (a cross-lane pass of the strip's",
              "last row, D float64 multiply-adds and a square root on float32 rows read from L1 / LDS), and the index-order sums of ADE and GD are n_gt",
              f"dependent additions fed by cross-lane reads: a chain of latencies, not a rate.  The time therefore grows with K / {WAVES} and with the step",
              "count, not with the arithmetic; metrics_min runs one thread per clip over K x T steps and is bounded the same way.",
              "", "# What this file does not say",
              "How the exact DTW here relates to the reference's fastdtw(radius=1) on sequences of 3 or more steps: fastdtw is not installed, the",
              "relation (an upper bound of this value) is not measured.  The inputs are Gaussian noise: the metric values mean nothing."]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "traj_full.txt"))
    a = ap.parse_args()
    out = {"B": B, "Tmax": TMAX, "D": D, "launches_per_graph": LAUNCHES, "reps": REPS, "clocks_before": clocks(), "us": {}, "host_gd_ms": {}}
    for k in KS:
        fns, host = arms(k, 3 + k)
        res = {name: [] for name in fns}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                res[name].append(round(graph_us(fn), 2))
        out["us"][f"K{k}"] = res
        out["host_gd_ms"][f"K{k}"] = round(host_gd_ms(*host), 2)
    out["clocks_after"] = clocks()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(render(out)) + "\n")
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:        # the raw line beside the table
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
