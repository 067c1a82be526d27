#!/usr/bin/env python3
"""What egomi_traj_modes (csrc/modes.hip) costs per launch beside egomi_traj_medoid (csrc/traj.hip), the kernel whose pairwise distances it
shares, in one process on the same inputs: B = 8 clips x K = 16 and 32 samples, Tmax = 20, D = 6, ragged lengths (the shapes of
tools/bench_select.py's kernel timings), M = 6, radius 0.5, ordered by scores and by centrality, with and without the `dist` output.
Every figure is LAUNCHES launches captured into one hipGraph, microseconds per launch = replay / LAUNCHES, best of REPS replays after a
warm-up; the arms are timed in ROUNDS rounds, alternated, so that the spread of one arm between rounds is next to every difference.  The
outputs of the timed calls are checked against each other (with and without dist: the same modes; M = 1 by centrality: the medoid's pick).
Prints one JSON line and writes the table to --out (default profiles/select_modes.txt) and that line beside it as .json.
GPU box only:  python tools/bench_modes.py [--out FILE]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench_best_of_k import clocks, timed
from egoscaler_amd import traj
from egoscaler_amd._lib import call
from egoscaler_amd.ops import S

LAUNCHES, REPS, ROUNDS = 256, 5, 2
B, TMAX, D, M, RADIUS = 8, 20, 6, 6, 0.5


def graph_us(fn):
    from egoscaler_amd.decode import _capture
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        for _ in range(LAUNCHES):
            fn()
    return timed(g.replay, REPS) * 1e3 / LAUNCHES


def arms(k, gen_seed):
    g = torch.Generator(device="cuda").manual_seed(gen_seed)
    gen = torch.randn(B, k, TMAX, D, device="cuda", generator=g)
    ng = torch.randint(1, TMAX + 1, (B, k), device="cuda", generator=g).to(torch.int32)
    sc = torch.randn(B, k, device="cuda", generator=g)
    cost = torch.empty(B, k, dtype=torch.float64, device="cuda")
    pick = torch.empty(B, dtype=torch.int32, device="cuda")
    dist = torch.empty(B, k, k, dtype=torch.float64, device="cuda")
    modes = torch.empty(B, M, dtype=torch.int32, device="cuda")
    conf = torch.empty(B, M, dtype=torch.float64, device="cuda")
    assign = torch.empty(B, k, dtype=torch.int32, device="cuda")
    nm, nn = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    mo = lambda s, d: (lambda: call("egomi_traj_modes", gen, ng, s, B, k, TMAX, D, M, RADIUS, d, modes, conf, assign, nm, nn, S()))
    # what is timed computes what it should: the dist output changes nothing else, and M = 1 by centrality is the medoid
    a, b = traj.select_modes(gen, ng, sc, M, RADIUS), traj.select_modes(gen, ng, sc, M, RADIUS, return_dist=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(traj.select_modes(gen, ng, None, 1, RADIUS)[0][:, 0], traj.select_medoid(gen, ng)[0])
    return {"medoid": lambda: call("egomi_traj_medoid", gen, ng, B, k, TMAX, D, cost, pick, S()),
            "modes_scores": mo(sc, None), "modes_scores_dist": mo(sc, dist), "modes_central": mo(None, None), "modes_central_dist": mo(None, dist)}


def render(out):
    """The lines of profiles/select_modes.txt for one run's JSON."""
    names = ["medoid", "modes_scores", "modes_scores_dist", "modes_central", "modes_central_dist"]
    lines = [f"# egomi_traj_modes beside egomi_traj_medoid: us per launch, B = {B}, Tmax = {TMAX}, D = {D}, ragged lengths, M = {M}, radius {RADIUS}.",
             f"# tools/bench_modes.py; one MI355X, one process; {LAUNCHES} launches captured into one hipGraph, replay / {LAUNCHES}, best of {REPS};",
             f"# {ROUNDS} rounds with the arms alternated (first / second round).  sclk / mclk before: {'; '.join(out['clocks_before'])}; after: {'; '.join(out['clocks_after'])}.",
             "", f"{'':22s}" + "".join(f"{'K = ' + k[1:]:>22s}" for k in out["us"])]
    for n in names:
        lines.append(f"{n:22s}" + "".join(f"{' / '.join(f'{v:.2f}' for v in out['us'][k][n]):>22s}" for k in out["us"]))
    lines.append("")
    for k, r in out["us"].items():
        med, worst = min(r["medoid"]), max(max(r[n]) for n in names[1:])
        spread = max(max(v) - min(v) for v in r.values())
        lines.append(f"{k}: the slowest modes arm takes {worst:.2f} us against the medoid's {med:.2f} us ({med / worst:.1f}x); "
                     f"an arm moved by at most {spread:.2f} us between the rounds.  " +
                     ("The expectation (not slower than the medoid kernel) holds." if worst <= med else "The expectation (not slower than the medoid kernel) is MISSED."))
    lines += ["", "# What this file does not say",
              "The quality of the chosen set.  The inputs are Gaussian noise: which samples become modes, and minADE_M / brierADE_M of a model with seeded",
              "Gaussian weights, mean nothing.  Whether M modes come close to minADE_K has to be measured with trained weights (driver --num_samples K",
              "--num_modes M [--mode_radius R] reports minADE_M / minFDE_M / brierADE_M next to minADE for that purpose); no trained model was used here."]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "select_modes.txt"))
    a = ap.parse_args()
    out = {"B": B, "Tmax": TMAX, "D": D, "M": M, "radius": RADIUS, "launches_per_graph": LAUNCHES, "reps": REPS, "clocks_before": clocks(), "us": {}}
    for k in (16, 32):
        fns = arms(k, 3 + k)
        res = {name: [] for name in fns}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                res[name].append(round(graph_us(fn), 2))
        out["us"][f"K{k}"] = res
    out["clocks_after"] = clocks()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(render(out)) + "\n")
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:        # the raw line beside the table
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
