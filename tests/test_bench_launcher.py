"""CPU: `python bench.py --gpus N` from a plain shell (no torchrun environment) spawns its own ranks, they rendezvous on
127.0.0.1 and see world_size N (the bench used to run one rank and print n_gpus 1)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(180)
@pytest.mark.parametrize("n", [2, 3])
def test_bench_spawns_its_own_ranks(n):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "gloo", "--dry-launch"],
                       capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                                     # rank 0 only
    assert json.loads(lines[0])["n_gpus"] == n


@pytest.mark.timeout(60)
def test_bench_rejects_world_size_mismatch():
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-launch"], capture_output=True, text=True, env=env, timeout=50)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


@pytest.mark.timeout(90)
def test_bench_fails_fast_when_one_rank_dies_at_startup():
    """one rank exiting non-zero must take the job down at once (the others are blocked in the rendezvous), not leave it
    to the driver's time limit.  Rank 1 exits with code 3 before init_process_group (EGOMI_BENCH_FAIL_RANK); the parent must return
    non-zero within seconds and leave no child behind."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(EGOMI_BENCH_FAIL_RANK="1", EGOMI_BENCH_RDV_TIMEOUT="600")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--backend", "gloo", "--dry-launch"],
                       capture_output=True, text=True, env=env, timeout=80)
    dt = time.time() - t0
    assert r.returncode != 0, (r.stdout, r.stderr[-500:])
    assert dt < 30, dt
    assert "rank 1 exited with code 3" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]                 # no result line from a broken job


def test_dump_outputs_within_budget_and_repeatable(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR` (bench.dump_outputs) on host tensors, with the budget shrunk to 1 MB: float64 loss, float32 gradients
    and masters (a bf16 gradient included), small tensors whole, large ones sampled at the same positions for a gradient and its master,
    the directory within the budget, and a second dump byte-identical to the first."""
    import types

    import numpy as np
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    shapes = {"small.weight": (64, 32), "big.weight": (512, 512), "wide.weight": (256, 1024)}
    state = {}
    for i, (n, shp) in enumerate(shapes.items()):
        master = torch.arange(shp[0] * shp[1], dtype=torch.float32).view(shp)          # value == flat index
        grad = (2 * master).to(torch.bfloat16 if i == 1 else torch.float32)             # big.weight: a bf16 gradient, as GradSync's wire buffers hold
        state[n] = {"p": types.SimpleNamespace(main_grad=grad, device=torch.device("cpu")), "master": master}
    model = types.SimpleNamespace(engine=types.SimpleNamespace(wait_param_updates=lambda: None))
    opt = types.SimpleNamespace(state=state)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, opt, torch.tensor(1.25))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(["loss.npy"] + [f"{k}.{n}.npy" for n in shapes for k in ("grad", "param")])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 20
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.dtype == np.float64 and float(loss) == 1.25
    small = np.load(tmp_path / "a" / "param.small.weight.npy")
    assert small.dtype == np.float32 and np.array_equal(small, state["small.weight"]["master"].numpy())
    for n in ("big.weight", "wide.weight"):
        p = np.load(tmp_path / "a" / f"param.{n}.npy")
        g = np.load(tmp_path / "a" / f"grad.{n}.npy")
        numel = shapes[n][0] * shapes[n][1]
        assert p.dtype == g.dtype == np.float32 and p.ndim == 1 and 1000 < p.size < numel
        assert np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < numel                 # sorted, unique flat indices of the tensor
        if n == "wide.weight":
            assert np.array_equal(g, 2 * p)                                           # the gradient sampled at the master's positions
        else:
            assert np.allclose(g, 2 * p, rtol=2 ** -7)                                # (bf16 gradient: values rounded to 8 bits)
