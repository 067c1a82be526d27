"""GPU: the driver's --num_modes / --mode_radius on the tiny fp32 model (the arguments of tests/test_gpu_generate_logprobs.py's driver
tests): the record's six new keys, the dump's "modes", minADE_M recomputed from the dumped trajectories and indices, the flags left off
against --num_modes 0 and against the run with them (everything that existed stays what it is), and the rejected combinations."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 4
ARGV = ["eval", "--tiny", "--num_samples", str(K), "--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5", "--max_traj_token", "48"]
BASE_KEYS = {"ADE", "FDE", "ADE_as_called", "GD", "n", "minADE", "minFDE", "n_min", "K"}
MODE_KEYS = {"minADE_M", "minFDE_M", "brierADE_M", "n_modes", "M", "mode_radius"}


def _eval(tmp, capsys, extra):
    from egoscaler_amd import driver
    os.makedirs(tmp, exist_ok=True)
    torch.manual_seed(3)
    driver.main(ARGV + ["--out_dir", tmp] + extra)
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return rec, json.load(open(os.path.join(tmp, "test_gen_trajs.json")))


def _clip_ades(dump):
    """Per image id: the ADE of each of the K dumped trajectories against the split's ground truth (NaN for an unparsed one)."""
    from egoscaler_amd import driver, traj as TR
    from egoscaler_amd.config import dims_tiny
    a = driver.parse_args(ARGV)
    data = driver.make_data(a, dims_tiny(), None, a.split, TR.TargetNorm(a.do_norm, a.do_standard), a.n_val, 977)
    batch = data.batch(list(range(a.n_val)), torch.device("cuda"), a.max_traj_token)
    gt, ids = batch["trajectories"], batch["image_ids"].cpu().tolist()
    res = {}
    for b, i in enumerate(ids):
        ades = []
        for tr in dump[str(int(i))]:
            if tr is None:
                ades.append(float("nan"))
            else:
                g = torch.tensor(tr, dtype=torch.float32, device="cuda")[None]
                ades.append(float(TR.metrics_batch(g, None, gt[b:b + 1])[0][0]))
        res[str(int(i))] = ades
    return res


def _check_modes(rec, dump, M, radius):
    assert MODE_KEYS <= set(rec) and rec["M"] == M and rec["mode_radius"] == radius
    modes = dump.pop("modes")
    dump.pop("selected", None)
    assert len(dump) == 4 and set(modes) == set(dump)                  # exactly the dumped image ids
    ades, best, count = _clip_ades(dump), [], []
    for i, entry in modes.items():
        assert set(entry) == {"index", "conf"} and len(entry["index"]) == len(entry["conf"]) <= M
        idx, parsed = entry["index"], [j for j, a in enumerate(ades[i]) if not np.isnan(a)]
        assert all(0 <= j < K for j in idx) and len(set(idx)) == len(idx) and set(idx) <= set(parsed)
        assert (len(idx) >= 1) == bool(parsed)
        count.append(len(idx))
        if idx:
            assert abs(sum(entry["conf"]) - 1.0) < 1e-12 and all(c > 0 for c in entry["conf"])
            best.append(min(ades[i][j] for j in idx))
            assert min(ades[i][j] for j in parsed) <= best[-1]         # minADE_K <= minADE_M, clip by clip
    assert abs(rec["n_modes"] - float(np.mean(count))) < 1e-12
    if best:
        assert abs(rec["minADE_M"] - float(np.mean(best))) < 1e-9      # the record's mean is the mean of these
        assert rec["minADE"] <= rec["minADE_M"] + 1e-12 and rec["minADE_M"] <= rec["brierADE_M"] and rec["minFDE_M"] >= 0
    return modes


def test_driver_num_modes_adds_its_keys_and_nothing_else_moves(tmp_path, capsys):
    rec0, dump0 = _eval(str(tmp_path / "plain"), capsys, [])
    rec, dump = _eval(str(tmp_path / "modes"), capsys, ["--num_modes", "2", "--mode_radius", "0.0"])
    assert set(rec) == BASE_KEYS | MODE_KEYS
    _check_modes(rec, dict(dump), 2, 0.0)
    assert {k: v for k, v in dump.items() if k != "modes"} == dump0    # the same seeded samples, the same trajectories
    assert json.dumps({k: rec[k] for k in rec0}, sort_keys=True) == json.dumps(rec0, sort_keys=True)


def test_driver_num_modes_zero_is_the_run_without_the_flag(tmp_path, capsys):
    rec0, dump0 = _eval(str(tmp_path / "plain"), capsys, [])
    rec1, dump1 = _eval(str(tmp_path / "zero"), capsys, ["--num_modes", "0"])
    assert dump0 == dump1 and "modes" not in dump1 and "selected" not in dump1
    assert set(rec1) == BASE_KEYS
    assert json.dumps(rec0, sort_keys=True) == json.dumps(rec1, sort_keys=True)


def test_driver_num_modes_orders_by_the_logprob_scores(tmp_path, capsys):
    rec, dump = _eval(str(tmp_path / "lp"), capsys, ["--select", "logprob", "--num_modes", "3", "--mode_radius", "0.25"])
    assert MODE_KEYS | {"ADE_sel", "select"} <= set(rec)
    sel = dump["selected"]
    modes = _check_modes(rec, dict(dump), 3, 0.25)
    for i, entry in modes.items():                                     # the top-ranked sample, when it parsed, is the first mode
        if dump[i][sel[i]] is not None:
            assert entry["index"][0] == sel[i]


def test_driver_rejects_num_modes_without_samples_to_pick_from(tmp_path):
    from egoscaler_amd import driver
    tail = ["--dtype", "fp32", "--bs", "2", "--n_val", "2", "--num_steps", "5", "--max_traj_token", "48", "--out_dir", str(tmp_path / "bad")]
    for bad in (["--num_samples", "1", "--num_modes", "1"], ["--num_samples", "4", "--num_modes", "5"], ["--num_samples", "4", "--num_modes", "-1"],
                ["--num_samples", "4", "--mode_radius", "0.5"], ["--num_samples", "4", "--num_modes", "2", "--mode_radius", "-1"],
                ["--num_samples", "4", "--num_modes", "2", "--mode_radius", "nan"]):
        with pytest.raises(SystemExit):
            driver.main(["eval", "--tiny"] + bad + tail)
    model = types.SimpleNamespace(dims=None)                           # run_validation's own checks come before it touches the model
    for kw in (dict(num_samples=1, num_modes=1), dict(num_samples=4, num_modes=5), dict(num_samples=65, num_modes=2),
               dict(num_samples=4, num_modes=-1), dict(num_samples=4, num_modes=0, mode_radius=0.5),
               dict(num_samples=4, num_modes=2, mode_radius=-1.0), dict(num_samples=4, num_modes=2, mode_radius=float("nan"))):
        with pytest.raises(ValueError):
            driver.run_validation(model, None, driver.parse_args(["eval", "--tiny"]), "cuda", **kw)
