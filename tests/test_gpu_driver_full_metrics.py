"""GPU: the driver's --full_metrics on the tiny fp32 model (the arguments of tests/test_gpu_driver_modes.py): the record's new keys per
decoding mode, the dump's "full", its ADE column recomputed from the dumped trajectories, GD_dev beside the host-computed GD, and the flag
left off against the run with it (everything that existed stays what it is).  Four seeded runs, shared by the tests."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 4
TAIL = ["--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5", "--max_traj_token", "48"]
PICKS = ["--num_samples", str(K), "--select", "medoid", "--num_modes", "2"]
BASE_KEYS = {"ADE", "FDE", "ADE_as_called", "GD", "n"}
FULL_KEYS = {"IDE", "DTW", "GD_dev", "n_full"}
COLS = ("ADE", "FDE", "IDE", "GD", "DTW")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from egoscaler_amd import driver
    out = {}
    for name, extra in (("k1", []), ("k1_full", ["--full_metrics"]), ("k4", PICKS), ("k4_full", PICKS + ["--full_metrics"])):
        tmp = str(tmp_path_factory.mktemp(name))
        torch.manual_seed(3)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            driver.main(["eval", "--tiny"] + TAIL + ["--out_dir", tmp] + extra)
        out[name] = (json.loads(buf.getvalue().strip().splitlines()[-1]), json.load(open(os.path.join(tmp, "test_gen_trajs.json"))))
    return out


def _ground_truth():
    from egoscaler_amd import driver, traj as TR
    from egoscaler_amd.config import dims_tiny
    a = driver.parse_args(["eval", "--tiny"] + TAIL)
    data = driver.make_data(a, dims_tiny(), None, a.split, TR.TargetNorm(a.do_norm, a.do_standard), a.n_val, 977)
    batch = data.batch(list(range(a.n_val)), torch.device("cuda"), a.max_traj_token)
    return {str(int(i)): batch["trajectories"][b:b + 1] for b, i in enumerate(batch["image_ids"].cpu().tolist())}


def test_single_draw_gains_four_keys(runs):
    rec0, rec = runs["k1"][0], runs["k1_full"][0]
    assert set(rec0) == BASE_KEYS and set(rec) == BASE_KEYS | FULL_KEYS
    assert rec["n_full"] == rec["n"] and type(rec["n_full"]) is int
    if rec["n"]:
        assert abs(rec["GD_dev"] - rec["GD"]) < 2e-7 and rec["IDE"] >= 0 and rec["DTW"] >= 0


def test_samples_pick_and_modes_gain_exactly_their_keys(runs):
    rec0, rec = runs["k4"][0], runs["k4_full"][0]
    assert set(rec) - set(rec0) == FULL_KEYS | {"minIDE", "minGD", "minDTW", "GD_sel", "DTW_sel", "minGD_M", "minDTW_M"}
    assert set(rec0) <= set(rec) and rec["n_full"] == rec["n"]
    if rec["n"]:
        assert abs(rec["GD_dev"] - rec["GD"]) < 2e-7
    if rec["n_min"]:
        assert rec["minGD"] <= rec["minGD_M"] and rec["minDTW"] <= rec["minDTW_M"] and rec["minDTW"] <= rec["DTW_sel"]


@pytest.mark.parametrize("off,on", [("k1", "k1_full"), ("k4", "k4_full")])
def test_the_flag_moves_nothing_that_existed(runs, off, on):
    (rec0, dump0), (rec1, dump1) = runs[off], runs[on]
    assert json.dumps({k: rec1[k] for k in rec0}, sort_keys=True) == json.dumps(rec0, sort_keys=True)      # every bit of every old key
    assert "full" not in dump0 and {k: v for k, v in dump1.items() if k != "full"} == dump0


@pytest.mark.parametrize("name,k", [("k1_full", 1), ("k4_full", K)])
def test_the_dump_holds_every_sample_of_every_clip(runs, name, k):
    from egoscaler_amd import traj as TR
    rec, dump = runs[name]
    full, gts = dump["full"], _ground_truth()
    assert set(full) == set(gts)                                      # every image id of the split, parsed or not
    dtw0, dtw_min = [], []
    for i, entry in full.items():
        assert set(entry) == set(COLS) and all(len(entry[c]) == k for c in COLS)
        trajs = dump.get(i) if k > 1 else [dump.get(i)]
        for j in range(k):
            parsed = trajs is not None and trajs[j] is not None
            assert all((entry[c][j] is not None) == parsed for c in COLS)
            if parsed:
                g = torch.tensor(trajs[j], dtype=torch.float32, device="cuda")[None]
                ade, fde = TR.metrics_batch(g, None, gts[i])
                assert abs(entry["ADE"][j] - float(ade[0])) < 1e-12 and abs(entry["FDE"][j] - float(fde[0])) < 1e-12
                assert entry["DTW"][j] <= entry["ADE"][j] * g.shape[1] * (1 + 1e-12)         # the padded alignment is a warping path
        if entry["DTW"][0] is not None:
            dtw0.append(entry["DTW"][0])
            dtw_min.append(min(v for v in entry["DTW"] if v is not None))
    assert len(dtw0) == rec["n_full"]
    if dtw0:
        assert abs(rec["DTW"] - float(np.mean(dtw0))) < 1e-9
        assert all(m <= v for m, v in zip(dtw_min, dtw0))             # minDTW <= DTW on the clips whose sample 0 parsed
        if k > 1 and rec["n_min"] == rec["n"]:
            assert abs(rec["minDTW"] - float(np.mean(dtw_min))) < 1e-9 and rec["minDTW"] <= rec["DTW"]


def test_full_metrics_goes_with_greedy_and_beams(tmp_path):
    from egoscaler_amd import driver
    for extra in (["--val_greedy"], ["--num_beams", "2"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            driver.main(["eval", "--tiny", "--full_metrics"] + TAIL + ["--out_dir", str(tmp_path)] + extra)
        assert set(json.loads(buf.getvalue().strip().splitlines()[-1])) == BASE_KEYS | FULL_KEYS
