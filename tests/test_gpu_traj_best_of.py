"""GPU: best-of-K trajectory metrics (traj.metrics_best_of -> egomi_traj_metrics_min) against oracle.traj.ade / fde looped over the K
samples (abs < 1e-12, as tests/test_gpu_traj.py::test_metrics_vs_oracle does for metrics_batch), and the driver's --num_samples."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _oracle_best(gen, ng, gt, nt):
    from oracle import traj as OT
    B, K = ng.shape
    ades = np.full((B, K), np.nan)
    fdes = np.full((B, K), np.nan)
    for b in range(B):
        for j in range(K):
            if ng[b, j] > 0:
                ades[b, j] = OT.ade(gen[b, j, :ng[b, j]].astype(np.float64), gt[b, :nt[b]].astype(np.float64))
                fdes[b, j] = OT.fde(gen[b, j, :ng[b, j]].astype(np.float64), gt[b, :nt[b]].astype(np.float64))
    return ades, fdes


def test_metrics_best_of_vs_oracle():
    from egoscaler_amd import traj as T
    g = np.random.default_rng(5)
    B, K, Tm = 5, 4, 20
    gen, gt = g.normal(size=(B, K, Tm, 6)).astype(np.float32), g.normal(size=(B, Tm, 6)).astype(np.float32)
    ng = np.array([[20, 15, 1, 20], [20, 20, 20, 20], [0, 7, 0, 20], [0, 0, 0, 0], [20, 20, 20, 20]], dtype=np.int32)   # ragged, unparsed, none left
    nt = np.array([20, 20, 12, 20, 20], dtype=np.int32)
    gen[4, 0] = gt[4] + 1e-3                                          # an exact tie between samples 0 and 2 of clip 4 that is also
    gen[4, 2] = gt[4] + 1e-3                                          # the best: the lower index wins
    d = lambda x: torch.from_numpy(x).cuda()
    made, mfde, best = T.metrics_best_of(d(gen), d(ng), d(gt), d(nt))
    assert made.dtype == mfde.dtype == torch.float64 and best.dtype == torch.int32
    made, mfde, best = made.cpu().numpy(), mfde.cpu().numpy(), best.cpu().numpy()
    ades, fdes = _oracle_best(gen, ng, gt, nt)
    for b in range(B):
        if not (ng[b] > 0).any():
            assert best[b] == -1 and np.isnan(made[b]) and np.isnan(mfde[b])
            continue
        assert abs(made[b] - np.nanmin(ades[b])) < 1e-12 and abs(mfde[b] - np.nanmin(fdes[b])) < 1e-12
        assert best[b] == int(np.nanargmin(ades[b])) and ng[b, best[b]] > 0
        for j in range(K):
            if ng[b, j] > 0:
                assert made[b] <= ades[b, j] + 1e-12
    assert best[4] == 0 and best[2] in (1, 3)
    # min FDE is the minimum over the samples, not the FDE of `best`
    b = 0
    assert abs(mfde[b] - fdes[b].min()) < 1e-12


def test_min_fde_is_not_the_fde_of_best():
    from egoscaler_amd import traj as T
    Tm = 6
    gt = np.zeros((1, Tm, 6), dtype=np.float32)
    gen = np.zeros((1, 2, Tm, 6), dtype=np.float32)
    gen[0, 0, :, 0] = 0.1                                             # sample 0: ADE 0.1, FDE 0.1
    gen[0, 1, :-1, 0] = 1.0                                           # sample 1: ADE 5/6, FDE 0
    made, mfde, best = T.metrics_best_of(torch.from_numpy(gen).cuda(), None, torch.from_numpy(gt).cuda())
    assert int(best[0]) == 0 and abs(float(made[0]) - float(np.float32(0.1))) < 1e-12 and float(mfde[0]) == 0.0


def test_k1_equals_metrics_batch():
    from egoscaler_amd import traj as T
    g = np.random.default_rng(2)
    B, Tm = 6, 20
    gen, gt = g.normal(size=(B, Tm, 6)).astype(np.float32), g.normal(size=(B, Tm, 6)).astype(np.float32)
    ng = torch.tensor([20, 15, 1, 20, 3, 9], dtype=torch.int32).cuda()
    nt = torch.tensor([20, 20, 20, 12, 20, 5], dtype=torch.int32).cuda()
    ade, fde = T.metrics_batch(torch.from_numpy(gen).cuda(), ng, torch.from_numpy(gt).cuda(), nt)
    made, mfde, best = T.metrics_best_of(torch.from_numpy(gen).cuda()[:, None], ng[:, None], torch.from_numpy(gt).cuda(), nt)
    assert torch.equal(made, ade) and torch.equal(mfde, fde) and bool((best == 0).all())
    with pytest.raises(ValueError):
        T.metrics_best_of(torch.from_numpy(gen).cuda(), None, torch.from_numpy(gt).cuda())


def _spy_generate(monkeypatch, seen):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    gen = TrajPointLLMForCausalLM.generate

    def spy(self, *a, **k):
        seen.append((k.get("num_return_sequences"), k.get("share_prompt")))
        return gen(self, *a, **k)
    monkeypatch.setattr(TrajPointLLMForCausalLM, "generate", spy)


def test_driver_eval_tiny_num_samples(tmp_path, monkeypatch, capsys):
    from egoscaler_amd import driver
    seen = []
    _spy_generate(monkeypatch, seen)
    torch.manual_seed(3)
    driver.main(["eval", "--tiny", "--num_samples", "4", "--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5",
                 "--max_traj_token", "48", "--out_dir", str(tmp_path)])
    assert seen and all(x == (4, True) for x in seen)
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["K"] == 4 and rec["n_min"] >= rec["n"] and rec["n_min"] <= 4
    assert {"ADE", "FDE", "ADE_as_called", "GD", "n", "minADE", "minFDE", "n_min", "K"} == set(rec)
    dump = json.load(open(os.path.join(str(tmp_path), "test_gen_trajs.json")))
    assert len(dump) == 4 and all(isinstance(v, list) and len(v) == 4 for v in dump.values())
    assert all(t is None or len(t[0]) == 6 for v in dump.values() for t in v)
    assert driver.parse_args(["eval", "--tiny"]).num_samples == 1


def test_driver_eval_tiny_num_samples_1_is_the_single_draw_record(tmp_path, monkeypatch, capsys):
    from egoscaler_amd import driver
    seen = []
    _spy_generate(monkeypatch, seen)
    driver.main(["eval", "--tiny", "--num_samples", "1", "--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5",
                 "--max_traj_token", "48", "--out_dir", str(tmp_path)])
    assert seen and all(x == (None, None) for x in seen)
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(rec) == {"ADE", "FDE", "ADE_as_called", "GD", "n"}


def test_driver_rejects_num_samples_with_greedy_or_beams(tmp_path):
    from egoscaler_amd import driver
    base = ["eval", "--tiny", "--num_samples", "4", "--dtype", "fp32", "--bs", "2", "--n_val", "2", "--num_steps", "5", "--max_traj_token", "48",
            "--out_dir", str(tmp_path)]
    for extra in (["--val_greedy"], ["--num_beams", "2"]):
        with pytest.raises(ValueError):
            driver.main(base + extra)
