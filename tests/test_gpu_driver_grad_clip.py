"""GPU: `driver train --max_grad_norm` end to end on the seeded synthetic data (tiny model): the epoch record and the step log gain the
gradient-norm keys with the flag and nothing without it, and a non-finite norm stops the run before the checkpoint is written."""
import math
import os

import pytest

pytestmark = pytest.mark.gpu

EXTRA = {"grad_norm_mean", "grad_norm_max", "clipped_steps", "nonfinite_steps"}


def _train(tmp, *flags):
    """driver.main(["train", "--tiny", "--epochs", "1", ...]) -> (epoch records, step-log entries)."""
    from egoscaler_amd import driver
    got, steps = [], []
    orig = driver.train

    def spy(args, model, train_data, val_data=None, device="cuda", log=print, step_log=None):
        got.extend(orig(args, model, train_data, val_data, device, log=lambda s: None, step_log=steps.append))
        return got
    driver.train = spy
    try:
        driver.main(["train", "--tiny", "--epochs", "1", "--n_train", "16", "--n_val", "4", "--bs", "4", "--out_dir", str(tmp), *flags])
    finally:
        driver.train = orig
    return got, steps


def test_epoch_record_and_step_log_gain_the_norm_keys_only_with_the_flag(tmp_path):
    on, steps_on = _train(tmp_path / "on", "--max_grad_norm", "0.5")
    off, steps_off = _train(tmp_path / "off")
    assert len(on) == len(off) == 1
    assert set(on[0]) - set(off[0]) == EXTRA and set(off[0]) - set(on[0]) == set()
    r = on[0]
    assert r["global_step"] == 4 and 0 <= r["clipped_steps"] <= r["global_step"] and r["nonfinite_steps"] == 0
    assert math.isfinite(r["grad_norm_max"]) and 0 < r["grad_norm_mean"] <= r["grad_norm_max"]
    norms = [s["grad_norm"] for s in steps_on]
    assert len(norms) == 4 and max(norms) == r["grad_norm_max"] and abs(sum(norms) / 4 - r["grad_norm_mean"]) <= 1e-12 * r["grad_norm_mean"]
    assert r["clipped_steps"] == sum(n + 1e-6 > 0.5 for n in norms)
    assert all("grad_norm" not in s for s in steps_off) and [set(s) - {"grad_norm"} for s in steps_on] == [set(s) for s in steps_off]
    assert os.path.exists(tmp_path / "on" / "latest_model.pt") and os.path.exists(tmp_path / "off" / "latest_model.pt")


def test_nonfinite_norm_stops_the_run_before_the_checkpoint(tmp_path, monkeypatch):
    """No batch is made non-finite (nothing here may fault the device): the epoch-end read is driven by a grad_stats that reports one
    non-finite step."""
    from egoscaler_amd.optim import EgoAdamW
    real = EgoAdamW.grad_stats

    def poisoned(self, reset=True):
        st = real(self, reset)
        st["nonfinite_steps"] = 1
        return st
    monkeypatch.setattr(EgoAdamW, "grad_stats", poisoned)
    with pytest.raises(FloatingPointError, match="epoch 0"):
        _train(tmp_path, "--max_grad_norm", "0.5")
    assert not os.path.exists(tmp_path / "latest_model.pt") and not os.path.exists(tmp_path / "best_model_ade.pt")
