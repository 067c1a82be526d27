"""GPU: the driver's --traj_max_step / --traj_workspace on the tiny fp32 model with seeded weights, one process (the set-up of
tests/test_gpu_driver_grammar.py): `eval --tiny --constrain_traj --traj_max_step ...` writes n_limit_viol == 0 and limits_mass_min, every
clip still parses, and the rows the same pass generates WITHOUT the limits break them (counted with the same table, so the 0 is not
vacuous).  With the flags off the record's keys are those of --constrain_traj alone, and the record and the dump of a pass without them
are what they were before a pass with them.

The tiny model has 16 bins and runs without --do_norm, so one bin is 2 / 15 of a unit: --traj_max_step 0.3 is dmax = 2 bins
(2 * 2 / 15 = 0.267 <= 0.3 < 0.4), and the workspace -0.75 .. 0.75 in x holds the bins 2 .. 13."""
import numpy as np
import pytest
import torch

from tests.test_gpu_driver_grammar import TAIL

pytestmark = pytest.mark.gpu
STEP = "0.3,0.3,0.3,0.3,0.3,"
BOX = "--traj_workspace=-0.75,0.75,,,,"


def test_limits_flags_write_a_clean_record(monkeypatch):
    from egoscaler_amd import driver, synth, traj as TR
    from egoscaler_amd.config import dims_tiny
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dev = torch.device("cuda")
    base = ["eval", "--tiny"] + TAIL + ["--constrain_traj"]
    off_args = driver.parse_args(base)
    on_args = driver.parse_args(base + ["--traj_max_step", STEP, BOX])
    k_args = driver.parse_args(base + ["--traj_max_step", STEP, "--num_samples", "4"])
    dims = dims_tiny()
    tok = dims.tok
    model = TrajPointLLMForCausalLM(off_args, dims, None, device=dev, dtype=torch.float32)
    model.load_state_dict(synth.synth_state_dict(dims, 0))
    norm = TR.TargetNorm(off_args.do_norm, off_args.do_standard)
    data = driver.make_data(off_args, dims, None, off_args.split, norm, off_args.n_val, 977)
    lo, hi, step = driver.traj_limit_options(on_args, True)
    lim1 = TR.motion_limits(tok, norm, lo, hi, step).numpy()
    assert lim1[0].tolist() == [2, 0, 0, 0, 0, 0, 13, 15, 15, 15, 15, 15, 2, 2, 2, 2, 2, 15]
    seen, orig = [], driver.generate_batch

    def spy(*a, **kw):
        seen.append(orig(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(driver, "generate_batch", spy)

    def run(args):
        del seen[:]
        torch.manual_seed(3)
        rec, dump = driver.run_validation(model, data, args, dev)
        viol = sum(int(TR.limits_violations(b.out.sequences, tok, np.repeat(lim1, len(b.out.sequences), 0), start=b.prompts.shape[1]).sum()) for b in seen)
        return rec, dump, viol
    rec_off, dump_off, viol_off = run(off_args)
    rec_on, dump_on, viol_on = run(on_args)
    print(f"driver --traj_max_step {STEP} {BOX}: n_limit_viol {rec_on['n_limit_viol']}, limits_mass_min {rec_on['limits_mass_min']:.4g}, "
          f"grammar_mass_min {rec_on['grammar_mass_min']:.4g}; the same pass without the limits breaks them {viol_off} times")
    assert viol_off > 0, "the pass without the limits keeps them: the inputs show nothing"
    assert rec_on["n_limit_viol"] == 0 == viol_on and rec_on["n"] == off_args.n_val == len(dump_on)
    assert set(rec_on) - set(rec_off) == {"n_limit_viol", "limits_mass_min", "traj_workspace", "traj_max_step"} and set(rec_off) <= set(rec_on)
    assert rec_on["traj_max_step"] == STEP and rec_on["traj_workspace"] == BOX.split("=", 1)[1]
    assert 0.0 < rec_on["limits_mass_min"] <= rec_on["grammar_mass_min"] <= 1.0
    assert all(b.lim is not None and tuple(b.lim.shape) == (len(b.prompts), 18) for b in seen)
    rec_k, _, _ = run(k_args)                                            # K = 4 samples per clip on the shared prompt: every row is counted
    assert rec_k["n_limit_viol"] == 0 and rec_k["K"] == 4 and rec_k["traj_workspace"] is None
    assert sum(int(TR.limits_violations(b.out.sequences, tok, b.lim.repeat_interleave(4, 0), start=b.prompts.shape[1]).sum()) for b in seen) == 0
    rec_again, dump_again, _ = run(off_args)                             # the flags off after the limited passes: the record and the dump it had
    assert rec_again == rec_off and dump_again == dump_off and all(b.lim is None and b.out.limits_mass is None for b in seen)
    with pytest.raises(ValueError, match="constrain_traj"):
        driver.run_validation(model, data, driver.parse_args(base + ["--traj_max_step", STEP]), dev, constrain_traj=False)
