"""GPU: the driver's --constrain_traj on the tiny fp32 model with seeded weights, one process: with the flag every validation clip is a
well-formed trajectory of exactly --num_steps steps and the record's parsed count `n` equals the number of clips; the same run without
the flag, on the same weights and seed, parses fewer.

"Parses" is the strict reading of tests/grammar_ref.py (<ts> (bin{6} <tsep>){n} <te> eos, n = num_steps, the prompt's step included),
counted on the rows generate_batch returned.  The record's own `n` cannot tell the two runs apart: it counts the rows with at least one
step after traj_scan's copy-forward, and the prompt's last seven tokens -- its first step and <tsep> -- go through the scan with every
row, so n equals the number of clips whatever was generated (tests/test_gpu_driver.py pins n == 4 of 4 on these seeded weights without
the flag).  n == clips is asserted with the flag; "fewer without it" is asserted on the strict count.
Measured on the MI355X: with the flag n 4, strict 4 of 4; without it n 4, strict 0 of 4; grammar_mass_mean 0.0382, grammar_mass_min 9.4e-4."""
import pytest
import torch

from tests import grammar_ref as G

pytestmark = pytest.mark.gpu
TAIL = ["--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5", "--max_traj_token", "48"]


def test_constrain_traj_makes_every_clip_parse(monkeypatch):
    from egoscaler_amd import driver, synth, traj as TR
    from egoscaler_amd.config import dims_tiny
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dev = torch.device("cuda")
    off_args = driver.parse_args(["eval", "--tiny"] + TAIL)
    on_args = driver.parse_args(["eval", "--tiny"] + TAIL + ["--constrain_traj"])
    assert on_args.constrain_traj and not off_args.constrain_traj
    dims = dims_tiny()
    model = TrajPointLLMForCausalLM(off_args, dims, None, device=dev, dtype=torch.float32)
    model.load_state_dict(synth.synth_state_dict(dims, 0))
    data = driver.make_data(off_args, dims, None, off_args.split, TR.TargetNorm(off_args.do_norm, off_args.do_standard), off_args.n_val, 977)
    spec = TR.grammar_spec(dims.tok, off_args.num_steps, off_args.num_steps)
    seen, orig = [], driver.generate_batch

    def spy(*a, **kw):
        seen.append(orig(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(driver, "generate_batch", spy)

    def run(args):
        del seen[:]
        torch.manual_seed(3)
        rec, dump = driver.run_validation(model, data, args, dev)
        strict = sum(bool(G.valid(spec, G.prompt_tail(spec, p), g, pad=dims.tok.pad))
                     for b in seen for p, g in zip(b.prompts.cpu().numpy(), b.all_ids.cpu().numpy()))
        return rec, dump, strict
    rec_off, dump_off, strict_off = run(off_args)
    rec_on, dump_on, strict_on = run(on_args)
    print(f"driver --constrain_traj: n {rec_on['n']} / strict {strict_on} of {off_args.n_val} with the flag, n {rec_off['n']} / strict {strict_off} "
          f"without; grammar_mass_mean {rec_on['grammar_mass_mean']:.4g} grammar_mass_min {rec_on['grammar_mass_min']:.4g}")
    assert rec_on["n"] == off_args.n_val == strict_on == len(dump_on)
    assert strict_off < off_args.n_val
    assert set(rec_on) - set(rec_off) == {"grammar_mass_mean", "grammar_mass_min"} and set(rec_off) <= set(rec_on)
    assert 0.0 < rec_on["grammar_mass_min"] <= rec_on["grammar_mass_mean"] <= 1.0
    with pytest.raises(ValueError, match="constrain_traj"):
        driver.run_validation(model, data, on_args, dev, num_beams=2)
    rec_again, dump_again, _ = run(off_args)                             # the flag off after a constrained pass: the record and the dump it had
    assert rec_again == rec_off and dump_again == dump_off
