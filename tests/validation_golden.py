"""The validation pass of driver.main as data: one tiny eval per argument set, (record, dump) each.

tests/golden/validation_records.json holds the pair of every case in CASES as recorded by tools/debug/record_validation_golden.py on the
commit before run_validation was split into parts; tests/test_gpu_validation_golden.py replays the cases against it.  Two recordings of
that commit in separate processes were byte-identical, so the comparison is exact: the same keys, the same values (NaN equals NaN).

Shapes: the tiny model, 5 clips in batches of 2 (the short last batch is exercised), 5 steps, 48 trajectory tokens."""
import contextlib
import io
import json
import os

import torch

BASE = ["eval", "--tiny", "--bs", "2", "--n_val", "5", "--num_steps", "5", "--max_traj_token", "48"]
FP32, BF16 = ["--dtype", "fp32"], ["--dtype", "bf16"]
CASES = {
    "sample": FP32,
    "greedy": FP32 + ["--val_greedy"],
    "beam2_greedy": FP32 + ["--num_beams", "2", "--val_greedy"],
    "beam2_split": FP32 + ["--num_beams", "2", "--kv_cache_layout", "split"],
    "k4": FP32 + ["--num_samples", "4"],
    "k4_medoid": FP32 + ["--num_samples", "4", "--select", "medoid"],
    "k4_logprob_rescore_modes2": FP32 + ["--num_samples", "4", "--select", "logprob", "--rescore", "--num_modes", "2", "--mode_radius", "0.05"],
    "k4_modes3_soft": FP32 + ["--num_samples", "4", "--num_modes", "3", "--soft_decode"],
    "greedy_soft": FP32 + ["--val_greedy", "--soft_decode"],
    "k4_kv8_logprob_bf16": BF16 + ["--num_samples", "4", "--kv_cache_dtype", "fp8", "--select", "logprob"],
}


def run_case(name, tmp):
    """driver.main on case `name`, in-process, writing under directory tmp -> [record, dump] as JSON gives them back.  A case that the
    driver refuses is recorded as what it raises, {"raises": type name, "message": text}: generate() has no shared-prompt decoder on an
    fp8 KV cache, so the last case is pinned as that NotImplementedError."""
    from egoscaler_amd import driver
    os.makedirs(tmp, exist_ok=True)
    buf = io.StringIO()
    torch.manual_seed(3)
    try:
        with contextlib.redirect_stdout(buf):
            driver.main(BASE + CASES[name] + ["--out_dir", tmp])
    except Exception as e:                                                # noqa: BLE001  (the refusal is the case's outcome)
        return {"raises": type(e).__name__, "message": str(e)}
    rec = json.loads(buf.getvalue().strip().splitlines()[-1])
    with open(os.path.join(tmp, "test_gen_trajs.json")) as f:
        return [rec, json.load(f)]


def canonical(outcome):
    """The text two equal outcomes of run_case share: sorted keys; NaN is written as NaN, so NaN compares equal to NaN."""
    return json.dumps(outcome, sort_keys=True)
