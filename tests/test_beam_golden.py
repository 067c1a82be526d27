"""CPU: tests/golden/beam_search.npz is what tools/gen_beam_golden.py records from HF's own beam search today (every key bit-equal),
and its cases keep decision margins that fp32 rounding on the device cannot cross."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_golden_regenerates_bit_equal(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_beam_golden
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    path = str(tmp_path / "beam_search.npz")
    gen_beam_golden.main(path)
    new = np.load(path, allow_pickle=False)
    old = np.load(os.path.join(golden_dir, "beam_search.npz"), allow_pickle=False)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k
    for c in old["cases"]:
        assert float(old[f"{c}/margin"]) > 1e-3, c
    it = {c: len(old[f"{c}/scores"]) for c in ("eos", "eos_es", "eos_never_lp2")}
    assert it["eos"] < int(old["t_new"])                               # hypotheses finish before max_length
    assert it["eos_es"] != it["eos"] and it["eos_never_lp2"] != it["eos"]     # early_stopping=True / "never" change the outcome
