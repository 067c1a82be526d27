#!/usr/bin/env python3
"""Writes tests/golden/validation_records.json: the (record, dump) pair of every case of tests/validation_golden.py (what a case is and
at which shapes is said there).  The file is the yardstick of tests/test_gpu_validation_golden.py, so it is recorded ONCE, in a checkout of
the commit a change to the validation pass starts from (copy tests/validation_golden.py and this script there), and never from the
changed tree.  Run it twice, in separate processes, and compare the files: they are expected to be byte-identical.
GPU box only:  python tools/debug/record_validation_golden.py [--out FILE]"""
import argparse, json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import validation_golden as VG


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "validation_records.json"))
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in VG.CASES:
            out[name] = VG.run_case(name, os.path.join(tmp, name))
            print(name, out[name][0] if isinstance(out[name], list) else out[name], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))


if __name__ == "__main__":
    main()
