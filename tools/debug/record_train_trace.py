#!/usr/bin/env python3
"""Writes tests/golden/train_launch_trace.json: the launch trace of every case of tests/train_trace.py (what it records and why is said
there).  The file is the yardstick of tests/test_gpu_train_trace.py, so it is recorded ONCE, in a checkout of the commit an engine change
starts from (copy tests/launch_trace.py, tests/train_trace.py, tests/decode_trace.py and this script there), and never from the changed
tree.
GPU box only:  python tools/debug/record_train_trace.py [--out FILE]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import train_trace as TT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_launch_trace.json"))
    a = ap.parse_args()
    models, out, failed = {}, {}, []
    for name in TT.CASES:
        try:
            out[name] = TT.run_case(models, name)
        except AssertionError as e:                  # a case that did not take the path it is there for: name them all, write nothing
            failed.append(name)
            print(f"{name}: {type(e).__name__}: {str(e)[:2000]}", file=sys.stderr)
    if failed:
        sys.exit(f"not recorded: {failed}")
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print({name: {k: len(v) for k, v in t.items()} for name, t in out.items()}, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
