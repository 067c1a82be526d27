#!/usr/bin/env python3
"""Writes tests/golden/decode_launch_trace.json: the launch trace of every case of tests/decode_trace.py (what it records and why is said
there).  The file is the yardstick of tests/test_gpu_decode_trace.py, so it is recorded ONCE, in a checkout of the commit a Decoder change
starts from (copy tests/decode_trace.py and this script there), and never from the changed tree.
GPU box only:  python tools/debug/record_decode_trace.py [--out FILE]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import decode_trace as DT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decode_launch_trace.json"))
    a = ap.parse_args()
    models = {}
    out = {name: DT.run_case(models, name) for name in DT.CASES}
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print({name: {k: len(v) for k, v in t.items()} for name, t in out.items()})


if __name__ == "__main__":
    main()
