#!/usr/bin/env python3
"""Writes tests/golden/wq_gemm_bits.json (the digests of every case of tests/wq_bits.py; GPU box) and tests/golden/wq_slab_counts.json
(the slab-count grid; host only, --counts-only skips the rest).  The files are the yardsticks of tests/test_gpu_wq_bits.py and
tests/test_wq_plan_host.py, so they are recorded ONCE, in a checkout of the commit a change to the products starts from (copy
tests/wq_bits.py and this script there), and never from the changed tree.
  python tools/debug/record_wq_bits.py --record --commit SHA [--counts-only] [--out DIR]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import wq_bits as WB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", required=True, help="the commit of the tree this runs in")
    ap.add_argument("--counts-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    from egoscaler_amd import _lib
    lib = _lib.lib()                                                      # the built library as it stands: this does not rebuild
    counts = {"commit": a.commit, **{f: WB.grid_counts(lib, f) for f in WB.FORMATS}}
    with open(os.path.join(a.out, "wq_slab_counts.json"), "w") as f:
        json.dump(counts, f, indent=0, sort_keys=True)
    print("slab counts:", {f: len(counts[f]) for f in WB.FORMATS})
    if a.counts_only:
        return
    import torch
    ws = torch.empty(WB.WS_BYTES, dtype=torch.uint8, device="cuda")
    bits = {"commit": a.commit,
            "inputs_68_160_3": {f: WB.sha(torch.cat([t.contiguous().view(torch.uint8).flatten() for t in WB.inputs(f, 68, 160, 3)])) for f in WB.FORMATS},
            "cases": {WB.key(f, N, K, M): WB.digests(f, N, K, M, ws) for f in WB.FORMATS for N, K in WB.SHAPES for M in WB.MS}}
    torch.cuda.synchronize()
    with open(os.path.join(a.out, "wq_gemm_bits.json"), "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
    print("cases:", len(bits["cases"]), "slab counts seen:", sorted({c["slabs_n"] for c in bits["cases"].values()}))


if __name__ == "__main__":
    main()
