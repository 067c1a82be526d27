"""CPU: the split-K plan of the quantized decode-weight products (csrc/wq_gemm.h).  egomi_gemm_w8_slab_count and egomi_gemm_w4_slab_count
are host arithmetic (the library loads without a device): over the grid of tests/wq_bits.py they return the counts recorded in
tests/golden/wq_slab_counts.json on the commit it names, and the two formats agree on every entry, which decode.Decoder relies on."""
import ctypes
import json
import os

import pytest

from egoscaler_amd import build as B
from tests import wq_bits as WB


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "wq_slab_counts.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def counts():
    lib = ctypes.CDLL(B.build())
    return {f: WB.grid_counts(lib, f) for f in WB.FORMATS}


def test_grid_is_the_recorded_one(golden, counts):
    assert golden["commit"]
    n = len(WB.PLAN_MS) * len(WB.PLAN_SHAPES) * 5
    for f in WB.FORMATS:
        assert set(golden[f]) == set(counts[f]) and len(counts[f]) == n


@pytest.mark.parametrize("fmt", WB.FORMATS)
def test_slab_counts_equal_the_recorded_ones(golden, counts, fmt):
    bad = {k: (v, golden[fmt][k]) for k, v in counts[fmt].items() if v != golden[fmt][k]}
    assert not bad, bad


def test_both_formats_plan_identically(golden, counts):
    assert counts["w8"] == counts["w4"] and golden["w8"] == golden["w4"]


def test_grid_reaches_every_branch_of_the_plan(counts):
    c = counts["w8"]
    assert c["513/4096/4096/67108864"] == 0 and c["1/66/128/67108864"] == 0 and c["1/128/100/67108864"] == 0     # refused shapes
    assert c["8/4096/4096/0"] == 0 and c[f"8/4096/4096/{8 * 4096 * 4 - 1}"] == 0                                # not one slab fits
    assert c[f"8/4096/4096/{8 * 4096 * 4}"] == 1 and c[f"8/4096/4096/{3 * 8 * 4096 * 4 + 1}"] == 3                 # the workspace caps
    assert c["8/4096/4096/67108864"] == 8 and c["1/4/32/67108864"] == 1                                         # the block target; sk_max < 1
