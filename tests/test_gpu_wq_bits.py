"""GPU: egomi_gemm_w8 and egomi_gemm_w4 give, bit for bit, the results recorded in tests/golden/wq_gemm_bits.json (tests/wq_bits.py says
from which inputs, at which shapes and in which three forms).  The file was recorded with tools/debug/record_wq_bits.py on the commit it
names, when each format had its own copy of everything, and is not re-recorded: a digest that differs means a change reordered or
re-rounded a sum somewhere between the loads and the store, which the float64 bounds of test_gpu_w8_kernels / test_gpu_w4_kernels allow."""
import json
import os

import pytest
import torch

from tests import wq_bits as WB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "wq_gemm_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ws():
    return torch.empty(WB.WS_BYTES, dtype=torch.uint8, device="cuda")


def test_every_case_is_recorded(golden):
    assert golden["commit"]
    assert set(golden["cases"]) == {WB.key(f, N, K, M) for f in WB.FORMATS for N, K in WB.SHAPES for M in WB.MS}


def test_inputs_are_what_the_fixture_was_recorded_from(golden):
    """The hash and the input rules, pinned on the host: a change to them would otherwise show as every digest differing."""
    got = {f: WB.sha(torch.cat([t.contiguous().view(torch.uint8).flatten() for t in WB.inputs(f, 68, 160, 3)])) for f in WB.FORMATS}
    assert got == golden["inputs_68_160_3"]
    x, res, codes, scales = WB.inputs("w8", 68, 160, 3)
    assert not bool(((codes & 0x7F) == 0x7F).any()) and float(x.abs().max()) <= 4 and float(res.abs().max()) <= 32
    assert float(scales.min()) >= 2.0 ** -10 and float(scales.max()) < 2.0 ** -9
    nib = WB.inputs("w4", 68, 160, 3)[2]
    assert int((nib & 15).min()) >= 1 and int((nib >> 4).min()) >= 1


@pytest.mark.parametrize("N,K", WB.SHAPES)
@pytest.mark.parametrize("fmt", WB.FORMATS)
def test_products_equal_the_recorded_bits(golden, ws, fmt, N, K):
    for M in WB.MS:
        got = WB.digests(fmt, N, K, M, ws)
        assert got == golden["cases"][WB.key(fmt, N, K, M)], WB.key(fmt, N, K, M)
        if (N, K) == (132, 2144):                                         # the case is there for the 4-way split: it must have happened
            assert got["slabs_n"] == 4
