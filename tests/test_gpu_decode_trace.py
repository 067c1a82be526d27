"""GPU: decode.Decoder issues, in every mode, the library calls recorded in tests/golden/decode_launch_trace.json: the same symbols in the
same order with the same arguments (tests/decode_trace.py says how a launch is written down and at which shapes).  The file was recorded
with tools/debug/record_decode_trace.py on the commit before Decoder's cache layouts became objects, so equality here means that the
Python driving the kernels changed and nothing that reaches the device did.  Each case also asserts the fused / unfused state it is there
for, else it would be vacuous."""
import json
import os

import pytest
import torch

from tests import decode_trace as DT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    m = {}
    yield m
    m.clear()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "decode_launch_trace.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(DT.CASES)
    for name, case in DT.CASES.items():
        assert set(golden[name]) == {"prefill", "loop"} | ({"prefill_chunked"} if case[5] else set()), name


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(DT.CASES))
def test_launches_equal_the_recorded_trace(models, golden, name):
    got = json.loads(json.dumps(DT.run_case(models, name)))             # as the recorded file went through JSON: tuples are lists
    assert set(got) == set(golden[name])
    for phase in ("prefill", "prefill_chunked", "loop"):
        if phase in got:
            diff = DT.first_difference(got[phase], golden[name][phase])
            assert diff is None, f"{name} / {phase}: {diff}"


def test_tracing_leaves_the_call_binding_as_it_was(models):
    from egoscaler_amd import _lib, decode, ops
    DT.run_case(models, "fp32_tiny_greedy")
    assert ops.call is _lib.call and decode.call is _lib.call and not isinstance(_lib.call, DT.Recorder)


@pytest.mark.timeout(300)
def test_sample_graph_is_captured_once_and_greedy_keeps_none(models):
    from egoscaler_amd.decode import Decoder
    if "bf16" not in models:
        models["bf16"] = DT.make_model("bf16")
    m = models["bf16"]
    dec = Decoder(m.engine, DT.ROWS, DT.S0 + DT.T)
    assert all(dec.fused.values()), dec.fused
    ids = DT.prompt(DT.ROWS)
    outs = []
    for _ in range(2):
        dec.prefill(ids, None, None, None, DT.T)
        seq, sc = dec.sample(DT.T, eos=m.dims.tok.eos, pad=m.dims.tok.pad, seed=5, use_graph=True)
        torch.cuda.synchronize()
        outs.append((seq.clone(), sc.clone(), dec.graph))
    assert len(dec._graphs) == 1 and outs[0][2] is outs[1][2]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][1]).any())
    dec.prefill(ids, None, None, None, DT.T)
    seq, scores = dec.greedy(DT.T, use_graph=True)
    torch.cuda.synchronize()
    assert len(dec._graphs) == 1 and dec.graph is not outs[0][2]
    assert len(scores) == DT.T and all(s.dtype == torch.float32 and s.shape == dec.lg.shape for s in scores)
    assert scores[1].data_ptr() - scores[0].data_ptr() == scores[0].numel() * 4      # captured: views of one buffer
