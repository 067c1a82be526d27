"""GPU: the training step and the prefill forward issue, in every mode, the library calls recorded in
tests/golden/train_launch_trace.json: the same symbols in the same order with the same arguments (tests/train_trace.py says how a launch
is written down, how buffers are named and at which shapes).  The file was recorded with tools/debug/record_train_trace.py on
egoscaler_amd/engine.py of commit 54cfb00 ("score(): teacher-forced log-probs of given trajectories, one pass"), the parent of the commit
that split Engine.forward_hidden / backward_hidden into stages, so equality here means that the Python driving the kernels changed and
nothing that reaches the device did.  Each case also asserts the decisions it is there for (train_trace.check_case), else it would be
vacuous."""
import json
import os

import pytest

from tests import train_trace as TT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    m = {}
    yield m
    m.clear()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "train_launch_trace.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(TT.CASES)
    for name, case in TT.CASES.items():
        assert set(golden[name]) == ({f"step{i}" for i in range(case[3])} or {"forward"}), name


@pytest.mark.parametrize("name", list(TT.CASES))
def test_launches_equal_the_recorded_trace(models, golden, name):
    got = json.loads(json.dumps(TT.run_case(models, name)))             # as the recorded file went through JSON: tuples are lists
    assert set(got) == set(golden[name])
    for phase in got:
        diff = TT.first_difference(got[phase], golden[name][phase])
        assert diff is None, f"{name} / {phase}: {diff}"


def test_tracing_leaves_the_call_binding_as_it_was(models):
    from egoscaler_amd import _lib, ops, pointbert_train
    from tests.launch_trace import Recorder
    TT.run_case(models, "tiny_fp32_frozen")
    assert ops.call is _lib.call and pointbert_train.call is _lib.call and not isinstance(_lib.call, Recorder)
    assert "backward_hidden" not in models["tiny"][0].engine.__dict__


def test_the_trace_sees_a_switched_off_tail_fusion(models, golden):
    got = json.loads(json.dumps(TT.run_case(models, "frozen_bf16", use_tail_fuse=False)))
    assert TT.first_difference(got["step0"], golden["frozen_bf16"]["step0"]) is not None
