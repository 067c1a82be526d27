"""GPU: the validation pass gives, for every argument set of tests/validation_golden.py, the (record, dump) pair recorded in
tests/golden/validation_records.json.  The file was recorded with tools/debug/record_validation_golden.py on the commit before
run_validation was split into parts; two recordings of that commit in separate processes were byte-identical, so every key, count, index
and float is compared exactly (NaN equal to NaN).  A case the driver refuses is pinned as the exception it raises."""
import json
import os

import pytest

from tests import validation_golden as VG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "validation_records.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert set(golden) == set(VG.CASES)


def _first_difference(got, want, path=""):
    if isinstance(want, dict) and isinstance(got, dict):
        if set(got) != set(want):
            return f"{path}: keys differ: missing {sorted(set(want) - set(got))[:4]}, unexpected {sorted(set(got) - set(want))[:4]}"
        return next((d for k in want for d in [_first_difference(got[k], want[k], f"{path}/{k}")] if d), None)
    if isinstance(want, list) and isinstance(got, list) and len(got) == len(want):
        return next((d for i in range(len(want)) for d in [_first_difference(got[i], want[i], f"{path}[{i}]")] if d), None)
    return None if VG.canonical(got) == VG.canonical(want) else f"{path}: {got!r} != {want!r}"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(VG.CASES))
def test_validation_equals_the_recorded_pass(golden, name, tmp_path):
    assert name in golden, f"{name} is not in the golden file"
    got = VG.run_case(name, str(tmp_path))
    diff = _first_difference(got, golden[name])
    assert diff is None, f"{name}: {diff}"
    assert VG.canonical(got) == VG.canonical(golden[name])
