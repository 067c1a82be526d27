"""CPU: what the full metric suite rests on that needs no GPU -- traj.dynamic_time_warping against the plain double loop and its own
properties, the driver's record formulas for --full_metrics on hand-made sums, the option's default and flag, the dump merge, and the
declaration of egomi_traj_metrics_full."""
import math
import types

import numpy as np
import pytest

from egoscaler_amd import _abi, driver, traj as T
from tests import traj_full_ref as R

LENGTHS = (1, 2, 3, 7, 20)


def _pair(n, m, seed, D=6):
    g = np.random.default_rng(seed)
    return g.normal(size=(n, D)).astype(np.float32), g.normal(size=(m, D)).astype(np.float32)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("m", LENGTHS)
def test_dtw_equals_the_double_loop(n, m):
    x, y = _pair(n, m, 100 * n + m)
    ref = R.dtw_loop(x.astype(np.float64), y.astype(np.float64))
    got = T.dynamic_time_warping(x, y)
    assert type(got) is float and abs(got - ref) <= 1e-12 * (1 + ref)


@pytest.mark.parametrize("n", LENGTHS)
def test_dtw_of_a_sequence_with_itself_is_zero(n):
    x, _ = _pair(n, 1, n)
    assert T.dynamic_time_warping(x, x) == 0.0


@pytest.mark.parametrize("n,m", [(1, 7), (3, 2), (7, 20), (20, 20)])
def test_dtw_is_symmetric_bit_for_bit(n, m):
    x, y = _pair(n, m, 7 * n + m)
    assert T.dynamic_time_warping(x, y) == T.dynamic_time_warping(y, x)


@pytest.mark.parametrize("m", LENGTHS)
def test_dtw_with_one_step_is_the_sum_of_distances(m):
    x, y = _pair(1, m, m)
    want = sum(float(np.linalg.norm(x[0].astype(np.float64) - y[k].astype(np.float64))) for k in range(m))
    assert abs(T.dynamic_time_warping(x, y) - want) <= 1e-12 * (1 + want)
    assert abs(T.dynamic_time_warping(y, x) - want) <= 1e-12 * (1 + want)


@pytest.mark.parametrize("n,m", [(1, 20), (3, 7), (7, 7), (7, 20), (20, 20)])
def test_dtw_is_at_most_the_padded_alignment(n, m):
    """len(gen) <= len(gt): gen padded with its last step is itself a warping path, of cost ADE * len(gt)."""
    x, y = _pair(n, m, 31 * n + m)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    assert T.dynamic_time_warping(x, y) <= T.average_displacement_error(x64, y64) * m * (1 + 1e-12)


def test_dtw_docstring_states_the_relation_to_the_reference():
    doc = T.dynamic_time_warping.__doc__
    assert "fastdtw" in doc and "upper bound" in doc and "NOT measured" in doc


# ------------------------------------------------------------------------------------------------ the driver's parts
def _sums(**given):
    assert len(set(driver.FULL_SUMS)) == len(driver.FULL_SUMS) and set(given) <= set(driver.FULL_SUMS)
    return {**dict.fromkeys(driver.FULL_SUMS, 0.0), **{k: float(v) for k, v in given.items()}}


def _same(rec, want):
    assert list(rec) == list(want)
    for k, v in want.items():
        assert type(rec[k]) is type(v), k
        assert rec[k] == v or (isinstance(v, float) and math.isnan(v) and math.isnan(rec[k])), k


def test_full_sums_stand_beside_the_existing_tuples():
    names = driver.BASE_SUMS + driver.BEST_SUMS + driver.SEL_SUMS + driver.MODE_SUMS + driver.SOFT_SUMS + driver.FULL_SUMS
    assert len(set(names)) == len(names)
    assert T.FULL_METRICS == ("ADE", "FDE", "IDE", "GD", "DTW")


def test_full_record_of_hand_made_sums():
    s = _sums(IDE=1.5, DTW=9.0, GD_dev=0.3, n_full=3, minIDE=1.0, minGD=0.5, minDTW=4.0, n_fmin=2, GD_sel=2.0, DTW_sel=6.0, n_fsel=4,
              minGD_M=1.0, minDTW_M=3.0, n_fM=2)
    base = {"IDE": 0.5, "DTW": 3.0, "GD_dev": 0.3 / 3, "n_full": 3}
    best = {"minIDE": 0.5, "minGD": 0.25, "minDTW": 2.0}
    sel = {"GD_sel": 0.5, "DTW_sel": 1.5}
    modes = {"minGD_M": 0.5, "minDTW_M": 1.5}
    _same(driver.full_record(types.SimpleNamespace(K=1, select="none", M=0), s), base)
    _same(driver.full_record(types.SimpleNamespace(K=4, select="none", M=0), s), {**base, **best})
    _same(driver.full_record(types.SimpleNamespace(K=4, select="medoid", M=0), s), {**base, **best, **sel})
    _same(driver.full_record(types.SimpleNamespace(K=4, select="medoid", M=2), s), {**base, **best, **sel, **modes})
    _same(driver.full_record(types.SimpleNamespace(K=4, select="none", M=2), s), {**base, **best, **modes})


def test_full_record_of_zero_counts_is_nan():
    nan = float("nan")
    _same(driver.full_record(types.SimpleNamespace(K=4, select="logprob", M=1), _sums()),
          {"IDE": nan, "DTW": nan, "GD_dev": nan, "n_full": 0, "minIDE": nan, "minGD": nan, "minDTW": nan, "GD_sel": nan, "DTW_sel": nan,
           "minGD_M": nan, "minDTW_M": nan})


def test_full_metrics_option_default_and_flag():
    assert driver.val_options(types.SimpleNamespace()).full is False
    assert driver.val_options(driver.parse_args(["eval", "--tiny"])).full is False
    a = driver.parse_args(["eval", "--tiny", "--full_metrics"])
    assert a.full_metrics is True and driver.val_options(a).full is True
    assert driver.val_options(types.SimpleNamespace(), full_metrics=True).full is True
    assert driver.val_options(a, full_metrics=False).full is False    # the explicit keyword comes before args
    for extra in (["--val_greedy"], ["--num_beams", "2"], ["--num_samples", "4", "--select", "medoid", "--num_modes", "2", "--soft_decode"]):
        b = driver.parse_args(["eval", "--tiny", "--full_metrics"] + extra)
        assert driver.val_options(b, num_beams=b.num_beams).full is True


def test_merge_dumps_carries_the_full_sub_dump():
    row = lambda v: {c: [v, None] for c in T.FULL_METRICS}
    r0 = {0: [[0.0] * 6], "full": {0: row(0.5)}}
    r1 = {1: [[1.0] * 6], "selected": {1: 0}, "full": {1: row(1.5)}}
    got = driver.merge_dumps([r0, r1])
    assert got == {0: [[0.0] * 6], 1: [[1.0] * 6], "full": {0: row(0.5), 1: row(1.5)}, "selected": {1: 0}}
    assert r0["full"] == {0: row(0.5)}


def test_the_entry_point_is_declared_as_the_issue_states_it():
    ret, params = _abi.PROTOS["egomi_traj_metrics_full"]
    assert [p for p, _ in params] == ["gen", "n_gen", "gt", "n_gt", "B", "K", "Tmax", "D", "rot0", "out", "mins", "args", "stream"]


def test_metrics_full_refuses_more_than_256_steps_before_any_launch():
    import torch
    gen, gt = torch.zeros(1, 1, 257, 6), torch.zeros(1, 257, 6)       # host tensors: the check comes before anything reaches the library
    with pytest.raises(ValueError, match="256"):
        T.metrics_full(gen, None, gt)
    with pytest.raises(ValueError):
        T.metrics_full(torch.zeros(1, 2, 5, 6), torch.zeros(1, 3), torch.zeros(1, 5, 6))
