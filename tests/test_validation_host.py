"""Host: the pieces run_validation is made of that need no GPU: the option check shared with parse_args, the rank merge of the dumps, the
record formulas on hand-made sums, and the pad-with-the-last-step rule."""
import math
import types

import numpy as np
import pytest

from egoscaler_amd import driver

BASE = ["eval", "--tiny"]
K4 = ["--num_samples", "4"]


def _raises(fn, exc):
    try:
        fn()
    except exc:
        return True
    return False


# ------------------------------------------------------------------------------------------------ the option check
# (extra command-line arguments, is it refused).  The rules the command line applies: parse_args exits exactly where the check raises.
CLI_TABLE = [
    ([], False),
    (K4, False),
    (K4 + ["--select", "medoid"], False),
    (K4 + ["--select", "logprob", "--rescore"], False),
    (K4 + ["--num_modes", "4", "--mode_radius", "0.25"], False),
    (["--num_samples", "64", "--num_modes", "64"], False),
    (K4 + ["--num_modes", "2", "--soft_decode"], False),
    (["--val_greedy", "--soft_decode"], False),
    (["--num_beams", "2"], False),
    (["--soft_decode", "--num_beams", "2"], True),
    (["--num_modes", "1"], True),
    (K4 + ["--num_modes", "5"], True),
    (["--num_samples", "65", "--num_modes", "2"], True),
    (K4 + ["--num_modes", "-2"], True),
    (K4 + ["--mode_radius", "1"], True),
    (K4 + ["--num_modes", "2", "--mode_radius", "-0.1"], True),
    (K4 + ["--num_modes", "2", "--mode_radius", "nan"], True),
    (["--rescore"], True),
    (K4 + ["--rescore"], True),
    (K4 + ["--rescore", "--select", "medoid"], True),
    (["--rescore", "--select", "logprob"], True),
]
# the rules on the decoding mode stay errors of the run: main() raises ValueError there (tests/test_gpu_traj_best_of.py,
# tests/test_gpu_generate_logprobs.py pin it), so parse_args lets them through and run_validation's check raises
RUN_ONLY = [K4 + ["--val_greedy"], K4 + ["--num_beams", "2"], ["--select", "medoid"], ["--num_samples", "-1"]]


def _options_of(argv):
    """The keyword arguments evaluate() hands run_validation for this command line, parsed without parse_args' own check."""
    a = types.SimpleNamespace(num_samples=1, num_beams=1, val_sample=True, select="none", rescore=False, num_modes=0, mode_radius=0.0,
                              soft_decode=False)
    flags = {"--val_greedy": ("val_sample", False), "--rescore": ("rescore", True), "--soft_decode": ("soft_decode", True)}
    i = 0
    while i < len(argv):
        if argv[i] in flags:
            setattr(a, *flags[argv[i]])
            i += 1
        else:
            name = argv[i][2:]
            setattr(a, name, argv[i + 1] if name == "select" else (float if name == "mode_radius" else int)(argv[i + 1]))
            i += 2
    return a


@pytest.mark.parametrize("extra,bad", CLI_TABLE)
def test_parse_args_exits_exactly_where_the_check_raises(extra, bad):
    a = _options_of(extra)
    assert _raises(lambda: driver.val_options(a, num_beams=a.num_beams), ValueError) is bad
    assert _raises(lambda: driver.parse_args(BASE + extra), SystemExit) is bad
    model = types.SimpleNamespace(dims=None)                           # run_validation checks its options before it touches anything
    if bad:
        with pytest.raises(ValueError):
            driver.run_validation(model, None, a, "cpu", num_beams=a.num_beams)


@pytest.mark.parametrize("extra", RUN_ONLY)
def test_decoding_mode_rules_are_errors_of_the_run(extra):
    a = driver.parse_args(BASE + extra)                                # no exit
    with pytest.raises(ValueError):
        driver.run_validation(types.SimpleNamespace(dims=None), None, a, "cpu", num_beams=a.num_beams)


def test_explicit_keywords_come_before_args():
    a = driver.parse_args(BASE + K4 + ["--select", "medoid", "--num_modes", "2", "--mode_radius", "0.5"])
    o = driver.val_options(a)
    assert (o.K, o.select, o.M, o.radius, o.soft, o.rescore, o.sample, o.num_beams) == (4, "medoid", 2, 0.5, False, False, True, 1)
    o = driver.val_options(a, num_samples=8, select="logprob", num_modes=3, mode_radius=0.0, soft_decode=True)
    assert (o.K, o.select, o.M, o.radius, o.soft) == (8, "logprob", 3, 0.0, True)
    o = driver.val_options(types.SimpleNamespace())                    # nothing given anywhere: the defaults
    assert (o.K, o.select, o.M, o.radius, o.soft, o.rescore, o.sample) == (1, "none", 0, 0.0, False, False, True)


# ------------------------------------------------------------------------------------------------ the dump merge
def test_merge_dumps_equals_the_single_rank_dump_of_the_union():
    traj = lambda i: [[float(i)] * 6] * 2
    r0 = {0: traj(0), 1: [traj(1), None]}                              # no sub-dump at all
    r1 = {2: traj(2), "selected": {2: 1}, "modes": {2: {"index": [1, 0], "conf": [0.75, 0.25]}}, "soft": {2: {"mean": traj(2), "std": traj(0)}}}
    r2 = {3: traj(3), 4: traj(4), "selected": {3: 0, 4: 3}, "soft": {3: {"mean": traj(3), "std": traj(0)}}}
    union = {0: traj(0), 1: [traj(1), None], 2: traj(2), 3: traj(3), 4: traj(4), "selected": {2: 1, 3: 0, 4: 3},
             "modes": {2: {"index": [1, 0], "conf": [0.75, 0.25]}},
             "soft": {2: {"mean": traj(2), "std": traj(0)}, 3: {"mean": traj(3), "std": traj(0)}}}
    got = driver.merge_dumps([r0, r1, r2])
    assert got == union and list(got) == list(union)                   # trajectories first, then the sub-dumps in their order
    assert driver.merge_dumps([r0]) == r0 and driver.merge_dumps([{}, {}]) == {}
    assert r1["selected"] == {2: 1}                                    # the ranks' dumps are left as they were


# ------------------------------------------------------------------------------------------------ the sums
def _sums(**given):
    names = driver.BASE_SUMS + driver.BEST_SUMS + driver.SEL_SUMS + driver.MODE_SUMS + driver.SOFT_SUMS
    assert len(set(names)) == len(names) and set(given) <= set(names)
    return {**dict.fromkeys(names, 0.0), **{k: float(v) for k, v in given.items()}}


def _same(rec, want):
    assert list(rec) == list(want)
    for k, v in want.items():
        assert type(rec[k]) is type(v), k                              # plain float / int / str: checkpoints are read with weights_only=True
        assert rec[k] == v or (isinstance(v, float) and math.isnan(v) and math.isnan(rec[k])), k


def test_records_of_hand_made_sums():
    o = types.SimpleNamespace(K=4, select="medoid", M=3, radius=0.5)
    s = _sums(ADE=1.5, FDE=3.0, ADE_as_called=0.75, GD=0.3, n=3, minADE=1.0, minFDE=2.0, n_min=2, ADE_sel=4.0, FDE_sel=6.0, n_sel=4,
              minADE_M=1.0, minFDE_M=3.0, brierADE_M=5.0, n_M=2, modes=7, clips_M=4, ADE_soft=0.9, FDE_soft=1.2, n_soft=3, std=0.6, n_std=24,
              mass_min=2.7)
    _same(driver.base_record(o, s), {"ADE": 1.5 / 3, "FDE": 1.0, "ADE_as_called": 0.25, "GD": 0.3 / 3, "n": 3})
    _same(driver.best_of_record(o, s), {"minADE": 0.5, "minFDE": 1.0, "n_min": 2, "K": 4})
    _same(driver.select_record(o, s), {"ADE_sel": 1.0, "FDE_sel": 1.5, "n_sel": 4, "select": "medoid"})
    _same(driver.modes_record(o, s), {"minADE_M": 0.5, "minFDE_M": 1.5, "brierADE_M": 2.5, "n_modes": 1.75, "M": 3, "mode_radius": 0.5})
    _same(driver.soft_record(o, s), {"ADE_soft": 0.9 / 3, "FDE_soft": 1.2 / 3, "n_soft": 3, "sigma_mean": 0.6 / 24, "bin_mass_min": 2.7 / 3})


def test_records_of_zero_counts_are_nan():
    o, nan = types.SimpleNamespace(K=2, select="logprob", M=1, radius=0.0), float("nan")
    s = _sums(modes=0, clips_M=2)                                      # clips without a single parsed sample: modes counted, nothing hit
    _same(driver.base_record(o, s), {"ADE": nan, "FDE": nan, "ADE_as_called": nan, "GD": nan, "n": 0})
    _same(driver.best_of_record(o, s), {"minADE": nan, "minFDE": nan, "n_min": 0, "K": 2})
    _same(driver.select_record(o, s), {"ADE_sel": nan, "FDE_sel": nan, "n_sel": 0, "select": "logprob"})
    _same(driver.modes_record(o, s), {"minADE_M": nan, "minFDE_M": nan, "brierADE_M": nan, "n_modes": 0.0, "M": 1, "mode_radius": 0.0})
    _same(driver.soft_record(o, s), {"ADE_soft": nan, "FDE_soft": nan, "n_soft": 0, "sigma_mean": nan, "bin_mass_min": nan})
    s = _sums()
    assert math.isnan(driver.modes_record(o, s)["n_modes"])


def test_sums_add_in_float64_whatever_the_term():
    s = _sums()
    driver._add(s, ADE=np.float32(0.1), n=1)
    driver._add(s, ADE=np.float32(0.2), n=np.int32(1))
    assert s["ADE"] == float(np.float32(0.1)) + float(np.float32(0.2)) and s["n"] == 2.0 and type(s["ADE"]) is float


# ------------------------------------------------------------------------------------------------ the pad step
def test_pad_last_step_is_the_rule():
    Tn, rng = 6, np.random.default_rng(0)
    n = np.array([0, 1, Tn - 1, Tn, Tn + 3])
    vals = rng.standard_normal((len(n), Tn, 6)).astype(np.float32)
    want = vals.copy()
    for r in np.nonzero((n > 0) & (n < Tn))[0]:
        want[r, n[r]:] = vals[r, n[r] - 1]
    got = driver.pad_last_step(vals.copy(), n)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], vals[0]) and np.array_equal(got[3], vals[3]) and np.array_equal(got[4], vals[4])     # 0, Tn, beyond: untouched
    assert (got[1] == vals[1, 0]).all() and np.array_equal(got[2, :Tn - 1], vals[2, :Tn - 1]) and np.array_equal(got[2, Tn - 1], vals[2, Tn - 2])
