"""CPU: the reference tests/test_gpu_binstats_kernel.py holds egomi_bin_stats to (tests/binstats_cases.py) is right where a closed form
exists, and its bounds mean something: three plausible kernel defects, applied to the reference's arithmetic on the same rows, each miss
the kernel bound on at least one case.
  * E[v^2] - mean^2 : the variance as a difference of moments in fp32, on the peaked rows (the cancellation the centred second pass avoids)
  * window sum-exp  : s taken over the window instead of the whole row (mass = 1 whatever the row)
  * shifted values  : the bin values taken one bin edge further (v_i = linspace[i + 1])
A bound of 0 (not yet measured) fails the sanity check below rather than passing everything."""
import numpy as np
import pytest
import torch

from tests import binstats_cases as C

V, NB, P0, R = 4099, 256, 3001, 2 * len(C.KINDS)


def _rows(dtype=torch.float32, V=V, p0=P0, nb=NB):
    return C.received(C.make_rows(R, V, p0, nb, dtype))


def _kind(name):
    return [r for r in range(R) if C.KINDS[r % len(C.KINDS)] == name]


def test_bounds_are_recorded():
    for n in C.NAMES:
        assert 0 < C.MEASURED[n] < C.BOUND[n] == 4 * C.MEASURED[n] < 1e-4, n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_closed_forms_of_the_reference(dtype):
    x = _rows(dtype)
    ref = C.ref_stats(x, P0, NB)
    v = C.values(NB)
    eq = _kind("equal")
    assert np.allclose(ref["mean"][eq], v.mean(), atol=1e-15) and np.allclose(ref["ent"][eq], np.log(NB), rtol=1e-14)
    assert np.allclose(ref["mass"][eq], NB / V, rtol=1e-13)
    assert np.allclose(ref["mass"][_kind("inf_out")], 1.0, rtol=1e-15)
    two = _kind("two")
    assert np.allclose(ref["std"][two], abs(v[0] - v[-1]) / 2, rtol=1e-15) and np.allclose(ref["mean"][two], 0.0, atol=1e-16)
    assert np.allclose(ref["ent"][two], np.log(2.0), rtol=1e-15)
    none = _kind("all_inf")
    assert (ref["mass"][none] == 0).all() and all(np.isnan(ref[n][none]).all() for n in ("mean", "std", "ent"))
    hot = _kind("one_hot")
    assert (ref["std"][hot] == 0).all() and (ref["ent"][hot] == 0).all() and np.isin(ref["mean"][hot], v).all()
    out = _kind("outside")
    assert (ref["mass"][out] < 1e-6).all() and (ref["mass"][out] > 0).all()
    rest = [r for r in range(R) if r not in none]
    assert all(np.isfinite(ref[n][rest]).all() for n in C.NAMES)
    assert (ref["std"][rest] >= 0).all() and (ref["std"][rest] <= 1).all() and (ref["ent"][rest] <= np.log(NB) + 1e-12).all()


def test_offset_rows_are_the_plain_rows():
    g = np.random.default_rng(0)
    x = g.normal(0, 3, (4, V))
    a, b = C.ref_stats(x, P0, NB), C.ref_stats(x + 80.0, P0, NB)
    for n in C.NAMES:
        assert np.allclose(a[n], b[n], rtol=1e-10, atol=1e-12), n


def test_ratio_treats_nan_as_a_value_the_kernel_must_match():
    nan = float("nan")
    assert C.ratio([nan, 1.0], [nan, 1.0]) == 0.0
    assert C.ratio([0.0], [nan]) == np.inf and C.ratio([nan], [0.0]) == np.inf and C.ratio([np.inf], [1.0]) == np.inf
    assert C.ratio([1e-3], [0.0]) == 1e-3                                # a reference of 0 (std of a one-hot row): the absolute error


def _moments_fp32(x, p0, nb):
    """std as sqrt(E[v^2] - mean^2) with every sum and product in fp32."""
    f = np.float32
    v = C.values(nb).astype(f)
    xw = x[:, p0:p0 + nb].astype(f)
    w = np.exp(xw - x.max(1, keepdims=True).astype(f)).astype(f)
    Z = w.sum(1, dtype=f)
    with np.errstate(invalid="ignore"):                                  # (the all_inf rows: 0 / 0)
        mean = ((w * v).sum(1, dtype=f) / Z).astype(f)
        ev2 = ((w * (v * v)).sum(1, dtype=f) / Z).astype(f)
        return np.sqrt((ev2 - mean * mean).astype(f))


def test_difference_of_moments_in_fp32_exceeds_the_bound_on_the_peaked_rows():
    worst = 0.0
    for nb, p0 in ((256, P0), (1024, 1000), (256, V - 256)):
        x = _rows(torch.float32, p0=p0, nb=nb)
        pk = _kind("peak")
        ref = C.ref_stats(x, p0, nb)["std"][pk]
        assert (ref > 1e-4).all() and (ref < 1e-1).all()                 # small, but not lost in sqrt(2^-24): the centred pass resolves it
        worst = max(worst, C.ratio(_moments_fp32(x, p0, nb)[pk], ref))
    assert worst > C.BOUND["std"], worst


def test_sum_exp_over_the_window_only_exceeds_the_bound():
    x = _rows()
    ref = C.ref_stats(x, P0, NB)
    bad = C.ref_stats(x[:, P0:P0 + NB], 0, NB)                           # the window as if it were the whole row
    for n in ("mean", "std", "ent"):                                     # the conditional statistics do not see the defect ...
        assert C.ratio(bad[n], ref[n]) < 1e-12, n
    for kind in ("gauss", "outside", "equal"):                           # ... the mass does, on every row with anything outside
        rows = _kind(kind)
        assert C.ratio(bad["mass"][rows], ref["mass"][rows]) > 1000 * max(C.BOUND["mass"], 1e-7), kind


def test_values_shifted_by_one_bin_exceed_the_bound():
    x = _rows()
    ref = C.ref_stats(x, P0, NB)
    bad = C.ref_stats(x, P0, NB, vals=np.linspace(-1, 1, NB + 1)[1:])   # NB + 1 edges, the upper one of every bin
    rows = [r for r in range(R) if r not in _kind("all_inf")]
    assert C.ratio(bad["mean"][rows], ref["mean"][rows]) > 1000 * max(C.BOUND["mean"], 1e-7)
    bad = C.ref_stats(x, P0, NB, vals=np.r_[C.values(NB)[1:], 1.0 + 2.0 / (NB - 1)])   # the same table read one entry further
    assert C.ratio(bad["mean"][rows], ref["mean"][rows]) > 1000 * max(C.BOUND["mean"], 1e-7)
