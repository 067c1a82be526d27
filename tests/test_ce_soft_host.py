"""CPU: the float64 statement of the bin-aware cross-entropy (tests/ce_soft_ref.py) checked against itself and torch, the bounds it carries
shown to have teeth, traj.soft_target_spec, the driver flags and the exported symbol."""
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import _abi, _lib, build as B, driver, traj
from tests import ce_soft_ref as C

V, P0, NB, IGN = 300, 40, 256, 299                                      # bins 40 .. 295; 296 .. 298 stand for <ts> <tsep> <te>; 299 is the pad
TOK = types.SimpleNamespace(p0=32000, num_bins=256)


def _rows(R, seed=0, V=V):
    return np.random.default_rng(seed).normal(0.0, 3.0, (R, V))


def test_q_sums_to_one_and_is_zero_outside_the_window():
    for sigma, W in ((0.5, 2), (1.0, 3), (2.5, 8), (8.0, 24), (16.0, 32), (1.0, 1), (0.01, 1)):
        spec = (P0, NB, sigma, W)
        tg = np.array([P0, P0 + 1, P0 + W - 1, P0 + W, P0 + 100, P0 + NB - 1 - W, P0 + NB - W, P0 + NB - 1])
        q = C.target_q(tg, V, IGN, spec)
        assert np.all(np.abs(q.sum(1) - 1.0) < 1e-14) and np.all(q >= 0)
        assert np.all(q[:, :P0] == 0) and np.all(q[:, P0 + NB:] == 0)
        for r, t in enumerate(tg):
            i = t - P0
            lo, hi = max(0, i - W), min(NB - 1, i + W)
            assert np.all(q[r, :P0 + lo] == 0) and np.all(q[r, P0 + hi + 1:] == 0)
            assert q[r].argmax() == t and np.all(q[r, P0 + lo:P0 + hi + 1] > 0 if sigma >= 0.5 else True)


def test_truncation_at_both_ends_renormalises():
    sigma, W = 1.0, 3
    w = np.exp(-np.arange(-W, W + 1) ** 2 / 2.0)
    q = C.target_q(np.array([P0, P0 + NB - 1, P0 + 1, P0 + 100]), V, IGN, (P0, NB, sigma, W))
    np.testing.assert_allclose(q[0, P0:P0 + W + 1], w[W:] / w[W:].sum(), rtol=1e-15)             # first bin: the right half alone
    np.testing.assert_allclose(q[1, P0 + NB - 1 - W:P0 + NB], w[:W + 1] / w[:W + 1].sum(), rtol=1e-15)
    np.testing.assert_allclose(q[2, P0:P0 + W + 2], w[W - 1:] / w[W - 1:].sum(), rtol=1e-15)
    np.testing.assert_allclose(q[3, P0 + 100 - W:P0 + 100 + W + 1], w / w.sum(), rtol=1e-15)
    assert C.default_radius(0.5) == 2 and C.default_radius(1.0) == 3 and C.default_radius(2.5) == 8 and C.default_radius(16.0) == 32


@pytest.mark.parametrize("spec", [(P0, 1, 1.0, 3), (P0, NB, 2.5, 8)], ids=["nb1", "specials"])
def test_one_hot_rows_equal_torch_cross_entropy(spec):
    R = 24
    x = _rows(R, 1)
    g = np.random.default_rng(2)
    if spec[1] == 1:
        tg = g.integers(0, V - 1, R)                                         # every id, the single bin P0 among them
        tg[0] = P0
    else:
        tg = g.choice(np.r_[0:P0, P0 + NB:V - 1], R)                         # text and special ids only
    tg[3], tg[7] = IGN, IGN
    ref = C.soft_ce(x, tg, IGN, spec, grad_scale=1.0)
    xt = torch.tensor(x, requires_grad=True)
    loss = torch.nn.functional.cross_entropy(xt, torch.from_numpy(tg), ignore_index=IGN)
    loss.backward()
    n = ref["count"]
    assert n == R - 2
    assert abs(ref["row_loss"].sum() / n - loss.item()) < 1e-13 and np.array_equal(ref["row_loss"], ref["row_nll"])
    assert np.abs(ref["grad"] - xt.grad.numpy()).max() < 1e-15
    assert ref["row_loss"][3] == 0 and not ref["grad"][3].any()
    soft, hard = C.torch_soft_ce(torch.tensor(x), torch.from_numpy(tg), IGN, spec)
    assert abs(float(soft) - loss.item()) < 1e-13 and abs(float(hard) - loss.item()) < 1e-13


def test_out_of_range_targets_are_ignored_and_inf_logits_follow_ieee():
    x = _rows(5, 3)
    tg = np.array([-1, V, V + 7, P0 + 10, P0 + 20])
    x[3, P0 + 11] = -np.inf                                             # under q > 0
    x[4, 5] = -np.inf                                                   # outside the window
    ref = C.soft_ce(x, tg, IGN, (P0, NB, 1.0, 3), count=2)
    assert not ref["row_loss"][:3].any() and not ref["grad"][:3].any()
    assert ref["row_loss"][3] == np.inf and np.isfinite(ref["row_nll"][3]) and np.isfinite(ref["row_loss"][4])
    assert ref["grad"][3, P0 + 11] == -ref["q"][3, P0 + 11] * ref["sc"] and ref["grad"][4, 5] == 0
    assert np.isfinite(ref["grad"]).all()


def test_gradient_matches_finite_differences_and_sums_to_zero():
    R = 6
    x = _rows(R, 4)
    tg = np.array([P0, P0 + 3, P0 + 128, P0 + NB - 1, 297, IGN])
    spec = (P0, NB, 2.5, 8)
    ref = C.soft_ce(x, tg, IGN, spec)
    mean = lambda y: C.soft_ce(y, tg, IGN, spec)["row_loss"].sum() / ref["count"]
    h, worst = 1e-5, 0.0
    for r in range(R):
        for c in np.r_[0:V:7, P0:P0 + 12, P0 + 120:P0 + 137, V - 10:V]:
            xp, xm = x.copy(), x.copy()
            xp[r, c] += h
            xm[r, c] -= h
            worst = max(worst, abs((mean(xp) - mean(xm)) / (2 * h) - ref["grad"][r, c]))
    print(f"soft CE: worst |finite difference - (p - q) / count| = {worst:.2e}")
    assert worst < 1e-8
    assert np.abs(ref["grad"].sum(1)).max() < 1e-15 and not ref["grad"][5].any()
    soft, _ = C.torch_soft_ce(torch.tensor(x), torch.from_numpy(tg), IGN, spec)
    assert abs(soft.item() - mean(x)) < 1e-13


# -- the bounds have teeth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5])
@pytest.mark.parametrize("defect", C.DEFECTS)
def test_defects_miss_both_bounds_by_more_than_100x(defect, sigma):
    """q not renormalised at a window edge, the window centred one bin off, mass spilling to p0 - 1: each applied to the float64 reference
    on Gaussian rows whose targets sit at the window's ends (and, for the shifted centre, anywhere)."""
    W = C.default_radius(sigma)
    tg = np.array([P0, P0 + NB - 1, P0 + 1, P0 + 100])
    x = _rows(len(tg), 5)
    spec = (P0, NB, sigma, W)
    ref, bad = C.soft_ce(x, tg, IGN, spec, grad_scale=0.37), C.soft_ce(x, tg, IGN, spec, grad_scale=0.37, defect=defect)
    # the rows the defect is judged on: a target on the edge itself for the two edge defects (one bin further in, the mass at stake is that
    # of the Gaussian's last kept bin, e^-8 at sigma 0.5: too little to ask 100x of), every kind of row for the shifted centre
    rows = {"no_renorm": [0, 1], "off_by_one": [0, 2, 3], "spill": [0]}[defect]
    for bf16_out in (False, True):
        b = C.grad_bound(x, ref, bf16_out)
        for r in rows:
            # the bound proper (fp32 output) is missed by far more than 100x by every defect.  With a bf16 output the rounding term alone is
            # 2^-8 |ref|, so a defect that rescales q by 1 - d cannot miss by more than 256 d: a Gaussian cut at an edge bin keeps
            # d = (e^-2 + e^-8) / (1 + 2 e^-2 + 2 e^-8) = 10.7 % of its mass beyond the edge at sigma 0.5 (27x), 31 % at sigma 1 (79x), 43 % at
            # sigma 2.5 (110x).  That one combination is held to 25x, which is all the arithmetic allows; the other two defects move mass
            # to ids where the reference has none and pass 100x with a bf16 output too.
            need = 25 if (bf16_out and defect == "no_renorm") else 100
            assert (np.abs(bad["grad"][r] - ref["grad"][r]) / b[r]).max() > need, (defect, r, bf16_out)
    for r in rows:
        assert C.loss_ratio(bad["row_loss"][r:r + 1], ref["row_loss"][r:r + 1]) > 100, (defect, r)
    assert C.loss_ratio(ref["row_loss"], ref["row_loss"]) == 0 and C.grad_ratio(ref["grad"], x, ref, False) == 0


def test_ratio_helpers_on_non_finite_values():
    assert C.loss_ratio([np.inf, 1.0], [np.inf, 1.0]) == 0 and C.loss_ratio([1e30], [np.inf]) == np.inf and C.loss_ratio([np.inf], [1.0]) == np.inf
    assert C.loss_ratio([np.nan], [np.nan]) == 0 and C.loss_ratio([np.nan], [1.0]) == np.inf


# -- the package ---------------------------------------------------------------------------------------------------------------------------
def test_soft_target_spec_defaults_and_refusals():
    assert traj.soft_target_spec(TOK, 1.0) == traj.SoftTargetSpec(32000, 256, 1.0, 3) == (32000, 256, 1.0, 3)
    assert traj.soft_target_spec(TOK, 0.5).radius == 2 and traj.soft_target_spec(TOK, 2.5).radius == 8
    assert traj.soft_target_spec(TOK, 16).radius == 32 and traj.soft_target_spec(TOK, 11.0).radius == 32
    assert traj.soft_target_spec(TOK, 0.1).radius == 1 and traj.soft_target_spec(TOK, 2.5, radius=1).radius == 1
    assert traj.soft_target_spec(TOK, 1.0, radius=np.int64(32)).radius == 32
    assert traj.SoftTargetSpec._fields == ("p0", "nb", "sigma", "radius")
    for sigma in (0, -1.0, 16.5, float("nan"), float("inf"), None, "wide"):
        with pytest.raises(ValueError):
            traj.soft_target_spec(TOK, sigma)
    for radius in (0, -3, 33, 2.5, True):
        with pytest.raises(ValueError):
            traj.soft_target_spec(TOK, 1.0, radius=radius)
    for sigma in (0.5, 1.0, 2.5, 8.0):
        assert traj.soft_target_spec(TOK, sigma).radius == C.default_radius(sigma)


def test_driver_flags():
    a = driver.parse_args(["train", "--tiny"])
    assert a.bin_sigma == 0.0 and a.bin_radius is None
    a = driver.parse_args(["train", "--tiny", "--bin_sigma", "1.5", "--bin_radius", "4"])
    assert a.bin_sigma == 1.5 and a.bin_radius == 4
    for bad in (["--bin_sigma", "-1"], ["--bin_sigma", "nan"], ["--bin_sigma", "inf"], ["--bin_sigma", "17"], ["--bin_sigma", "1", "--bin_radius", "0"],
                ["--bin_sigma", "1", "--bin_radius", "33"], ["--bin_radius", "3"]):
        with pytest.raises(SystemExit):
            driver.parse_args(["train", "--tiny"] + bad)


def test_library_exports_the_entry_point_with_the_headers_arity():
    names = [p for p, _ in _abi.PROTOS["egomi_ce_soft_fwd_bwd"][1]]
    assert names == ["logits", "ld", "targets", "R", "V", "ignore", "count", "p0", "nb", "sigma", "radius", "loss_sum", "nll_sum", "row_loss",
                     "row_nll", "dlogits", "ldd", "grad_scale", "dtype", "stream"]
    B.build()
    fn = _lib.lib().egomi_ce_soft_fwd_bwd
    assert len(fn.argtypes) == 20 and len(_abi.PROTOS["egomi_ce_fwd_bwd"][1]) == 14
