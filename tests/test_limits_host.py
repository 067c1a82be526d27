"""CPU: the host side of the motion limits of constrained decoding (generate(traj_limits=...)).

1. decode.traj_limits_check refuses every kind of bad table (lo > hi, an entry outside [0, nb - 1], a wrong shape, a non-integer or
   device table) and returns a good one as contiguous int32.
2. traj.motion_limits rounds conservatively in every normalisation mode of TargetNorm (none, do_norm, do_standard with per-sample
   max_abs): every bin centre inside a window de-normalises inside the physical box, the bins just outside do not (the window is not
   narrower than it must be), two bins dmax apart de-normalise no farther apart than max_step and two bins dmax + 1 apart do.
   The comparisons use TargetNorm.denorm itself, in float64, with no tolerance: that is the conversion's own definition.
3. traj.limits_violations agrees with the restatement tests/limits_ref.py on hand-made sequences: inside the limits, a jump beyond dmax,
   a waypoint outside the box, a start outside the box by more than dmax that walks in at dmax per step (0 violations) or does not, an
   unknown previous step (a short run before <tsep> in the prompt), and a prompt whose own tokens break the limits but lie before `start`.
4. The driver's --traj_workspace / --traj_max_step parse, need --constrain_traj, and are off by default."""
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import driver, traj as T
from egoscaler_amd.decode import traj_limits_check
from tests import grammar_ref as G
from tests import limits_ref as L

NB = 256
TOK = types.SimpleNamespace(p0=32006, num_bins=NB, ts=32003, tsep=32004, te=32005, eos=2, pad=0)
SPEC = G.Spec(TOK.p0, NB, TOK.ts, TOK.tsep, TOK.te, TOK.eos, 1, 8)


def test_limits_check_refuses_bad_tables():
    good = L.full_range(NB, 3)
    out = traj_limits_check(good, NB, 3)
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (3, 18) and np.array_equal(out.numpy(), good)
    assert torch.equal(traj_limits_check(torch.from_numpy(good).long(), NB, 3), out)
    bad = {}
    bad["lo > hi"] = good.copy()
    bad["lo > hi"][1, 2], bad["lo > hi"][1, 8] = 9, 8
    bad["below 0"] = good.copy()
    bad["below 0"][0, 0] = -1
    bad["hi above nb - 1"] = good.copy()
    bad["hi above nb - 1"][2, 11] = NB
    bad["dmax above nb - 1"] = good.copy()
    bad["dmax above nb - 1"][2, 17] = NB
    bad["dmax below 0"] = good.copy()
    bad["dmax below 0"][0, 12] = -2
    for name, t in bad.items():
        with pytest.raises(ValueError, match="traj_limits"):
            traj_limits_check(t, NB, 3)
    for shape_bad in (good[:2], good[:, :17], good.reshape(-1), good[None]):
        with pytest.raises(ValueError, match="traj_limits"):
            traj_limits_check(shape_bad, NB, 3)
    with pytest.raises(ValueError, match="integer"):
        traj_limits_check(good.astype(np.float32), NB, 3)
    with pytest.raises(ValueError, match="integer"):
        traj_limits_check(torch.from_numpy(good).float(), NB, 3)
    assert np.array_equal(T.motion_limits_bins(nb=NB, rows=3).numpy(), good)
    one = T.motion_limits_bins(lo=[1, 2, 3, 4, 5, 6], hi=200, dmax=2, nb=NB, rows=2).numpy()
    assert one[:, :6].tolist() == [[1, 2, 3, 4, 5, 6]] * 2 and (one[:, 6:12] == 200).all() and (one[:, 12:] == 2).all()
    with pytest.raises(ValueError, match="traj_limits"):
        T.motion_limits_bins(lo=5, hi=4, nb=NB)


NORMS = {
    "none": T.TargetNorm(),
    "norm": T.TargetNorm(do_norm=True),
    "standard": T.TargetNorm(do_standard=True, mean=[0.1, -0.2, 1.1, 0.0, 0.3, -0.1], std=[0.5, 0.7, 0.4, 0.9, 1.3, 0.2]),
}
# physical limits per mode: (lo, hi, max_step); NaN = no limit in that dimension
PHYS = {
    "none": ([-0.5, -1.0, 0.013, np.nan, -0.25, -2.0], [0.5, 0.2, 0.9, np.nan, 0.25, 2.0], [0.05, 0.0, 0.2, np.nan, 3.0, 0.0079]),
    "norm": ([-2.0, -1.3, 0.0, np.nan, -1.0, np.nan], [2.0, 1.21, 2.5, np.nan, 1.0, 0.5], [0.08, 0.1, 0.0099, 0.2, np.nan, 7.0]),
    "standard": ([-0.4, -1.0, 0.6, np.nan, -3.0, -0.3], [0.9, 0.8, 1.7, np.nan, 3.0, 0.05], [0.05, 0.3, 0.01, np.nan, 0.0, 0.1]),
}
MAX_ABS = np.asarray([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [2.5, 0.7, 3.1, 1.9, 1.0, 4.2], [0.31, 5.0, 1.0, 2.2, 3.3, 0.9]])


@pytest.mark.parametrize("mode", list(NORMS))
def test_motion_limits_round_conservatively(mode):
    norm, (lo, hi, step) = NORMS[mode], PHYS[mode]
    lim = T.motion_limits(TOK, norm, lo=lo, hi=hi, max_step=step, max_abs=MAX_ABS).numpy()
    B = len(MAX_ABS)
    assert lim.shape == (B, 18) and lim.dtype == np.int32
    centres = np.linspace(-1, 1, NB)
    phys = norm.denorm(np.broadcast_to(centres[None, :, None], (B, NB, 6)), MAX_ABS)       # [B, NB, 6]
    plo, phi, pst = (np.where(np.isnan(v), f, v) for v, f in ((np.asarray(lo), -np.inf), (np.asarray(hi), np.inf), (np.asarray(step), np.inf)))
    for b in range(B):
        for d in range(6):
            a, z, k = int(lim[b, d]), int(lim[b, 6 + d]), int(lim[b, 12 + d])
            assert 0 <= a <= z <= NB - 1 and 0 <= k <= NB - 1
            inside = phys[b, a:z + 1, d]
            assert inside.min() >= plo[d] and inside.max() <= phi[d], (mode, b, d)
            assert a == 0 or phys[b, a - 1, d] < plo[d], (mode, b, d, "lo could round lower")
            assert z == NB - 1 or phys[b, z + 1, d] > phi[d], (mode, b, d, "hi could round higher")
            if k:
                assert (phys[b, k:, d] - phys[b, :NB - k, d]).max() <= pst[d], (mode, b, d)
            if k < NB - 1:
                assert (phys[b, k + 1:, d] - phys[b, :NB - k - 1, d]).max() > pst[d], (mode, b, d, "dmax could be larger")
    if mode != "standard":                                               # max_abs does not enter: every row is the same, and None gives one row
        assert (lim == lim[0]).all()
        assert np.array_equal(T.motion_limits(TOK, norm, lo=lo, hi=hi, max_step=step).numpy(), lim[:1])
    else:
        assert not (lim == lim[0]).all()
    assert np.array_equal(T.motion_limits(TOK, norm, max_abs=MAX_ABS).numpy(), L.full_range(NB, B))       # None: the full range
    with pytest.raises(ValueError, match="no bin centre"):
        T.motion_limits(TOK, norm, lo=[0.1001] * 6, hi=[0.1002] * 6)


def test_workspace_of_the_reference_is_the_full_range_under_do_norm():
    ws = T.WORKSPACE
    lim = T.motion_limits(TOK, NORMS["norm"], lo=[ws["min_x"], ws["min_y"], ws["min_z"]] + [np.nan] * 3,
                          hi=[ws["max_x"], ws["max_y"], ws["max_z"]] + [np.nan] * 3).numpy()
    assert np.array_equal(lim[:, :12], L.full_range(NB)[:, :12])
    lim = T.motion_limits(TOK, NORMS["norm"], max_step=[0.2] * 3 + [np.nan] * 3).numpy()      # 0.2 m per step: 4 m / 255 per bin in x, y
    assert lim[0, 12:].tolist() == [12, 12, 20, 255, 255, 255]


def _seq(prompt_bins, steps):
    """<ts> prompt step <tsep> | steps ... <te> eos pad pad; -> (ids, the prompt length)."""
    p = [7, 9, TOK.ts] + [TOK.p0 + b for b in prompt_bins] + [TOK.tsep]
    g = []
    for s in steps:
        g += [TOK.p0 + b for b in s] + [TOK.tsep]
    return p + g + [TOK.te, TOK.eos, TOK.pad, TOK.pad], len(p)


def test_limits_violations_against_the_restatement():
    lim = np.asarray([10] * 6 + [200] * 6 + [3] * 6, dtype=np.int32)
    cases = {
        "inside": (_seq([50] * 6, [[53, 47, 50, 51, 49, 50], [56, 44, 50, 52, 48, 53]]), 0),
        "one jump beyond dmax": (_seq([50] * 6, [[54, 50, 50, 50, 50, 50], [57, 50, 50, 50, 50, 50]]), 1),
        "outside the box": (_seq([12] * 6, [[9, 12, 12, 12, 12, 12], [10, 12, 12, 12, 12, 10]]), 1),
        # the prompt's pose lies 8 above / 9 below the box, farther than dmax = 3: the only legal move is dmax toward the box
        "walks in from outside": (_seq([208, 1, 50, 50, 50, 50], [[205, 4, 50, 50, 50, 50], [202, 7, 50, 50, 50, 50], [199, 10, 50, 50, 50, 50]]), 0),
        "jumps in from outside": (_seq([208, 1, 50, 50, 50, 50], [[200, 10, 50, 50, 50, 50]]), 2),
        "stays outside": (_seq([208, 1, 50, 50, 50, 50], [[208, 1, 50, 50, 50, 50]]), 2),
        "overshoots dmax - 1 is not the window": (_seq([208] * 6, [[206] * 6]), 6),
    }
    for name, ((ids, S0), want) in cases.items():
        ref = L.violations(SPEC, ids, lim, start=S0)
        got = int(T.limits_violations(np.asarray([ids]), TOK, lim[None], start=S0)[0])
        assert got == ref == want, (name, got, ref, want)
    # an unknown previous step: the prompt's step holds five bins only, so the first generated step is held against the box alone
    ids = [TOK.ts] + [TOK.p0 + 50] * 5 + [TOK.tsep] + [TOK.p0 + b for b in (199, 11, 200, 10, 100, 150)] + [TOK.tsep, TOK.te, TOK.eos]
    assert L.init_pose(SPEC, ids[:7])[:6] == L.UNKNOWN
    assert int(T.limits_violations(np.asarray([ids]), TOK, lim[None], start=7)[0]) == 0
    ids[8] = TOK.p0 + 9
    assert int(T.limits_violations(np.asarray([ids]), TOK, lim[None], start=7)[0]) == 1
    # the prompt's own tokens break the box: counted from column 0, not from the prompt's end; rows are independent; tensors are taken
    (ids, S0), _ = cases["walks in from outside"]
    both = torch.tensor([ids, cases["inside"][0][0] + [TOK.pad] * (len(ids) - len(cases["inside"][0][0]))])
    lims = torch.from_numpy(np.stack([lim, lim]))
    assert T.limits_violations(both, TOK, lims, start=S0).tolist() == [0, 0]
    assert T.limits_violations(both, TOK, lims).tolist() == [2, 0] == [L.violations(SPEC, r, lim) for r in both.numpy()]
    assert T.limits_violations(both, TOK, torch.from_numpy(L.full_range(NB, 2))).tolist() == [0, 0]
    assert T.limits_violations(np.asarray([[5, 6, 7]]), TOK, lim[None]).tolist() == [0]          # no <ts>: nothing to count
    with pytest.raises(ValueError):
        T.limits_violations(both, TOK, lims[:1])


def test_window_rule_by_hand():
    w = L.window
    assert w(10, 200, 3, -1) == (10, 200) == T.limits_window(10, 200, 3, -1)
    for args, want in (((10, 200, 3, 50), (47, 53)), ((10, 200, 3, 11), (10, 14)), ((10, 200, 3, 199), (196, 200)), ((10, 200, 0, 60), (60, 60)),
                       ((10, 200, 3, 5), (8, 8)), ((10, 200, 3, 7), (10, 10)), ((10, 200, 3, 230), (227, 227)), ((10, 200, 3, 203), (200, 200)),
                       ((0, 255, 255, 0), (0, 255)), ((0, 0, 255, 255), (0, 0)), ((255, 255, 1, 0), (1, 1)), ((7, 7, 0, 9), (9, 9))):
        assert w(*args) == want == T.limits_window(*args), args
    for lo in range(0, 12):
        for hi in range(lo, 12):
            for dmax in range(0, 12):
                for q in range(-1, 12):
                    a, b = w(lo, hi, dmax, q)
                    assert 0 <= a <= b <= 11
                    assert q < 0 or all(abs(x - q) <= dmax for x in (a, b))


def test_driver_flags():
    a = driver.parse_args(["eval", "--tiny"])
    assert a.traj_workspace is None and a.traj_max_step is None and driver.traj_limit_options(a, False) is None
    a = driver.parse_args(["eval", "--tiny", "--constrain_traj", "--traj_workspace=-2,2,-2,2,0,2.5", "--traj_max_step", "0.2,0.2,0.2,,,"])      # (= : the value starts with a minus sign)
    lo, hi, step = driver.traj_limit_options(a, True)
    assert lo[:3] == [-2.0, -2.0, 0.0] and hi[:3] == [2.0, 2.0, 2.5] and step[:3] == [0.2] * 3
    assert all(np.isnan(v) for v in lo[3:] + hi[3:] + step[3:])
    for bad in (["--traj_max_step", "1,1,1,1,1,1"], ["--constrain_traj", "--traj_max_step", "1,1,1"], ["--constrain_traj", "--traj_workspace", "2,-2,0,1,0,1"],
                ["--constrain_traj", "--traj_max_step=-1,1,1,1,1,1"], ["--constrain_traj", "--traj_workspace", "a,b,c,d,e,f"]):
        with pytest.raises(SystemExit):
            driver.parse_args(["eval", "--tiny"] + bad)
    with pytest.raises(ValueError, match="constrain_traj"):
        driver.traj_limit_options(types.SimpleNamespace(traj_max_step="1,1,1,1,1,1"), False)
