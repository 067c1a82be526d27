"""CPU: what egomi_traj_modes rests on that needs no GPU -- the numpy restatement's own properties on the clustered inputs of the GPU tests
(tests/modes_ref.py), the declaration in include/egomi.h and its binding, and the driver's flags."""
import os
import re
import types

import numpy as np
import pytest

from egoscaler_amd import _abi, driver
from tests import modes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K,Tm,D", [(16, 7, 6), (33, 25, 3), (2, 7, 3), (3, 1, 3), (64, 1, 6), (64, 7, 6)])
def test_clustered_inputs_keep_their_margin_and_select_ref_finds_the_clusters(K, Tm, D):
    gen, n, lab = R.clustered_inputs(K, Tm, D)
    assert gen.dtype == np.float32 and n.dtype == np.int32 and (n[1] > 0).sum() == 1 and not n[2].any() and (n[3] == Tm).all()
    if K >= 3:
        assert np.array_equal(gen[3, 1], gen[3, K - 1])
    sc = R.distinct_scores(4, K, K)
    assert all(len(set(sc[b].tolist())) == K for b in range(4))
    for ng in (n, None):
        d = R.dist_ref(gen, ng)
        assert np.array_equal(d, d.transpose(0, 2, 1), equal_nan=True)
        valid = (np.minimum(ng, Tm) > 0) if ng is not None else np.ones((4, K), bool)
        assert np.array_equal(~np.isnan(d), valid[:, :, None] & valid[:, None, :])
        intra, inter = R.margins(d, lab)
        assert min(R.RADIUS - intra.max(), inter.min() - R.RADIUS) > R.margin_for(K, Tm, D) >= R.LOW_MARGIN
        assert all(k >= 16 and t == 1 for k, t, _ in R.LOW) and R.margin_for(K, Tm, D) == (R.LOW_MARGIN if (K, Tm, D) in R.LOW else 0.79)
        present = R.clusters_present(d, lab)
        for M in (1, 3, 6, 64):
            for s in (sc, None):
                for b in range(4):
                    modes, conf, assign, nm, nnms = R.select_ref(d[b], None if s is None else s[b], M, R.RADIUS)
                    nv = int(valid[b].sum())
                    assert nnms == min(M, present[b]) and nnms <= nm <= min(M, nv)
                    assert len({int(lab[b, j]) for j in modes[:nnms]}) == nnms and np.all(modes[nm:] == -1)
                    if nv:
                        assert abs(conf.sum() - 1.0) < 1e-12 and np.all(assign[valid[b]] >= 0) and np.all(assign[~valid[b]] == -1)
                        if s is not None:                              # the best-scored valid sample leads
                            assert modes[0] == max(np.flatnonzero(valid[b]), key=lambda j: s[b, j])
                    else:
                        assert nm == 0 and not conf.any()
                    if b == 3 and K >= 3:
                        assert not {1, K - 1} <= set(modes.tolist())
                    # each cluster's NMS mode collects its cluster: the confidences of the NMS run alone are the clusters' shares
                    if nm == nnms == present[b] and nv:
                        for m in range(nm):
                            share = np.mean(lab[b][valid[b]] == lab[b, modes[m]])
                            assert conf[m] == float(int(round(share * nv))) / float(nv)


def test_select_ref_fill_and_ties_on_a_hand_made_matrix():
    d = np.array([[0, 0, 3, 5, np.nan], [0, 0, 3, 5, np.nan], [3, 3, 0, 4, np.nan], [5, 5, 4, 0, np.nan], [np.nan] * 5], dtype=np.float64)
    modes, conf, assign, nm, nnms = R.select_ref(d, np.array([1, 5, 2, 3, 9], dtype=np.float32), 4, 10.0)
    assert (nm, nnms) == (3, 1) and modes.tolist() == [1, 3, 2, -1]    # best valid score, then the farthest, then the next; 0 duplicates 1
    assert assign.tolist() == [0, 0, 2, 1, -1] and conf.tolist() == [0.5, 0.25, 0.25, 0.0]
    modes, _, _, nm, nnms = R.select_ref(d, None, 2, 0.0)              # centrality: 0 and 1 tie at (0 + 3 + 5) / 3, the lower index leads
    assert modes.tolist() == [0, 2] and (nm, nnms) == (2, 2)


def test_symbol_is_declared_and_bound_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "egomi.h")).read()
    m = re.search(r"^int egomi_traj_modes\((.*?)\);", text, flags=re.S | re.M)
    assert m, "egomi_traj_modes is not declared in include/egomi.h"
    ret, params = _abi.PROTOS["egomi_traj_modes"]
    assert len(params) == len(m.group(1).split(",")) == 16
    assert [p for p, _ in params] == ["gen", "n_gen", "score", "B", "K", "Tmax", "D", "M", "radius", "dist", "modes", "conf", "assign", "n_modes",
                                      "n_nms", "stream"]
    import ctypes
    assert ret is ctypes.c_int and params[8][1] is ctypes.c_double and all(t is ctypes.c_int for _, t in params[3:8])
    assert all(t is ctypes.c_void_p for _, t in params[:3] + params[9:])


def test_driver_flags():
    base = ["eval", "--tiny"]
    a = driver.parse_args(base)
    assert a.num_modes == 0 and a.mode_radius == 0.0
    a = driver.parse_args(base + ["--num_samples", "8", "--num_modes", "3", "--mode_radius", "0.25"])
    assert (a.num_modes, a.mode_radius) == (3, 0.25)
    for bad in (["--num_modes", "2"], ["--num_samples", "1", "--num_modes", "1"], ["--num_samples", "4", "--num_modes", "5"],
                ["--num_samples", "65", "--num_modes", "2"], ["--num_samples", "4", "--num_modes", "-2"], ["--num_samples", "4", "--mode_radius", "1"],
                ["--num_samples", "4", "--num_modes", "2", "--mode_radius", "-0.1"], ["--num_samples", "4", "--num_modes", "2", "--mode_radius", "nan"]):
        with pytest.raises(SystemExit):
            driver.parse_args(base + bad)
    model = types.SimpleNamespace(dims=None)                           # run_validation checks its options before it touches the model
    for kw in (dict(num_samples=1, num_modes=1), dict(num_samples=4, num_modes=5), dict(num_samples=65, num_modes=2),
               dict(num_samples=4, mode_radius=0.5), dict(num_samples=4, num_modes=2, mode_radius=-1.0)):
        with pytest.raises(ValueError):
            driver.run_validation(model, None, driver.parse_args(base), "cpu", **kw)
