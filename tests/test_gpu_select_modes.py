"""GPU: egomi_traj_modes (csrc/modes.hip) through traj.select_modes / traj.metrics_modes, against tests/modes_ref.py.
  * dist against the float64 numpy restatement: the same NaN pattern, < 1e-12 elsewhere (the bar of tests/test_gpu_select_kernels.py's
    medoid test), bit-symmetric, exact zeros on the diagonal of valid samples
  * the rules, exactly, on the values returned: select_ref run on the kernel's OWN dist with the same scores reproduces modes, n_modes,
    n_nms, assign and conf (==) -- a last-bit difference in a distance cannot excuse anything
  * from scratch on clustered clips (every pair of samples is farther from the radius than modes_ref.margin_for, asserted here): n_nms is
    the number of clusters present, capped at M, and the NMS modes are the reference's
  * M = 1 is seq_rank's / select_medoid's pick; edge clips, edge radii, NaN and -inf scores, replay bits, argument checks, metrics_modes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib, decode, traj as T
from egoscaler_amd.ops import P, S
from tests import modes_ref as R

pytestmark = pytest.mark.gpu
c_i, c_d = ctypes.c_int, ctypes.c_double
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def _case(K, Tm, D, B=4):
    """The shape's inputs and float64 references, computed once and shared read-only by every test of the shape."""
    gen, n, lab = R.clustered_inputs(K, Tm, D, B=B)
    refs = {True: R.dist_ref(gen, n), False: R.dist_ref(gen, None)}
    sc = R.distinct_scores(B, K, 7 * K + Tm)
    for a in (gen, n, lab, sc, refs[True], refs[False]):
        a.setflags(write=False)
    return gen, n, lab, refs, sc


@functools.lru_cache(maxsize=None)
def _separation(K, Tm, D, with_n):
    """(smallest |distance - RADIUS| over the valid pairs, clusters present per clip) of the shape's reference distances."""
    gen, n, lab, refs, _ = _case(K, Tm, D)
    intra, inter = R.margins(refs[with_n], lab)
    return min(R.RADIUS - float(intra.max()), float(inter.min()) - R.RADIUS), R.clusters_present(refs[with_n], lab)


def _run(gen, n, sc, M, radius):
    out = T.select_modes(torch.tensor(gen).cuda(), None if n is None else torch.tensor(n).cuda(),
                         None if sc is None else torch.tensor(sc).cuda(), num_modes=M, radius=radius, return_dist=True)
    return tuple(t.cpu().numpy() for t in out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_dist(dist, ref):
    assert np.array_equal(np.isnan(dist), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = float(np.abs(dist[ok] - ref[ok]).max()) if ok.any() else 0.0
    assert err < TOL, err
    assert np.array_equal(_bits(dist), _bits(dist.transpose(0, 2, 1)))                  # bit-symmetric
    diag = np.diagonal(dist, axis1=1, axis2=2)
    assert np.all((diag == 0.0) | np.isnan(diag)) and not np.signbit(diag[~np.isnan(diag)]).any()


def _check_rules(got, sc, M, radius):
    """select_ref on the kernel's own dist reproduces everything else the kernel returned, exactly."""
    modes, conf, assign, n_modes, n_nms, dist = got
    for b in range(dist.shape[0]):
        rm, rc, ra, rn, rnms = R.select_ref(dist[b], None if sc is None else sc[b], M, radius)
        assert (n_modes[b], n_nms[b]) == (rn, rnms), (b, n_modes[b], n_nms[b], rn, rnms)
        assert np.array_equal(modes[b], rm) and np.array_equal(assign[b], ra), (b, modes[b], rm)
        assert np.array_equal(conf[b], rc), (b, conf[b], rc)                             # ==: a ratio of two small integers


def _check_invariants(got, M):
    modes, conf, assign, n_modes, n_nms, dist = got
    B, K = assign.shape
    for b in range(B):
        valid = [j for j in range(K) if not np.isnan(dist[b, j, j])]
        nm = int(n_modes[b])
        assert 0 <= n_nms[b] <= nm <= min(M, len(valid))
        used = modes[b, :nm].tolist()
        assert len(set(used)) == nm and set(used) <= set(valid) and np.all(modes[b, nm:] == -1) and np.all(conf[b, nm:] == 0.0)
        if valid:
            assert nm >= 1 and abs(float(conf[b, :nm].sum()) - 1.0) < 1e-12
            counts = conf[b, :nm] * len(valid)
            assert np.all(np.abs(counts - np.round(counts)) < 1e-9) and int(np.round(counts).sum()) == len(valid) and np.all(counts >= 1 - 1e-9)
            assert all(assign[b, m] == s for s, m in enumerate(used))                    # a mode is assigned to itself
        inv, val = np.array([j for j in range(K) if j not in valid], dtype=int), np.array(valid, dtype=int)
        assert np.all(assign[b, inv] == -1) and np.all((assign[b, val] >= 0) & (assign[b, val] < max(nm, 1)))


@pytest.mark.parametrize("M", [1, 3, 6, 64])
@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("Tm", [1, 7, 25])
@pytest.mark.parametrize("K", [1, 2, 3, 16, 33, 64])
def test_modes_against_the_rules_and_from_scratch(K, Tm, D, M):
    gen, n, lab, refs, scores = _case(K, Tm, D)
    for with_n in (True, False):
        ref = refs[with_n]
        margin, present = _separation(K, Tm, D, with_n)
        assert margin > R.margin_for(K, Tm, D), margin                                  # the inputs' own property; see modes_ref.LOW_MARGIN
        for sc in (scores, None):
            got = _run(gen, n if with_n else None, sc, M, R.RADIUS)
            modes, conf, assign, n_modes, n_nms, dist = got
            _check_dist(dist, ref)
            _check_rules(got, sc, M, R.RADIUS)
            _check_invariants(got, M)
            for b in range(4):                                                           # from scratch: the reference on its own distances
                rm, _, _, _, rnms = R.select_ref(ref[b], None if sc is None else sc[b], M, R.RADIUS)
                assert n_nms[b] == rnms == min(M, present[b]), (b, n_nms[b], rnms, present[b])
                assert np.array_equal(modes[b, :rnms], rm[:rnms])
                assert len({int(lab[b, j]) for j in modes[b, :rnms]}) == rnms            # one NMS mode per cluster
            if with_n:
                assert modes[1, 0] == K - 1 and conf[1, 0] == 1.0 and n_modes[1] == 1 and assign[1, K - 1] == 0     # one valid sample
                assert np.all(modes[2] == -1) and np.all(conf[2] == 0.0) and np.all(assign[2] == -1) and n_modes[2] == 0 == n_nms[2]
            if K >= 3:                                                                   # bit-identical samples 1 and K - 1: never two modes
                assert dist[3, 1, K - 1] == 0.0 and not {1, K - 1} <= set(modes[3].tolist())
            if M == 1:
                if sc is not None:
                    _, order = decode.seq_rank(torch.tensor(sc).cuda().view(-1), torch.ones(4 * K, dtype=torch.int32, device="cuda"), 4, K, 0.0)
                    order = order.cpu().numpy()
                    for b in range(4):                                                   # the first-ranked index (that parsed, where lengths are given)
                        v = [j for j in order[b] if not np.isnan(dist[b, j, j])]
                        assert modes[b, 0] == (v[0] if v else -1)
                        if not with_n:
                            assert modes[b, 0] == order[b, 0]
                else:
                    pick, _ = T.select_medoid(torch.tensor(gen).cuda(), torch.tensor(n).cuda() if with_n else None)
                    assert np.array_equal(modes[:, 0], pick.cpu().numpy())


def test_more_clips_than_compute_units():
    # no margin is asserted for this shape: nothing here is from scratch, the rules are checked on the kernel's own dist alone
    K, Tm, D, M, B = 5, 7, 3, 3, 300
    gen, n, lab, refs, scores = _case(K, Tm, D, B)
    for sc in (scores, None):
        got = _run(gen, n, sc, M, R.RADIUS)
        _check_dist(got[5], refs[True])
        _check_rules(got, sc, M, R.RADIUS)
        _check_invariants(got, M)


@pytest.mark.parametrize("K,Tm,D", [(3, 7, 6), (16, 25, 3), (33, 7, 6), (64, 5, 6)])
def test_lengths_ragged_per_sample(K, Tm, D):
    """The clustered clips give one length to a whole cluster; here every sample has a length of its own (0 and beyond Tmax included) on
    plain Gaussian samples, so the own-last-step padding runs between every pair.  No clusters, so no margin and nothing from scratch:
    dist against dist_ref, and the rules on the kernel's own dist."""
    g = np.random.default_rng(1000 * K + 10 * Tm + D)
    gen = g.normal(0, 1, (4, K, Tm, D)).astype(np.float32)
    n = g.integers(0, Tm + 3, (4, K)).astype(np.int32)
    n[0, 0], n[1, :], n[1, K - 1] = Tm, 1, Tm                          # clip 1: single steps against one full-length sample
    ref, scores = R.dist_ref(gen, n), R.distinct_scores(4, K, K + Tm)
    for sc in (scores, None):
        for M, radius in ((1, 0.0), (6, 1.5), (64, 0.0)):
            got = _run(gen, n, sc, M, radius)
            _check_dist(got[5], ref)
            _check_rules(got, sc, M, radius)
            _check_invariants(got, M)
        if sc is None:
            pick, _ = T.select_medoid(torch.tensor(gen).cuda(), torch.tensor(n).cuda())
            assert np.array_equal(_run(gen, n, None, 1, 0.0)[0][:, 0], pick.cpu().numpy())


@pytest.mark.parametrize("D", [1, 6])
@pytest.mark.parametrize("Tm", [1, 7])
@pytest.mark.parametrize("K", [1, 2, 3, 64])
def test_medoid_cost_is_the_index_order_mean_of_a_row_of_dist(K, Tm, D):
    """select_medoid's cost from select_modes' dist, bit for bit: both kernels call one pairwise distance (csrc/traj_disp.h), so
    cost[b, j] is the float64 sum of dist[b, j, i] over the valid i != j in index order, divided once; 0 with no other valid sample, NaN
    for an invalid j.  Clip 0 ragged lengths (0 included), clip 1 one valid sample, clip 2 none, clip 3 two identical samples."""
    g = np.random.default_rng(100 * K + 10 * Tm + D)
    gen = g.normal(0, 1, (4, K, Tm, D)).astype(np.float32)
    n = g.integers(0, Tm + 1, (4, K)).astype(np.int32)
    n[0, 0] = 0
    n[1, :], n[1, K - 1] = 0, Tm
    n[2, :] = 0
    n[3, :] = np.maximum(n[3, :], 1)
    if K >= 2:
        gen[3, K - 1], n[3, K - 1] = gen[3, 0], n[3, 0]
    dist = _run(gen, n, None, 1, 0.0)[5]
    pick, cost = T.select_medoid(torch.tensor(gen).cuda(), torch.tensor(n).cuda())
    cost = cost.cpu().numpy()
    ref = np.full((4, K), np.nan)
    for b in range(4):
        valid = [j for j in range(K) if n[b, j] > 0]
        assert valid == [j for j in range(K) if not np.isnan(dist[b, j, j])]
        for j in valid:
            tot, others = 0.0, 0
            for i in valid:
                if i != j:
                    tot, others = tot + float(dist[b, j, i]), others + 1
            ref[b, j] = tot / others if others else 0.0
    assert np.array_equal(np.isnan(cost), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(_bits(cost[ok]), _bits(ref[ok]))
    assert cost[1, K - 1] == 0.0 and np.isnan(cost[2]).all() and pick.cpu().tolist()[1:3] == [K - 1, -1]
    if K >= 2:
        assert dist[3, 0, K - 1] == 0.0 and _bits(cost[3, :1]) == _bits(cost[3, K - 1:])


@pytest.mark.parametrize("K", [3, 16, 33])
def test_edge_radii(K):
    Tm, D = 7, 6
    gen, n, lab, refs, scores = _case(K, Tm, D)
    for with_n in (True, False):
        ng = n if with_n else None
        got = _run(gen, ng, scores, K, 0.0)                                              # radius 0, M = K: every non-duplicate, in score order
        modes, conf, assign, n_modes, n_nms, dist = got
        _check_rules(got, scores, K, 0.0)
        _check_invariants(got, K)
        nondup = []
        for b in range(4):
            order = sorted((j for j in range(K) if not np.isnan(dist[b, j, j])), key=lambda j: (-scores[b, j], j))
            if b == 3:                                                                   # of the two copies the lower-scored one is suppressed
                order.remove(max((1, K - 1), key=lambda j: (-scores[b, j], j)))
            nondup.append(len(order))
            assert modes[b, :n_modes[b]].tolist() == order and n_nms[b] == n_modes[b] == len(order)
        for M in (1, 6, 64):                                                             # a huge radius: one NMS mode, the fill does the rest
            got = _run(gen, ng, scores, M, 1e30)
            _check_rules(got, scores, M, 1e30)
            _check_invariants(got, M)
            for b in range(4):
                assert got[4][b] == (1 if nondup[b] else 0) and got[3][b] == min(M, nondup[b])
        for sc in (scores, None):
            assert not {1, K - 1} <= set(_run(gen, ng, sc, 64, 0.0)[0][3].tolist())      # the duplicate is never a second mode


def test_nan_and_neg_inf_scores_rank_last_in_index_order():
    K, Tm, D = 16, 7, 6
    gen, n, lab, refs, scores = _case(K, Tm, D)
    sc = scores.copy()
    sc[:, 9], sc[:, 2], sc[:, 5] = -np.inf, np.nan, -np.inf
    got = _run(gen, None, sc, K, 0.0)
    _check_rules(got, sc, K, 0.0)
    for b in range(3):                                                                   # (clip 3 holds the duplicate)
        assert got[3][b] == K and got[0][b, -3:].tolist() == [2, 5, 9]
        rest = [j for j in range(K) if j not in (2, 5, 9)]
        assert got[0][b, :-3].tolist() == sorted(rest, key=lambda j: (-scores[b, j], j))


def test_two_calls_give_identical_bits():
    gen, n, lab, refs, scores = _case(33, 25, 6)
    for sc in (scores, None):
        a, b = _run(gen, n, sc, 6, R.RADIUS), _run(gen, n, sc, 6, R.RADIUS)
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x) if x.dtype == np.float64 else x, _bits(y) if y.dtype == np.float64 else y)
    plain = T.select_modes(torch.tensor(gen).cuda(), torch.tensor(n).cuda(), None, 6, R.RADIUS)       # and without the dist output
    assert len(plain) == 5 and all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(plain, a))


def test_argument_checks_on_the_symbol_and_the_wrapper():
    fn = _lib.lib().egomi_traj_modes
    fn.restype = c_i
    dev = "cuda"
    gen = torch.zeros(2, 3, 4, 6, device=dev)
    dist = torch.zeros(2, 3, 3, dtype=torch.float64, device=dev)
    modes = torch.zeros(2, 64, dtype=torch.int32, device=dev)
    conf = torch.zeros(2, 64, dtype=torch.float64, device=dev)
    assign = torch.zeros(2, 3, dtype=torch.int32, device=dev)
    nm, nn = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)

    def call(g=gen, B=2, K=3, Tm=4, D=6, M=2, r=0.0, d=dist, mo=modes, co=conf, a=assign, x=nm, y=nn):
        return fn(P(g), P(None), P(None), c_i(B), c_i(K), c_i(Tm), c_i(D), c_i(M), c_d(r), P(d), P(mo), P(co), P(a), P(x), P(y), S())
    assert call() == 0 and call(d=None) == 0 and call(M=64) == 0 and call(r=0.0) == 0
    assert call(g=None) == -1 and call(mo=None) == -1 and call(co=None) == -1 and call(a=None) == -1 and call(x=None) == -1 and call(y=None) == -1
    assert call(r=float("nan")) == -1 and call(r=-1.0) == -1 and call(r=-1e-300) == -1
    assert call(B=0) == -2 and call(K=0) == -2 and call(Tm=0) == -2 and call(D=0) == -2 and call(M=0) == -2
    assert call(B=1, K=65) == -4 and call(M=65) == -4
    torch.cuda.synchronize()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    for bad in (lambda: T.select_modes(gen[0]), lambda: T.select_modes(torch.zeros(1, 65, 2, 3, device=dev)),
                lambda: T.select_modes(gen, num_modes=0), lambda: T.select_modes(gen, num_modes=65),
                lambda: T.select_modes(gen, n_gen=i32(2, 4)), lambda: T.select_modes(gen, scores=torch.zeros(3, 3, device=dev)),
                lambda: T.select_modes(gen, radius=float("nan")), lambda: T.select_modes(gen, radius=-0.5)):
        with pytest.raises(ValueError):
            bad()


def test_metrics_modes_is_metrics_best_of_on_the_gathered_rows():
    g = torch.Generator().manual_seed(11)
    B, K, Tm, D, M = 6, 7, 9, 6, 4
    gen = torch.randn(B, K, Tm, D, generator=g).cuda()
    gt = torch.randn(B, Tm, D, generator=g).cuda()
    n_gen = torch.randint(1, Tm + 1, (B, K), generator=g).to(torch.int32)
    n_gen[1, 2:] = 0                                                                     # two valid samples: two unused slots
    n_gen[2, :] = 0                                                                      # nothing left
    n_gen = n_gen.cuda()
    n_gt = torch.randint(1, Tm + 1, (B,), generator=g).to(torch.int32).cuda()
    scores = torch.randn(B, K, generator=g).cuda()
    for ng, nt, sc in ((n_gen, n_gt, None), (n_gen, None, scores), (None, None, None)):
        modes, conf, _, n_modes, _ = T.select_modes(gen, ng, sc, M, 0.0)
        ade, fde, slot, brier = T.metrics_modes(gen, ng, gt, nt, modes, conf)
        assert slot.dtype == torch.int32 and ade.dtype == fde.dtype == brier.dtype == torch.float64
        mh = modes.long()
        rows = torch.stack([gen[b, mh[b].clamp(min=0)] for b in range(B)])
        full = torch.full((B, K), Tm, dtype=torch.int32, device="cuda") if ng is None else ng
        nrows = torch.stack([torch.where(mh[b] >= 0, full[b, mh[b].clamp(min=0)], torch.zeros_like(full[b, :M])) for b in range(B)])
        ra, rf, rb = T.metrics_best_of(rows, nrows, gt, nt)
        same = lambda x, y: torch.equal(x.view(torch.int64), y.view(torch.int64))       # bit-equal, NaN included
        assert same(ade, ra) and same(fde, rf) and torch.equal(slot, rb)
        a, s, c = ade.cpu().numpy(), slot.cpu().numpy(), conf.cpu().numpy()
        want = np.array([a[b] + (1.0 - c[b, s[b]]) ** 2 if s[b] >= 0 else np.nan for b in range(B)])
        assert np.array_equal(brier.cpu().numpy(), want, equal_nan=True)
        if ng is not None:
            assert int(n_modes[1]) == 2 and s[1] in (0, 1) and s[2] == -1 and np.isnan(a[2]) and np.isnan(want[2])
        best_k = T.metrics_best_of(gen, ng, gt, nt)[0].cpu().numpy()                      # minADE_K <= minADE_M <= the ADE of the single pick
        one = T.metrics_selected(gen, ng, gt, nt, modes[:, 0].contiguous())[0].cpu().numpy()
        ok = s >= 0
        assert np.all(best_k[ok] <= a[ok]) and np.all(a[ok] <= one[ok]) and ok.sum() >= B - 1
        pick = T.select_medoid(gen, ng)[0] if sc is None else decode.seq_rank(sc.view(-1), (full > 0).to(torch.int32).view(-1), B, K, 0.0)[1][:, 0]
        assert torch.equal(modes[:, 0][torch.tensor(ok).cuda()], pick.contiguous()[torch.tensor(ok).cuda()])
