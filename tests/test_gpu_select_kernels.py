"""GPU: the two per-clip selection kernels, against numpy restatements written here.
  * egomi_seq_rank (csrc/logprob.hip): score = sum_lp / n_tok ** length_penalty in fp32 (n_tok = 0: -inf), order = the clip's indices by
    descending score, ties to the lower index, empty rows last in index order (np.argsort of (-score, index), stable).
  * egomi_traj_medoid (csrc/traj.hip): float64 mean pairwise displacement with each sample padded by its own last step, < 1e-12 (the bar of
    tests/test_gpu_traj_best_of.py); traj.select_medoid / traj.metrics_selected on top of it."""
import ctypes

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib, decode, traj as T
from egoscaler_amd.ops import P, S

pytestmark = pytest.mark.gpu
c_i, c_f = ctypes.c_int, ctypes.c_float
TOL = 1e-12


# ------------------------------------------------------------------------------------------------ seq_rank
def rank_ref(sum_lp, n_tok, lp):
    """numpy restatement: (score fp32 [B, K], order [B, K])."""
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(n_tok > 0, sum_lp.astype(np.float32) / np.power(n_tok.astype(np.float32), np.float32(lp)), -np.inf).astype(np.float32)
    return score, order_of(score)


def order_of(score):
    B, K = score.shape
    return np.stack([np.lexsort((np.arange(K), -score[b].astype(np.float64))) for b in range(B)]).astype(np.int32)


def _rank_inputs(K, seed):
    g = np.random.default_rng(seed)
    B = 3
    n = g.integers(1, 40, (B, K)).astype(np.int32)
    s = (-g.random((B, K)) * 3 * n).astype(np.float32)
    if K >= 2:
        s[0, K - 1], n[0, K - 1] = s[0, 0], n[0, 0]                    # an exact tie, first against last
        n[0, K // 2] = 0                                               # an empty row among full ones (K = 2: it is row 1, the tie's partner)
    if K >= 5:
        s[1, 1:4], n[1, 1:4] = s[1, 4], n[1, 4]                        # four equal rows
        n[1, 0] = 0
    n[2, :] = 0                                                        # a clip whose rows are all empty
    return s, n


@pytest.mark.parametrize("K", [1, 2, 5, 32, 1024])
@pytest.mark.parametrize("lp", [0.0, 1.0, 0.7])
def test_seq_rank_against_numpy(K, lp):
    s, n = _rank_inputs(K, 11 * K)
    score, order = decode.seq_rank(torch.from_numpy(s).cuda().view(-1), torch.from_numpy(n).cuda().view(-1), 3, K, lp)
    score, order = score.cpu().numpy(), order.cpu().numpy()
    ref_score, ref_order = rank_ref(s, n, lp)
    fin = np.isfinite(ref_score)
    assert np.array_equal(np.isneginf(score), np.isneginf(ref_score)) and not np.isnan(score).any()
    # fp32 rounding of the restated formula: the division is correctly rounded, powf is within 2 ulp on either side
    assert np.all(np.abs(score[fin] - ref_score[fin]) <= 4 * np.spacing(np.abs(ref_score[fin])))
    assert np.array_equal(order, order_of(score))                      # the ranking rule, exactly, on the scores returned
    if lp in (0.0, 1.0):                                                # n ** 0 and n ** 1 are exact: the same scores, the same order
        assert np.array_equal(score, ref_score) and np.array_equal(order, ref_order)
    for b in range(3):
        assert sorted(order[b].tolist()) == list(range(K))
    assert order[2].tolist() == list(range(K))                         # all empty: index order
    if K >= 2:
        o = order[0].tolist()
        assert o.index(0) < o.index(K - 1) or n[0, 0] == 0             # the tie goes to the lower index
        assert o[-1] == max(j for j in range(K) if n[0, j] == 0)       # empty rows come last


def test_seq_rank_argument_checks():
    fn = _lib.lib().egomi_seq_rank
    fn.restype = c_i
    s = torch.zeros(8, dtype=torch.float32, device="cuda")
    n = torch.ones(8, dtype=torch.int32, device="cuda")
    sc, od = torch.zeros(8, dtype=torch.float32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    call = lambda a=s, b=n, B=2, K=4, lp=1.0, c=sc, d=od: fn(P(a), P(b), c_i(B), c_i(K), c_f(lp), P(c), P(d), S())
    assert call() == 0
    assert call(a=None) == -1 and call(b=None) == -1 and call(c=None) == -1 and call(d=None) == -1 and call(lp=float("nan")) == -1
    assert call(B=0) == -2 and call(K=0) == -2
    assert call(B=1, K=1025) == -4
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ medoid
def medoid_ref(gen, n_gen):
    """float64 numpy restatement: (cost [B, K], pick [B])."""
    B, K, Tm, D = gen.shape
    g = gen.astype(np.float64)
    n = np.full((B, K), Tm) if n_gen is None else n_gen
    cost, pick = np.full((B, K), np.nan), np.full(B, -1, dtype=np.int32)

    def padded(b, j, L):
        return g[b, j][np.minimum(np.arange(L), n[b, j] - 1)]
    for b in range(B):
        valid = [j for j in range(K) if n[b, j] > 0]
        for j in valid:
            d = []
            for i in valid:
                if i != j:
                    L = max(n[b, j], n[b, i])
                    d.append(np.sqrt(((padded(b, j, L) - padded(b, i, L)) ** 2).sum(1)).mean())
            cost[b, j] = float(sum(d) / len(d)) if d else 0.0                # index order
        if valid:
            pick[b] = min(valid, key=lambda j: (cost[b, j], j))
    return cost, pick


def _medoid_inputs(K, Tm, D, seed):
    g = np.random.default_rng(seed)
    B = 4
    gen = g.normal(0, 1, (B, K, Tm, D)).astype(np.float32)
    n = g.integers(0, Tm + 1, (B, K)).astype(np.int32)                 # ragged, 0 and Tmax included
    n[0, 0] = Tm
    n[1, :] = 0
    n[1, K - 1] = max(1, Tm // 2)                                      # a clip with one valid sample
    n[2, :] = 0                                                        # a clip with none
    if K >= 3:                                                         # two identical samples that are the medoid: far copies around them
        n[3, :] = Tm
        gen[3] = 50.0 + gen[3]
        gen[3, 1] = gen[3, K - 1] = 50.0
    return gen, n


@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("Tm", [1, 7, 25])
@pytest.mark.parametrize("K", [1, 2, 3, 16, 32])
def test_medoid_against_float64_numpy(K, Tm, D):
    gen, n = _medoid_inputs(K, Tm, D, 100 * K + 10 * Tm + D)
    for n_gen in (n, None):                                            # None = every sample Tmax long
        pick, cost = T.select_medoid(torch.from_numpy(gen).cuda(), None if n_gen is None else torch.from_numpy(n_gen).cuda())
        pick, cost = pick.cpu().numpy(), cost.cpu().numpy()
        ref_cost, ref_pick = medoid_ref(gen, n_gen)
        assert np.array_equal(np.isnan(cost), np.isnan(ref_cost))
        ok = ~np.isnan(ref_cost)
        assert np.all(np.abs(cost[ok] - ref_cost[ok]) < TOL)
        for b in range(4):                                             # the arg-min rule on the costs returned (a last-bit difference cannot move it)
            v = [j for j in range(K) if not np.isnan(cost[b, j])]
            assert pick[b] == (min(v, key=lambda j: (cost[b, j], j)) if v else -1)
        if n_gen is not None:
            assert pick[1] == K - 1 and cost[1, K - 1] == 0.0          # one valid sample: itself, at cost 0
            assert pick[2] == -1 and np.isnan(cost[2]).all()
            if K >= 3:
                assert cost[3, 1] == cost[3, K - 1] and pick[3] == 1 == ref_pick[3]     # identical samples: the lower index
        assert np.array_equal(pick, ref_pick) or K < 3                 # (K < 3: every cost of a clip ties mathematically)


def test_medoid_argument_checks_and_shapes():
    fn = _lib.lib().egomi_traj_medoid
    fn.restype = c_i
    gen = torch.zeros(2, 3, 4, 6, device="cuda")
    cost = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    pick = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda g=gen, B=2, K=3, Tm=4, D=6, c=cost, p=pick: fn(P(g), P(None), c_i(B), c_i(K), c_i(Tm), c_i(D), P(c), P(p), S())
    assert call() == 0
    assert call(g=None) == -1 and call(c=None) == -1 and call(p=None) == -1
    assert call(B=0) == -2 and call(K=0) == -2 and call(Tm=0) == -2 and call(D=0) == -2
    assert call(B=1, K=1025) == -4
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        T.select_medoid(gen[0])
    with pytest.raises(ValueError):
        T.select_medoid(gen, torch.zeros(2, 4, dtype=torch.int32, device="cuda"))


def test_metrics_selected_is_metrics_batch_on_the_gathered_rows():
    g = torch.Generator().manual_seed(5)
    B, K, Tm, D = 5, 4, 9, 6
    gen = torch.randn(B, K, Tm, D, generator=g).cuda()
    gt = torch.randn(B, Tm, D, generator=g).cuda()
    n_gen = torch.randint(1, Tm + 1, (B, K), generator=g).to(torch.int32).cuda()
    n_gt = torch.randint(1, Tm + 1, (B,), generator=g).to(torch.int32).cuda()
    pick = torch.tensor([3, 0, -1, 2, 1], dtype=torch.int32).cuda()
    for ng, nt in ((n_gen, n_gt), (None, None)):
        ade, fde = T.metrics_selected(gen, ng, gt, nt, pick)
        rows = torch.tensor([0, 1, 3, 4], device="cuda")
        pk = pick.long()[rows]
        ra, rf = T.metrics_batch(gen[rows, pk], None if ng is None else ng[rows, pk], gt[rows], None if nt is None else nt[rows])
        assert torch.equal(ade[rows], ra) and torch.equal(fde[rows], rf)
        assert bool(torch.isnan(ade[2])) and bool(torch.isnan(fde[2]))
    mp, cost = T.select_medoid(gen, n_gen)                             # and end to end: the medoid's metrics
    ade, _ = T.metrics_selected(gen, n_gen, gt, n_gt, mp)
    made, _, _ = T.metrics_best_of(gen, n_gen, gt, n_gt)
    assert bool((made <= ade).all())
