"""GPU: egomi_traj_metrics_full (csrc/traj_full.hip) through traj.metrics_full, against tests/traj_full_ref.py.

Bounds.  ADE, FDE, IDE: abs < 1e-12 (tests/test_gpu_traj.py's for metrics_batch).  DTW: |got - ref| <= 1e-12 (1 + ref): a value is a sum of
at most 511 float64 terms.  GD per row: the mean over the row's steps of 2 d / sqrt(max(1 - c^2, d)) + 1e-12 with d = 8e-15, c the
reference's clipped dot product: the condition number of acos times a few tens of ulps in the dot product (numpy's float64 against 80-bit
long double stays within 1.18x of the same formula at d = 8e-16 over 20 000 pairs on a CPU; the factor 10 is the margin for a second
implementation).  Every test prints the worst ratio error / bound it met per column."""
import numpy as np
import pytest
import torch

from tests import traj_full_ref as R

pytestmark = pytest.mark.gpu


def d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def run(gen, ng, gt, nt, rot0=3):
    from egoscaler_amd import traj as T
    return T.metrics_full(d(gen), None if ng is None else d(ng), d(gt), None if nt is None else d(nt), rot0=rot0)


def stacked(m):
    return torch.stack(list(m[:5]), -1)


def all_same_bits(m1, m2):
    return same_bits(stacked(m1), stacked(m2)) and same_bits(m1.mins, m2.mins) and torch.equal(m1.args, m2.args)


def check_against(m, ref, what, rot=True):
    """The five columns and the minima of one result against reference()'s; prints the worst error / bound per column."""
    vals, bound, mins, args = ref
    got, gmins, gargs = stacked(m).cpu().numpy(), m.mins.cpu().numpy(), m.args.cpu().numpy()
    assert got.shape == vals.shape and got.dtype == np.float64 and gmins.dtype == np.float64 and gargs.dtype == np.int32
    if not rot:
        vals, mins, args = vals.copy(), mins.copy(), args.copy()
        vals[..., 3], mins[:, 3], args[:, 3] = np.nan, np.nan, -1
    assert np.array_equal(np.isnan(got), np.isnan(vals)), what
    lim = np.empty_like(vals)
    lim[..., :3] = 1e-12
    lim[..., 3] = bound if rot else 1.0
    lim[..., 4] = 1e-12 * (1 + vals[..., 4])
    ok = ~np.isnan(vals)
    ratio = np.where(ok, np.abs(got - vals) / lim, 0.0)
    print(f"{what}: worst error / bound per column " + ", ".join(f"{c} {ratio[..., i].max():.3g}" for i, c in enumerate(R.COLS)))
    assert (ratio <= 1.0).all(), (what, ratio.max(axis=tuple(range(ratio.ndim - 1))))
    # the minima are minima of the kernel's own columns, taken at the reference's arg-minimum
    assert np.array_equal(gargs, args), (what, gargs, args)
    for b in range(len(args)):
        for c in range(5):
            if args[b, c] < 0:
                assert np.isnan(gmins[b, c])
            else:
                assert gmins[b, c] == got[b, args[b, c], c] == np.nanmin(got[b, :, c])


@pytest.fixture(scope="module")
def oracle_case():
    inp = R.oracle_inputs()
    return inp, R.reference(*inp)


def test_oracle_batch(oracle_case):
    (gen, ng, gt, nt), ref = oracle_case
    m = run(gen, ng, gt, nt)
    assert all(t.dtype == torch.float64 and tuple(t.shape) == ng.shape for t in m[:5])
    assert tuple(m.mins.shape) == tuple(m.args.shape) == (5, 5) and m.args.dtype == torch.int32
    assert m.ade._base is not None and tuple(m.ade._base.shape) == (5, 4, 5)                # views of the one [B, K, 5] tensor
    assert all(t._base is m.ade._base and t.data_ptr() == m.ade.data_ptr() + 8 * i for i, t in enumerate(m[:5]))
    check_against(m, ref, "oracle batch")
    args = m.args.cpu().numpy()
    assert (args[3] == -1).all() and torch.isnan(m.mins[3]).all()     # the clip with no parsed sample
    assert (args[4] == 0).all()                                       # the exact tie of samples 0 and 2, which is the best in every column
    assert set(args[2].tolist()) <= {1, 3}


def test_the_gd_cases_are_what_they_claim(oracle_case):
    (gen, ng, gt, nt), (vals, bound, _, _) = oracle_case
    c_same, c_neg, c_far = (R.clipped_dots(gen[1, j, :, 3:6].astype(np.float64), gt[1, :, 3:6].astype(np.float64)) for j in range(3))
    assert (c_same > 1 - 1e-15).all() and vals[1, 0, 3] < 1e-7                       # identical: the reference itself is about 3e-8 or 0
    assert (c_neg < 1).all() and vals[1, 1, 3] > 0.1                                # r, -r
    assert np.cos(4.0 / 2) < 0 and (c_far < 0).any() and (2 * np.arccos(c_far) > np.pi).any()      # negative w, angles above pi
    small = np.linalg.norm(np.concatenate([gt[0, :4, 3:6], gen[0, 0, :4, 3:6]]).astype(np.float64), axis=1)
    assert (small <= 1e-3).sum() >= 3 and (small > 1e-3).sum() >= 2 and ((small > 9e-4) & (small <= 1e-3)).any()


@pytest.mark.parametrize("case", R.SINGLE, ids=lambda c: "T{}_ng{}_nt{}_D{}".format(*c))
def test_single_clip_edges(case):
    inp = R.single_inputs(*case)
    check_against(run(*inp), R.reference(*inp), f"single {case}")


def test_more_samples_than_wavefronts():
    """K = 35 ragged samples of 2 clips: a wavefront of the clip's workgroup runs several samples one after the other."""
    g = np.random.default_rng(35)
    B, K, Tm = 2, 35, 5
    gen, gt = g.normal(size=(B, K, Tm, 6)).astype(np.float32), g.normal(size=(B, Tm, 6)).astype(np.float32)
    ng, nt = g.integers(0, Tm + 1, size=(B, K)).astype(np.int32), np.array([Tm, 3], dtype=np.int32)
    assert (ng == 0).any() and (ng == Tm).any()
    check_against(run(gen, ng, gt, nt), R.reference(gen, ng, gt, nt), "K = 35")


def test_ade_fde_and_minima_are_the_existing_kernels_bits(oracle_case):
    from egoscaler_amd import traj as T
    (gen, ng, gt, nt), _ = oracle_case
    B, K = ng.shape
    m = run(gen, ng, gt, nt)
    ade, fde = T.metrics_batch(d(gen.reshape(B * K, *gen.shape[2:])), d(ng.reshape(-1)), d(np.repeat(gt, K, axis=0)), d(np.repeat(nt, K)))
    keep = d(ng.reshape(-1) > 0)                                      # (an unparsed row is NaN on both sides)
    assert torch.equal(m.ade.reshape(-1)[keep], ade[keep]) and torch.equal(m.fde.reshape(-1)[keep], fde[keep])
    assert same_bits(m.ade.reshape(-1), ade) and same_bits(m.fde.reshape(-1), fde)
    made, mfde, best = T.metrics_best_of(d(gen), d(ng), d(gt), d(nt))
    assert same_bits(m.mins[:, 0], made) and same_bits(m.mins[:, 1], mfde) and torch.equal(m.args[:, 0], best)
    for case in R.SINGLE[3:6]:                                        # across the wavefront width too
        g1, n1, t1, nt1 = R.single_inputs(*case)
        m1 = run(g1, n1, t1, nt1)
        a1, f1 = T.metrics_batch(d(g1[:, 0]), d(n1[:, 0]), d(t1), d(nt1))
        assert same_bits(m1.ade[:, 0], a1) and same_bits(m1.fde[:, 0], f1)


def test_a_row_alone_is_bit_equal_to_the_row_in_the_batch(oracle_case):
    (gen, ng, gt, nt), _ = oracle_case
    whole = stacked(run(gen, ng, gt, nt))
    for b in range(ng.shape[0]):
        for j in range(ng.shape[1]):
            alone = stacked(run(gen[b:b + 1, j:j + 1], ng[b:b + 1, j:j + 1], gt[b:b + 1], nt[b:b + 1]))
            assert same_bits(alone[0, 0], whole[b, j]), (b, j)
    # a 3-d gen is K = 1, shaped like its leading dimension
    m3 = run(gen[:, 1], ng[:, 1], gt, nt)
    assert tuple(m3.dtw.shape) == (5,) and same_bits(stacked(m3), whole[:, 1])
    # strips of rows (ng > 64) beside short neighbours
    g1, n1, t1, nt1 = R.single_inputs(*R.SINGLE[4])
    g4 = np.concatenate([g1[:, :, ::-1].copy(), g1, g1 * 0.5, g1 + 1], axis=1)
    m4 = run(g4, np.array([[3, int(n1[0, 0]), 70, 0]], dtype=np.int32), t1, nt1)
    assert same_bits(stacked(m4)[0, 1], stacked(run(g1, n1, t1, nt1))[0, 0])


def test_replays_and_a_captured_graph_are_bit_equal(oracle_case):
    from egoscaler_amd import traj as T
    from egoscaler_amd.decode import _capture
    (gen, ng, gt, nt), _ = oracle_case
    a = [d(x) for x in (gen, ng, gt, nt)]
    first, second = T.metrics_full(*a), T.metrics_full(*a)
    assert all_same_bits(first, second)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        captured = T.metrics_full(*a)
    g.replay()
    torch.cuda.synchronize()
    assert all_same_bits(first, captured)
    g.replay()
    torch.cuda.synchronize()
    assert all_same_bits(first, captured)


def _poisoned(gen, ng, gt, nt):
    gen, gt = gen.copy(), gt.copy()
    for b in range(gen.shape[0]):
        gt[b, max(int(nt[b]), 0):] = np.nan
        for j in range(gen.shape[1]):
            gen[b, j, max(int(ng[b, j]), 0):] = np.nan
    return gen, ng, gt, nt


def test_nothing_beyond_the_lengths_is_read(oracle_case):
    inp, _ = oracle_case
    assert all_same_bits(run(*inp), run(*_poisoned(*inp)))
    for case in R.SINGLE:
        inp = R.single_inputs(*case)
        assert all_same_bits(run(*inp), run(*_poisoned(*inp))), case


def test_position_only_input(oracle_case):
    (gen, ng, gt, nt), ref = oracle_case
    m, off = run(gen, ng, gt, nt), run(gen, ng, gt, nt, rot0=-1)
    assert torch.isnan(off.gd).all() and torch.isnan(off.mins[:, 3]).all() and bool((off.args[:, 3] == -1).all())
    keep = [0, 1, 2, 4]
    assert same_bits(stacked(m)[..., keep], stacked(off)[..., keep]) and same_bits(m.mins[:, keep], off.mins[:, keep])
    assert torch.equal(m.args[:, keep], off.args[:, keep])
    assert torch.isnan(run(gen, ng, gt, nt, rot0=4).gd).all()         # rot0 + 3 > D
    pos, pgt = np.ascontiguousarray(gen[..., :3]), np.ascontiguousarray(gt[..., :3])
    check_against(run(pos, ng, pgt, nt, rot0=-1), R.reference(pos, ng, pgt, nt, rot0=-1), "positions only", rot=False)


def test_no_lengths_means_full_length(oracle_case):
    (gen, ng, gt, nt), _ = oracle_case
    full_g, full_t = np.full_like(ng, gen.shape[2]), np.full_like(nt, gen.shape[2])
    assert all_same_bits(run(gen, None, gt, None), run(gen, full_g, gt, full_t))
    assert all_same_bits(run(gen, full_g + 7, gt, full_t + 1), run(gen, full_g, gt, full_t))      # lengths above T count as T


def test_refusals():
    from egoscaler_amd import traj as T
    from egoscaler_amd._lib import EgomiError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError):
        T.metrics_full(z(1, 1, 257, 6), None, z(1, 257, 6))
    with pytest.raises(EgomiError, match="shape"):
        T.metrics_full(z(1, 1, 4, 65), None, z(1, 4, 65))
    with pytest.raises(ValueError):
        T.metrics_full(z(2, 3, 4, 6), None, z(2, 5, 6))
    with pytest.raises(ValueError):
        T.metrics_full(z(2, 3, 4, 6), torch.zeros(2, 2, dtype=torch.int32, device="cuda"), z(2, 4, 6))
