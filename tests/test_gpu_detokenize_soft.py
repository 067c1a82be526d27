"""GPU: traj.detokenize_soft (egomi_traj_detokenize_soft, csrc/traj.hip) against traj.detokenize_batch on the same ids.
  * with bin_mean[b, j] = float32(values[ids[b, j] - p0]) on the bin positions the soft mean is detokenize_batch's output bit for bit and
    n_steps is equal: rows with a missing step (copy-forward), a leading broken segment, an eos mid-row, no eos, text between the bins;
    B in {1, 65}
  * std and mass gather as specified: a numpy restatement of the scan below."""
import numpy as np
import pytest
import torch

from egoscaler_amd import traj as T
from egoscaler_amd.config import dims_7b, dims_tiny

pytestmark = pytest.mark.gpu
TMAX = 9


def _rows(tok, B, L, seed=0):
    """B rows of L ids: row b cycles through five shapes; bins drawn at random, padding after the eos is noise that must not be read."""
    g = np.random.default_rng(seed)
    text = 3                                                             # an id that is neither a bin nor a separator
    rows = []
    for b in range(B):
        step = lambda: list(tok.p0 + g.integers(0, tok.num_bins, 6))
        kind = b % 5
        if kind == 0:                                                    # four plain steps, then eos
            r = sum((step() + [tok.tsep] for _ in range(4)), []) + [tok.te, tok.eos]
        elif kind == 1:                                                  # the second segment holds five bins only: copied forward
            r = step() + [tok.tsep] + step()[:5] + [tok.tsep] + step() + [tok.tsep, tok.eos]
        elif kind == 2:                                                  # a leading broken segment (nothing to copy yet), text inside a segment
            r = step()[:3] + [text] + step()[:2] + [tok.tsep] + [text] + step() + [tok.tsep] + step() + [tok.tsep, tok.eos]
        elif kind == 3:                                                  # an eos in the middle of a step: the rest is not read
            r = step() + [tok.tsep] + step()[:2] + [tok.eos] + step() + [tok.tsep] + step()
        else:                                                            # no eos at all, more steps than TMAX
            r = sum((step() + [tok.tsep] for _ in range(L // 7)), [])
        r = (r + list(g.integers(0, tok.p0 + tok.num_bins, L)))[:L] if kind != 4 else (r + [tok.tsep] * L)[:L]
        rows.append(r)
    return torch.tensor(np.array(rows, dtype=np.int64))


def _scan(ids, tok, bin_mean, bin_std, bin_mass, tmax):
    """The scan restated: per row cut at the first eos, split on <tsep>, first run of six bin ids per segment, copy-forward."""
    B = ids.shape[0]
    mean, std, mass, n = np.zeros((B, tmax, 6), np.float32), np.zeros((B, tmax, 6), np.float32), np.zeros((B, tmax), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        r = list(ids[b])
        r = r[:r.index(tok.eos)] if tok.eos in r else r
        last, j0 = None, 0
        for seg_end in [j for j, t in enumerate(r) if t == tok.tsep] + [len(r)]:
            run, hit = 0, None
            for j in range(j0, seg_end):
                run = run + 1 if tok.p0 <= r[j] < tok.p0 + tok.num_bins else 0
                if run == 6:
                    hit = j - 5
                    break
            if hit is not None:
                last = (bin_mean[b, hit:hit + 6], bin_std[b, hit:hit + 6], bin_mass[b, hit:hit + 6].min())
            if last is not None and n[b] < tmax:
                mean[b, n[b]], std[b, n[b]], mass[b, n[b]] = last
                n[b] += 1
            j0 = seg_end + 1
    return mean, std, mass, n


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("dims", [dims_tiny, dims_7b], ids=["tiny", "7b"])
def test_one_hot_statistics_give_the_hard_trajectory_and_the_rest_gathers(dims, B):
    tok, L = dims().tok, 44
    ids = _rows(tok, B, L, seed=B).cuda()
    hard, n_hard = T.detokenize_batch(ids, tok, TMAX)
    values = T.bin_edges(tok.num_bins, "cuda")
    isbin = (ids >= tok.p0) & (ids < tok.p0 + tok.num_bins)
    g = torch.Generator().manual_seed(B)
    noise = lambda: torch.rand(B, L + 3, generator=g).cuda()             # the statistics may be wider than the ids
    bin_mean = noise()
    bin_mean[:, :L] = torch.where(isbin, values[(ids - tok.p0).clamp(0, tok.num_bins - 1)].float(), bin_mean[:, :L])
    bin_std, bin_mass = noise(), noise()
    mean, std, mass, n = T.detokenize_soft(ids, tok, TMAX, bin_mean, bin_std, bin_mass)
    assert mean.shape == (B, TMAX, 6) and std.shape == (B, TMAX, 6) and mass.shape == (B, TMAX) and n.dtype == torch.int32
    assert torch.equal(n, n_hard) and torch.equal(mean, hard)
    if B > 4:
        # every row's tail segment (<te>, or nothing after the last <tsep>) repeats the last step; the broken head yields none; row 4 fills TMAX
        assert n.tolist()[:5] == [5, 4, 3, 2, TMAX]
    rm, rs, rmass, rn = _scan(ids.cpu().numpy(), tok, bin_mean.cpu().numpy(), bin_std.cpu().numpy(), bin_mass.cpu().numpy(), TMAX)
    assert np.array_equal(n.cpu().numpy(), rn)
    assert np.array_equal(mean.cpu().numpy(), rm) and np.array_equal(std.cpu().numpy(), rs) and np.array_equal(mass.cpu().numpy(), rmass)
    m2, s2, none, n2 = T.detokenize_soft(ids, tok, TMAX, bin_mean, bin_std)
    assert none is None and torch.equal(m2, mean) and torch.equal(s2, std) and torch.equal(n2, n)


def test_hard_and_soft_scan_agree_on_the_edge_rows():
    """Both kernels are one scan (csrc/traj.hip: traj_scan): a row with no eos, a row whose first id is the eos, and a row whose first
    segment has no run of six bin ids (copy-forward with nothing to copy yet).  L = 20, Tmax = 4."""
    tok, L, tmax, text = dims_tiny().tok, 20, 4, 3
    g = np.random.default_rng(20)
    step = lambda: list(tok.p0 + g.integers(0, tok.num_bins, 6))
    noise = lambda k: list(g.integers(0, tok.p0 + tok.num_bins, k))
    rows = [step() + [tok.tsep] + step() + [tok.tsep] + step()[:5] + [text],                      # no eos: the row's end closes a broken segment
            [tok.eos] + noise(L - 1),                                                               # eos first: nothing is read
            step()[:3] + [text] + step()[:2] + [tok.tsep] + step() + [tok.tsep, tok.te, tok.eos] + noise(4)]
    rows[0] = [t if t != tok.eos else text for t in rows[0]]
    assert all(len(r) == L for r in rows)
    ids = torch.tensor(np.array(rows, dtype=np.int64)).cuda()
    hard, n_hard = T.detokenize_batch(ids, tok, tmax)
    values = T.bin_edges(tok.num_bins, "cuda")
    isbin = (ids >= tok.p0) & (ids < tok.p0 + tok.num_bins)
    tg = torch.Generator().manual_seed(20)
    bin_mean, bin_std, bin_mass = (torch.rand(3, L, generator=tg).cuda() for _ in range(3))
    bin_mean = torch.where(isbin, values[(ids - tok.p0).clamp(0, tok.num_bins - 1)].float(), bin_mean)
    mean, std, mass, n = T.detokenize_soft(ids, tok, tmax, bin_mean, bin_std, bin_mass)
    assert torch.equal(n, n_hard) and torch.equal(mean, hard)
    assert n.tolist() == [3, 0, 2]
    rm, rs, rmass, rn = _scan(ids.cpu().numpy(), tok, bin_mean.cpu().numpy(), bin_std.cpu().numpy(), bin_mass.cpu().numpy(), tmax)
    assert np.array_equal(n.cpu().numpy(), rn)
    assert np.array_equal(mean.cpu().numpy(), rm) and np.array_equal(std.cpu().numpy(), rs) and np.array_equal(mass.cpu().numpy(), rmass)


def test_rejected_inputs():
    tok = dims_tiny().tok
    ids = _rows(tok, 2, 20).cuda()
    ok = torch.zeros(2, 20, device="cuda")
    with pytest.raises(ValueError):
        T.detokenize_soft(ids, tok, TMAX, ok[:, :19], ok)                # fewer columns than ids
    with pytest.raises(ValueError):
        T.detokenize_soft(ids, tok, TMAX, ok, ok[:1])
