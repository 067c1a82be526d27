"""CPU: the bound tests/test_gpu_logprob_kernel.py holds egomi_token_logprob to (tests/logprob_cases.py BOUND) means something: three
plausible kernel defects, applied to the float64 reference on the same rows, each miss it by more than 100x.
  * tail dropped : the last V % 1024 columns never reach the sum (a loop over whole passes of the 1024-thread workgroup)
  * processed row: the log-softmax of HF's processed top-k 50 scores in place of the raw row (what `scores` would give)
  * early max    : the maximum taken over the first 1024 columns only (one pass); simulated in fp32 like the kernel's arithmetic, because
                   in exact arithmetic a wrong shift cancels: it shows when exp(x - m) overflows
and the reference itself sits far inside the bound when evaluated in fp32 the plain way (so the bound is not merely out of reach)."""
import numpy as np
import pytest
import torch

from tests import logprob_cases as C

R = 130


def _rows(V, dtype=torch.float32):
    x, tok = C.make_rows(R, V, dtype)
    return C.received(x), tok.numpy()


def _lp(x, tok, cols_sum=None, m=None, f=np.float64):
    """(x[tok] - m) - log sum_{cols_sum} exp(x - m) in precision f."""
    x = x.astype(f)
    m = x.max(1) if m is None else m.astype(f)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(x - m[:, None])
        s = (e if cols_sum is None else e[:, cols_sum]).sum(1, dtype=f)
        return (x[np.arange(len(tok)), tok] - m) - np.log(s)


def test_reference_restated_in_fp32_is_inside_the_bound():
    for V in C.VS:
        x, tok = _rows(V)
        assert C.ratio(_lp(x, tok, f=np.float64), C.ref_logprob(x, tok)) < 1e-12
    assert 0 < C.MEASURED < C.BOUND == 4 * C.MEASURED < 1e-5


@pytest.mark.parametrize("V", [v for v in C.VS if v > 1024 and v % 1024])
def test_dropped_tail_columns_exceed_the_bound(V):
    x, tok = _rows(V)
    bad = _lp(x, tok, cols_sum=slice(0, V - V % 1024))
    assert C.ratio(bad, C.ref_logprob(x, tok)) > 100 * C.BOUND


@pytest.mark.parametrize("V", [v for v in C.VS if v > 50])
def test_processed_topk_scores_exceed_the_bound(V):
    x, tok = _rows(V)
    kth = np.sort(x, 1)[:, -50][:, None]
    proc = np.where(x < kth, -np.inf, x)                                 # TopKLogitsWarper: scores < kth removed
    with np.errstate(invalid="ignore"):
        bad = C.ref_logprob(proc, tok)                                    # -inf where the token was removed
    assert C.ratio(bad, C.ref_logprob(x, tok)) > 100 * C.BOUND
    kinds = [C.KINDS[r % len(C.KINDS)] for r in range(R)]
    g = [r for r, k in enumerate(kinds) if k == "gauss"]                 # also on the plain rows alone
    assert C.ratio(bad[g], C.ref_logprob(x, tok)[g]) > 100 * C.BOUND


@pytest.mark.parametrize("V", [v for v in C.VS if v > 1024])
def test_max_over_first_pass_only_exceeds_the_bound(V):
    x, tok = _rows(V)
    bad = _lp(x, tok, m=x[:, :1024].max(1), f=np.float32)
    assert C.ratio(bad, C.ref_logprob(x, tok)) > 100 * C.BOUND
    good = _lp(x, tok, f=np.float32)                                     # the same fp32 arithmetic with the right maximum: no such miss
    assert C.ratio(good, C.ref_logprob(x, tok)) < 100 * C.BOUND
