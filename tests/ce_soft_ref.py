"""Shared by tests/test_ce_soft_host.py (CPU), tests/test_gpu_ce_soft_kernel.py and tests/test_gpu_ce_soft_train.py (GPU): the float64 statement
of the bin-aware cross-entropy (include/egomi.h, egomi_ce_soft_fwd_bwd) and the bounds the kernel is held to.  Not a test file; numpy and
torch-CPU only.

The target.  A spec is (p0, nb, sigma, W).  A kept row with target t, p0 <= t < p0 + nb, i = t - p0, lo = max(0, i - W), hi = min(nb - 1, i + W):
    w_j = exp(-(j - i)^2 / (2 sigma^2)) for lo <= j <= hi,  Z = sum w_j (j ascending),  q[p0 + j] = w_j / Z,  0 elsewhere
(truncation at either end of the bin window renormalises; no mass leaves it; nb = 1 is the one-hot).  Any other kept t: the one-hot.
Ignored rows (t == ignore, t < 0, t >= V): loss 0 and a zero gradient row.
    row_loss = sum_j q_j (lse - x_j) over the ids with q_j > 0, j ascending      row_nll = lse - x_t
    dlogits_c = (p_c - q_c) sc,  p_c = exp(x_c - lse),  sc = grad_scale / count
A -inf logit under a positive q_j gives +inf; the gradient there is -q_c sc.

The bounds (derived, not measured on the kernel under test):
  * row_loss, row_nll:  |got - ref| <= BOUND (1 + |ref|), BOUND = tests/logprob_cases.py's: m and s are egomi_token_logprob's own code, whose
    measured error set that bound; the float64 dot product of at most 65 terms adds 65 * 2^-53.  Where the reference is inf: equality.
  * gradient, per element:  [BOUND (1 + |x_c - lse|) + 2^-23] p_c sc + 3 * 2^-24 (p_c + q_c) sc  (+ 2^-8 |ref| for a bf16 output) + the
    smallest normal fp32.  Term by term: the relative error of p from the error in log s and x - m; one expf; q rounded once from float64, one
    subtraction and one product; one rounding to bf16.  That last term is 2^-8, not 2^-9: bf16 keeps 8 significant bits, so a value in
    [2^e, 2^(e+1)) sits within half a spacing 2^(e-8) of its rounding, up to 2^-8 of the value itself (fp32 with 24 bits: 2^-24, as used
    above).  With 2^-9 a kernel whose fp32 value is exact to the last bit misses the bound by a factor 2 on the elements that round worst.
    The three 2^-24 terms hold only because the kernel forms no fp32 sc: grad_scale / count is a fourth fp32 rounding, and where p ~ 0
    (error q sc (1 + 1 + 1) 2^-24 from q, the quotient and the product) it takes the whole allowance.  The kernel keeps q, p - q and sc in
    float64 and rounds once.
  * loss_sum, nll_sum against the float64 sum of the kernel's own fp32 rows: ordered_sum_kernel's tree, (R / 1024 + 12) 2^-24 sum |row|.
tests/test_ce_soft_host.py shows the two per-row bounds have teeth: three plausible defects (DEFECTS) miss each by more than 100x."""
import math

import numpy as np
import torch

from tests.logprob_cases import BOUND

TINY = float(np.finfo(np.float32).tiny)
DEFECTS = ("no_renorm", "off_by_one", "spill")


def default_radius(sigma):
    return min(32, int(math.ceil(3.0 * float(sigma))))


def window(t, p0, nb, sigma, W, defect=None):
    """-> (ids, q): the ids with q > 0 possible, ascending, and their float64 weights.  t must be a kept target.
    defect (for the teeth tests only): "no_renorm" Z is the untruncated window's; "off_by_one" the window is centred one bin up;
    "spill" the lower clip lets one id below p0 in."""
    t = int(t)
    if not p0 <= t < p0 + nb:
        return np.array([t], dtype=np.int64), np.array([1.0])
    i = t - p0
    c = i + 1 if defect == "off_by_one" else i
    lo, hi = max(-1 if defect == "spill" else 0, c - W), min(nb - 1, c + W)
    j = np.arange(lo, hi + 1)
    w = np.exp(-((j - c).astype(np.float64) ** 2) / (2.0 * float(sigma) ** 2))
    if defect == "no_renorm":
        jj = np.arange(c - W, c + W + 1)
        Z = float(np.cumsum(np.exp(-((jj - c).astype(np.float64) ** 2) / (2.0 * float(sigma) ** 2)))[-1])
    else:
        Z = float(np.cumsum(w)[-1])                                       # j ascending
    return (p0 + j).astype(np.int64), w / Z


def kept(targets, V, ignore):
    t = np.asarray(targets, dtype=np.int64)
    return (t != ignore) & (t >= 0) & (t < V)


def target_q(targets, V, ignore, spec, defect=None):
    """Dense q float64 [R, V]; zero rows for ignored targets."""
    p0, nb, sigma, W = spec
    t = np.asarray(targets, dtype=np.int64)
    q = np.zeros((len(t), V))
    for r in np.nonzero(kept(t, V, ignore))[0]:
        ids, w = window(t[r], p0, nb, sigma, W, defect)
        q[r, ids] = w
    return q


def soft_ce(x64, targets, ignore, spec, grad_scale=1.0, count=None, defect=None):
    """x64 float64 [R, V] (the values the kernel receives) -> dict of float64 arrays: row_loss [R], row_nll [R], grad [R, V], p, q [R, V],
    lse [R], and count, sc.  count defaults to the number of targets != ignore (egomi_ce_count's)."""
    x64 = np.asarray(x64, dtype=np.float64)
    R, V = x64.shape
    p0, nb, sigma, W = spec
    t = np.asarray(targets, dtype=np.int64)
    keep = kept(t, V, ignore)
    count = int((t != ignore).sum()) if count is None else int(count)
    sc = float(np.float32(grad_scale)) / count if count else float("nan")
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = x64.max(1)
        lse = m + np.log(np.exp(x64 - m[:, None]).sum(1))
        p = np.exp(x64 - lse[:, None])
    q = np.zeros((R, V))
    row_loss, row_nll = np.zeros(R), np.zeros(R)
    for r in np.nonzero(keep)[0]:
        ids, w = window(t[r], p0, nb, sigma, W, defect)
        q[r, ids] = w
        acc = 0.0
        for c, qc in zip(ids, w):                                         # j ascending, only where q > 0
            if qc > 0.0:
                acc += qc * (lse[r] - x64[r, c])
        row_loss[r] = acc
        row_nll[r] = lse[r] - x64[r, t[r]]
    grad = (p - q) * sc
    grad[~keep] = 0.0
    p[~keep] = 0.0
    return dict(row_loss=row_loss, row_nll=row_nll, grad=grad, p=p, q=q, lse=lse, count=count, sc=sc, keep=keep)


# -- the bounds ------------------------------------------------------------------------------------------------------------------------
def loss_ratio(got, ref):
    """worst |got - ref| / (BOUND (1 + |ref|)) over the rows; where ref is inf (or NaN) got must be the same, else inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    same = np.where(np.isnan(ref), np.isnan(got), got == ref)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / (BOUND * (1.0 + np.abs(ref)))
    e = np.where(fin, np.where(np.isfinite(got), e, np.inf), np.where(same, 0.0, np.inf))
    return float(e.max()) if e.size else 0.0


def grad_bound(x64, ref, bf16_out):
    """Per element, float64 [R, V]: see the module comment.  `ref` is soft_ce's dict."""
    p, q, sc = ref["p"], ref["q"], abs(ref["sc"])
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(x64, dtype=np.float64) - ref["lse"][:, None])
        rel = np.where(p > 0.0, BOUND * (1.0 + d) + 2.0 ** -23, 0.0)       # p = 0 (a -inf logit): expf gives 0 exactly
    b = rel * p * sc + 3.0 * 2.0 ** -24 * (p + q) * sc + TINY
    if bf16_out:
        b = b + 2.0 ** -8 * np.abs(ref["grad"])
    return b


def grad_ratio(got, x64, ref, bf16_out):
    """worst |got - ref| / bound over every element of every row (inf where got is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref["grad"]) / grad_bound(x64, ref, bf16_out)
    e = np.where(np.isfinite(got), e, np.inf)
    return float(e.max())


def sum_bound(rows):
    rows = np.asarray(rows, dtype=np.float64)
    return (len(rows) / 1024.0 + 12.0) * 2.0 ** -24 * float(np.abs(rows).sum())


# -- the same loss for autograd ----------------------------------------------------------------------------------------------------------
def torch_soft_ce(logits, targets, ignore, spec):
    """Mean soft cross-entropy of `logits` [R, V] (any float dtype, may require grad) in float64, and the mean hard loss of the same rows."""
    R, V = logits.shape
    t = targets.detach().cpu().numpy()
    q = torch.from_numpy(target_q(t, V, ignore, spec)).to(logits.device)
    lp = torch.log_softmax(logits.to(torch.float64), dim=1)
    n = int((t != ignore).sum())
    soft = -(torch.where(q > 0, q * lp, torch.zeros_like(lp))).sum() / n
    hard = torch.nn.functional.cross_entropy(logits.to(torch.float64), targets, ignore_index=ignore, reduction="sum") / n
    return soft, hard
