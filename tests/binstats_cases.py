"""Shared by tests/test_gpu_binstats_kernel.py (GPU) and tests/test_binstats_host.py (CPU): the rows egomi_bin_stats is pinned on, its
float64 reference, and the bounds.  Not a test file; numpy / torch-CPU only.

The reference is the four statistics in float64 of the values the kernel receives (the bf16 rows after their rounding) and of
values = numpy.linspace(-1, 1, nb):  m = max x, s = sum exp(x - m), w_i = exp(x[p0 + i] - m), Z = sum w_i, q_i = w_i / Z,
    mass = Z / s,  mean = sum q_i v_i,  std = sqrt(sum q_i (v_i - mean)^2),  ent = -sum q_i log q_i  (0 log 0 = 0).
A case passes when  |got - ref| <= BOUND[name] * (1 + |ref|)  on every row, for each of the four outputs (where the reference is NaN --
every bin -inf -- the kernel must give NaN).  std of a row with all its mass on one bin has ref = 0: the same expression is then the
absolute comparison against 0.

MEASURED on the MI355X over every case of tests/test_gpu_binstats_kernel.py (bf16 and fp32, the (V, nb, p0, R) of cases(), both strides,
the rows of KINDS), worst |got - ref| / (1 + |ref|) per output, with the case that produced it:
    mass  MEASURED = 1.907e-07   (bf16, V = 32262, nb = 1024, p0 = 0, R = 1, the `peak` row)
    mean  MEASURED = 4.261e-07   (fp32, V = 32262, nb = 3, p0 = 32259, R = 3, rows equal / outside / inf_out)
    std   MEASURED = 1.132e-07   (fp32, V = 5, nb = 3, p0 = 2, R = 130)
    ent   MEASURED = 2.504e-07   (fp32, V = 40003, nb = 1024, p0 = 38979, R = 3, rows equal / outside / inf_out)
    BOUND = 4 x MEASURED per output (the convention of tests/logprob_cases.py: room for another box's expf)
The bf16 cases stay under 2.4e-08 (mean), 2.1e-08 (std) and 4.6e-08 (ent): their x_i - m is exact.
What the error is made of: w_i = expf(x_i - m) carries the rounding of x_i - m in fp32 (up to 2^-24 |x_i - m|, i.e. 5e-6 relative in w_i for
a logit 80 below the maximum; exact for bf16 inputs of nearby exponents) plus expf's own ulp; the sums over the nb bins run in float64 and
add nothing visible; each result is then rounded to fp32 once (6e-8 relative), and mass takes one fp32 division by the fp32 sum s
(token_logprob's, a few 2^-24 relative)."""
import numpy as np
import torch

MEASURED = {"mass": 1.907e-07, "mean": 4.261e-07, "std": 1.132e-07, "ent": 2.504e-07}
BOUND = {k: 4 * v for k, v in MEASURED.items()}
NAMES = ("mass", "mean", "std", "ent")

VS = (5, 261, 32262, 40003)                      # below one chunk, no multiple of 8 above the largest window but one, the 7B vocabulary, the two-read form
NBS = (1, 3, 256, 1024)
RS = (1, 3, 130)
PAD = 58                                         # ld = V + PAD: an even number of elements that shifts every row's 16-byte phase
KINDS = ("gauss", "peak", "two", "equal", "outside", "inf_out", "all_inf", "offset_up", "offset_down", "bf16r", "one_hot")


def values(nb):
    return np.linspace(-1, 1, nb)


def cases(V):
    """The (nb, p0, R) the kernel runs at for a row length V: every nb <= V of NBS with the window at the row's start, in its middle (an odd
    offset) and at its end (p0 + nb == V); R = 1 and 3 everywhere, 130 once per V on the end window of the largest nb (V = 32262, nb = 256,
    p0 = 32006 is the 7B tokenizer's layout)."""
    out = []
    nbs = [nb for nb in NBS if nb <= V]
    for nb in nbs:
        for p0 in sorted({0, ((V - nb) // 2) | 1 if V - nb > 1 else 0, V - nb}):
            out.append((nb, p0, 3 if nb != nbs[-1] else 1))
    nb = 256 if V == 32262 else nbs[-1]
    out.append((nb, V - nb, 3))
    if V <= 32768:
        out.append((nb, V - nb, 130))
    return out


def make_rows(R, V, p0, nb, dtype, first_kind=0, seed=0):
    """R rows of V logits (CPU tensor of `dtype`); row r is of kind KINDS[(first_kind + r) % len(KINDS)], the window being [p0, p0 + nb):
    gauss        N(0, 3^2)
    peak         Gaussian N(0, 1) with the LAST bin 18 above the largest of the rest: std small but far above sqrt(2^-24)
    two          two equal bins far apart (the first and the last of the window), every other bin -inf: std = |v_a - v_b| / 2
    equal        all logits equal: mean = mean(values), ent = log nb, mass = nb / V
    outside      Gaussian with one token outside the window 20 above everything (nb < V): the mass lies mostly outside
    inf_out      Gaussian inside the window, -inf outside: mass = 1
    all_inf      Gaussian outside, every bin -inf (nb < V; with nb == V the row is `equal`): mass = 0, the rest NaN
    offset_up    Gaussian + 80 (exp overflows without the max subtraction); offset_down: Gaussian - 80
    bf16r        Gaussian rounded to bf16 first, whatever `dtype`
    one_hot      one bin finite, every other bin -inf, Gaussian outside: std = 0 and ent = 0 exactly"""
    g = np.random.default_rng(1000 * seed + 7 * V + 13 * nb + p0 + R + 31 * first_kind)
    x = g.normal(0.0, 3.0, (R, V))
    win = slice(p0, p0 + nb)
    out_idx = np.r_[0:p0, p0 + nb:V]
    for r in range(R):
        kind = KINDS[(first_kind + r) % len(KINDS)]
        if kind == "peak":
            x[r] = g.normal(0.0, 1.0, V)
            x[r, p0 + nb - 1] = np.delete(x[r], p0 + nb - 1).max() + 18.0 if V > 1 else 0.0
        elif kind == "two":
            x[r, win] = -np.inf
            x[r, p0] = x[r, p0 + nb - 1] = 2.5
        elif kind == "equal" or (kind == "all_inf" and nb == V):
            x[r] = 1.5
        elif kind == "outside" and nb < V:
            x[r, out_idx[int(g.integers(0, V - nb))]] = x[r].max() + 20.0
        elif kind == "inf_out":
            x[r, out_idx] = -np.inf
        elif kind == "all_inf":
            x[r, win] = -np.inf
        elif kind == "offset_up":
            x[r] += 80.0
        elif kind == "offset_down":
            x[r] -= 80.0
        elif kind == "bf16r":
            x[r] = torch.from_numpy(x[r]).to(torch.bfloat16).double().numpy()
        elif kind == "one_hot":
            k = p0 + int(g.integers(0, nb))
            keep = x[r, k]
            x[r, win] = -np.inf
            x[r, k] = keep
    return torch.from_numpy(x).to(dtype)


def received(x):
    """The values the kernel receives, as float64 numpy [R, V]."""
    return x.to(torch.float64).numpy()


def ref_stats(x64, p0, nb, vals=None):
    """float64 (mass, mean, std, ent), each [R], of x64 [R, V] over the window [p0, p0 + nb) with bin values `vals` (default values(nb))."""
    v = values(nb) if vals is None else np.asarray(vals, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x64.max(1, keepdims=True)
        e = np.exp(x64 - m)
        s = e.sum(1)
        w = e[:, p0:p0 + nb]
        Z = w.sum(1)
        q = w / Z[:, None]
        mean = (q * v).sum(1)
        std = np.sqrt((q * (v - mean[:, None]) ** 2).sum(1))
        ent = -np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), np.where(np.isnan(q), np.nan, 0.0)).sum(1)
    return {"mass": Z / s, "mean": mean, "std": std, "ent": ent}


def ratio(got, ref):
    """worst |got - ref| / (1 + |ref|) over the rows; a row whose reference is NaN counts 0 when got is NaN too and inf otherwise, and a
    got that is not finite where the reference is counts inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / (1.0 + np.abs(ref))
    e = np.where(np.isnan(ref), np.where(np.isnan(got), 0.0, np.inf), np.where(np.isfinite(got), e, np.inf))
    return float(e.max())
