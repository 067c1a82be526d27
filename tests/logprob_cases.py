"""Shared by tests/test_gpu_logprob_kernel.py (GPU) and tests/test_logprob_host.py (CPU): the rows egomi_token_logprob is pinned on, its
float64 reference, and the bound.  Not a test file; numpy / torch-CPU only.

The reference is log_softmax in float64 of the values the kernel receives (the bf16 rows after their rounding), gathered at the token.
A case passes when  |got - ref| <= BOUND * (1 + |ref|)  on every row.

MEASURED on the MI355X over every case of tests/test_gpu_logprob_kernel.py (bf16 and fp32, V in VS + VS_LONG, R in RS, both strides,
the rows of KINDS), worst |got - ref| / (1 + |ref|):
    MEASURED = 1.095e-07   (fp32, V = 32262, R = 130; the bf16 cases stay under 8.7e-08)
    BOUND    = 4 x MEASURED = 4.38e-07  (the margin of tests/attn_oracle.py's kind: room for another box's expf / logf)
What the error is made of: the stored fp32 lp carries half an ulp of its own (8 <= |lp| < 16: 4.8e-7 absolute, 5e-8 of 1 + |lp|), x - m and
log s add about an ulp each, and the fp32 sum of V positive terms in 1024 interleaved partial sums stays within a few 2^-24 relative.
tests/test_logprob_host.py shows that the bound is tight enough to mean something: three plausible kernel defects, applied to the
float64 reference on these same rows, miss it by more than 100x."""
import numpy as np
import torch

MEASURED = 1.095e-07
BOUND = 4 * MEASURED

VS = (5, 1023, 1024, 1025, 4099, 32262)          # the issue's sizes: below / at / above one pass of 1024 threads, no multiple of the 8-element chunk, the 7B vocabulary
VS_LONG = (32768, 32769, 40003)                  # the last size the row stays in registers for, and the two-pass form above it
RS = (1, 3, 130)
PAD = 58                                         # ld = V + PAD: an even number of elements that shifts every row's 16-byte phase
KINDS = ("gauss", "peak_tok", "peak_other", "equal", "offset", "tok_first", "tok_last", "low_head")


def make_rows(R, V, dtype, first_kind=0, seed=0):
    """R rows of V logits (CPU tensor of `dtype`) and their tokens (int64 [R]); row r is of kind KINDS[(first_kind + r) % 8]:
    gauss       N(0, 3^2), a random token
    peak_tok    one logit 80 above the largest of the rest; the token is the peak (lp ~ 0)
    peak_other  the same row, the token elsewhere (lp ~ -80)
    equal       all logits equal (lp = -log V)
    offset      fp32: Gaussian + 30000 (exp overflows without the max subtraction); bf16 (spacing 256 up there): Gaussian
    tok_first   Gaussian, token 0
    tok_last    Gaussian, token V - 1
    low_head    Gaussian with the first 1024 columns 120 lower (V > 1024): the row's maximum lies beyond one pass of the workgroup"""
    g = np.random.default_rng(1000 * seed + 7 * V + R + 31 * first_kind)
    x = g.normal(0.0, 3.0, (R, V))
    tok = g.integers(0, V, R)
    for r in range(R):
        kind = KINDS[(first_kind + r) % len(KINDS)]
        if kind in ("peak_tok", "peak_other"):
            p = int(g.integers(0, V))
            x[r, p] = np.delete(x[r], p).max() + 80.0 if V > 1 else 0.0
            tok[r] = p if kind == "peak_tok" else (p + 1 + int(g.integers(0, max(V - 1, 1)))) % V
        elif kind == "equal":
            x[r] = 1.5
        elif kind == "offset" and dtype == torch.float32:
            x[r] += 30000.0
        elif kind == "tok_first":
            tok[r] = 0
        elif kind == "tok_last":
            tok[r] = V - 1
        elif kind == "low_head" and V > 1024:
            x[r, :1024] -= 120.0
    return torch.from_numpy(x).to(dtype), torch.from_numpy(tok.astype(np.int64))


def received(x):
    """The values the kernel receives, as float64 numpy [R, V]."""
    return x.to(torch.float64).numpy()


def ref_logprob(x64, tok):
    """float64 log_softmax of x64 [R, V] gathered at tok [R]."""
    m = x64.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x64 - m).sum(1))
    return x64[np.arange(x64.shape[0]), np.asarray(tok)] - lse


def ratio(got, ref):
    """worst |got - ref| / (1 + |ref|) over the rows (inf when got is not finite where ref is)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / (1.0 + np.abs(ref))
    e = np.where(np.isfinite(got), e, np.inf)
    return float(e.max())
