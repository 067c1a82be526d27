"""CPU: the GEMM metric of tests/gemm_oracle.py.  Emulated correct kernels (fp32 accumulation of exact 32-term MFMA steps in blocked
orders, K-slices summed in fp32, RNE to bf16 on output) pass it on every input family with margin; six defects that the older per-tensor
criterion (tol max|ref|) accepts fail it; the bf16 bracket agrees with an exact rounding."""
import math
from fractions import Fraction

import pytest
import torch

from tests import gemm_oracle as G

TAU = G.TAU_BF16_MFMA


def emulate(A, B, bias=None, residual=None, alpha=1.0, act=0, slices=1, step=32, out=torch.float32, slab_dtype=torch.float32,
            truncate=False):
    """A correct kernel's arithmetic: each 32-K MFMA step exact (bf16 products, summed exactly, rounded once to fp32), steps added in fp32
    in K order inside a slice; slices summed in fp32; then alpha, bias, activation, residual in fp32 and one rounding of the output."""
    M, K = A.shape
    Ad, Bd = A.double(), B.double()
    per = -(-(K // step) // slices) * step
    total = torch.zeros(M, B.shape[0], dtype=torch.float32)
    for s0 in range(0, K, per):
        acc = torch.zeros(M, B.shape[0], dtype=torch.float32)
        for k in range(s0, min(K, s0 + per), step):
            acc = acc + (Ad[:, k:k + step] @ Bd[:, k:k + step].t()).float()
        total = total + acc.to(slab_dtype).float()
    v = total * alpha
    if bias is not None:
        v = v + bias.float()[None]
    if act == 1:
        v = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))
    elif act == 2:
        v = v.clamp_min(0.0)
    if residual is not None:
        v = v + residual.float()
    if out == torch.bfloat16 and truncate:
        return (v.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    return v.to(out)


def bf(x):
    return x.to(torch.bfloat16)


FAMILIES = ["bench", "graded", "cancel", "exact"]


def operands(fam, M=96, N=72, K=512):
    if fam == "bench":
        A, B = G.bench_like(M, N, K)
    elif fam == "graded":
        A, B = G.graded(M, N, K)
    elif fam == "cancel":
        A, B = G.graded(M, N, K, cancel_rows=3)
    else:
        A, B, _, _ = G.exact_ints(M, N, K)
    return bf(A), bf(B)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("out", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slices", [1, 3])
def test_metric_accepts_correct_kernels_with_margin(fam, out, slices):
    A, B = operands(fam)
    got = emulate(A, B, slices=slices, out=out)
    ref, T, _ = G.reference(A, B)
    if fam == "exact":
        G.check_exact(got, ref)
    r = G.check(got, ref, T, TAU / 2)                           # half of tau: the emulated orders stay well inside the bound
    assert r < TAU / 2
    if fam == "cancel":
        assert bool((ref[::3] == 0).all()) and bool((T[::3] > 0).all())


@pytest.mark.parametrize("out", [torch.float32, torch.bfloat16])
def test_metric_accepts_epilogues(out):
    A, B, ra, cb = G.exact_ints(64, 40, 256, rows_span=1)
    bias, res, c0 = G.exact_epilogue(ra, cb)
    for alpha in (1.0, 0.5, -2.0):
        for act in (0, 2):
            got = emulate(bf(A), bf(B), bias=bf(bias), residual=res.to(out), alpha=alpha, act=act, out=out)
            ref, T, _ = G.reference(bf(A), bf(B), alpha=alpha, bias=bf(bias), act=act, residual=res.to(out))
            G.check_exact(got, ref)
    A, B = operands("graded", 64, 40, 256)
    bias = bf(torch.randn(40))
    got = emulate(A, B, bias=bias, alpha=0.5, act=1, out=out)
    ref, T, extra = G.reference(A, B, alpha=0.5, bias=bias, act=1)
    G.check(got, ref, T, TAU / 2, extra)


def _fails(got, ref, T, extra=None):
    with pytest.raises(AssertionError):
        G.check(got, ref, T, TAU, extra)


def test_rejects_zeroed_small_row():
    A, B = operands("bench")
    A[5] = bf(A[5].float() * 1e-2)
    ref, T, _ = G.reference(A, B)
    got = emulate(A, B, out=torch.bfloat16)
    got[5] = 0
    assert G.old_criterion(got, ref, 2e-2)
    _fails(got, ref, T)


def test_rejects_slab_rounded_to_bf16():
    A, B = operands("bench", K=2048)
    ref, T, _ = G.reference(A, B)
    got = emulate(A, B, slices=4, slab_dtype=torch.bfloat16)
    assert G.old_criterion(got, ref, 2e-3)
    _fails(got, ref, T)


def test_rejects_one_missing_product():
    A, B = operands("bench")
    ref, T, _ = G.reference(A, B)
    got = emulate(A, B)
    i, j = 7, 11
    terms = (A[i].double() * B[j].double()).abs()
    k = int((terms - 5e-4 * float(ref.abs().max())).abs().argmin())   # a product the per-tensor criterion cannot see
    got[i, j] -= float(A[i, k].double() * B[j, k].double())
    assert G.old_criterion(got, ref, 1e-3)
    _fails(got, ref, T)


def test_rejects_truncation_instead_of_rne():
    A, B = operands("graded")
    ref, T, _ = G.reference(A, B)
    G.check(emulate(A, B, out=torch.bfloat16), ref, T, TAU)
    got = emulate(A, B, out=torch.bfloat16, truncate=True)
    assert G.old_criterion(got, ref, 2e-2)
    _fails(got, ref, T)


def test_rejects_bias_shifted_in_last_partial_column_group():
    M, N = 96, 70                                                  # columns 64..69: the last, partial group of 8
    A, B = operands("bench", M, N)
    bias = bf(5e-3 * torch.randn(N + 1, generator=torch.Generator().manual_seed(3)))
    ref, T, _ = G.reference(A, B, bias=bias[:N])
    good = emulate(A, B, bias=bias[:N], out=torch.bfloat16)
    G.check(good, ref, T, TAU)
    shifted = bias[:N].clone()
    shifted[64:] = bias[65:N + 1]
    got = emulate(A, B, bias=shifted, out=torch.bfloat16)
    assert G.old_criterion(got, ref, 2e-2)
    _fails(got, ref, T)


def test_rejects_residual_from_neighbouring_row_in_last_row_group():
    M, N = 100, 64                                                 # rows 96..99: the last, partial group of 8
    A, B = operands("bench", M, N)
    R = bf(1e-2 * torch.randn(M, N, generator=torch.Generator().manual_seed(4)))
    ref, T, _ = G.reference(A, B, residual=R)
    G.check(emulate(A, B, residual=R, out=torch.bfloat16), ref, T, TAU)
    Rw = R.clone()
    Rw[96:] = R[95:99]
    got = emulate(A, B, residual=Rw, out=torch.bfloat16)
    assert G.old_criterion(got, ref, 2e-2)
    _fails(got, ref, T)


def _rne_bf16_exact(x: float) -> float:
    if x == 0 or not math.isfinite(x):
        return x
    m, e = math.frexp(x)                                          # x = m 2^e, 0.5 <= |m| < 1: bf16 keeps 8 significant bits
    q = round(Fraction(m) * 256)                                  # Fraction rounding: half to even, exact
    return float(Fraction(q, 256) * Fraction(2) ** e)


def test_bf16_rounding_helpers_are_exact():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(4000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 20, (4000,), generator=g).double())
    b16 = base.to(torch.bfloat16).double()
    ulp = torch.exp2(torch.floor(torch.log2(b16.abs())) - 7)
    tiny = torch.exp2(torch.floor(torch.log2(b16.abs())) - 40)
    mids = b16 + 0.5 * ulp                                        # exact midpoints, and values just beside them that fp32 cannot tell apart
    xs = torch.cat([base, mids, mids + tiny, mids - tiny, b16])
    want = torch.tensor([_rne_bf16_exact(float(v)) for v in xs], dtype=torch.float64)
    assert torch.equal(G.exact_bf16(xs), want)
    assert not torch.equal(xs.to(torch.bfloat16).double(), want)  # torch's double rounding differs somewhere here: the helpers are needed
    lo, hi = G.bracket(xs, xs)
    assert bool((lo <= want).all()) and bool((want <= hi).all())
    wide = (lo < want) | (hi > want)                              # one bf16 ulp at most, and only where x is within an fp32 ulp of a midpoint
    step = torch.exp2(torch.floor(torch.log2(want.abs())) - 7)
    assert bool(((want - lo) <= step).all()) and bool(((hi - want) <= step).all())
    assert int(wide.sum()) <= 4 * len(base) - len(base) // 2


def test_exact_family_is_exact_in_any_fp32_order():
    A, B, _, _ = G.exact_ints(48, 40, 4096)
    ref, T, _ = G.reference(bf(A), bf(B))
    assert torch.equal(bf(A).float(), A) and torch.equal(bf(B).float(), B)
    for slices, step in ((1, 32), (5, 64), (1, 4096)):
        G.check_exact(emulate(bf(A), bf(B), slices=slices, step=step), ref)
        G.check_exact(emulate(bf(A), bf(B), slices=slices, step=step, out=torch.bfloat16), ref)
