"""float64 oracle and per-element error metric for the dense products (egomi_gemm: csrc/gemm.hip, gemm_fast.hip, gemm_tn.hip).
A plain module, not a test file: tests/test_gemm_oracle_host.py checks the metric on the CPU, tests/test_gpu_gemm_oracle.py runs every
form of egomi_gemm against it.

Reference.  From the exact values the kernel received (bf16 or fp32 operands, bias, residual, the previous C when accumulating):
    ref  = act(alpha A.B + bias) + R (+ C0)
    E_ij = sum_k |a_ik b_kj|
    T_ij = g (|alpha| E_ij + |bias_j|) + |R_ij| + |C0_ij|          g = 1, or max|GELU'| = 1.13 for GELU
Products of at most 2^29 multiply-adds are computed in float64 on the CPU; larger ones (the bench-size products) with torch's float64
matmul on the device the operands live on.  Both sums are exact to far below the bounds (relative error <= K 2^-53 of E), and
test_gpu_gemm_oracle.py cross-checks the device against the CPU once, on a mid-size product.

Why T.  Every product a_ik b_kj of bf16 operands is exact in fp32, and so is every fp32 MFMA product step's input; what a correct kernel
adds is the rounding of its fp32 partial sums, whatever their order (blocked, split over K-slices and summed in fp32, combined in-launch),
plus the epilogue's few fp32 operations on terms whose magnitudes T already counts.  So the error of each element is bounded by
    |got - ref| <= tau T                                                                            (fp32 outputs, no floor)
and where T = 0 the element is exactly 0.  The a-priori ceiling is gamma_K = K 2^-24 (a serial fp32 sum); tau is far below it because
the kernels sum in short MFMA chains and trees.  For bf16 outputs the kernel rounds once, to nearest even, at the end:
    bf16(ref - tau T) <= got <= bf16(ref + tau T)
i.e. "a correctly rounded value of something inside the accumulation bound" — at most one bf16 ulp wider than exact rounding, and far
tighter than 2^-8 |ref|.  bf16() must be an exact RNE of the float64 end points: torch rounds float64 to bf16 through float32 (double
rounding), so bracket() moves each end one fp32 ulp outward before the bf16 rounding (test_gemm_oracle_host.py checks it against an exact
integer RNE).

Transcendental epilogues.  GELU (erff, act 1) adds RHO_GELU |z|, z = alpha A.B + bias its argument: erff to ~2 fp32 ulps, three roundings,
and 1 + erf(z/sqrt 2) cancelling for z << 0 make the fp32 error an absolute multiple of |z|, not of |gelu(z)|.  SiLU (the SwiGLU
epilogues, from the kernel's own bf16 gate|up) adds RHO_SILU relative to the magnitude of its terms: __expf, one division, one product;
the forward rounds silu(g) to bf16 before multiplying by u (HF's bf16 arithmetic), so its output is bracketed twice.

tau, one per accumulation kind, about 3x the worst err / T measured on MI355X over the whole of test_gpu_gemm_oracle.py (every form, every
input family, K from 50 to 32320).  Worst per form (bf16 operands): 8-phase 1.69e-7, 256x128 1.67e-7, k-major 1.67e-7, m256 1.62e-7,
352x256 1.55e-7, 128x128 1.54e-7, gemv_m16 1.28e-7, column split 1.20e-7, generic 1.18e-7, persistent 0.94e-7, k-major 352x256 0.94e-7;
slab sums 0.7e-8 .. 4.6e-8.  All far under gamma_K.
    TAU_BF16_MFMA   bf16 operands, fp32 MFMA accumulation (every tuned form, the bf16 generic kernel)    measured 1.69e-7   tau 5e-7
    TAU_F32_MFMA    fp32 operands, v_mfma_f32_16x16x4_f32 (the fp32 generic kernel)                      measured 2.83e-7   tau 8.5e-7
"""
import math

import torch

TAU_BF16_MFMA = 5e-7
TAU_F32_MFMA = 8.5e-7
RHO_GELU = 5e-7
RHO_SILU = 1e-6
GELU_SLOPE = 1.13                 # max |GELU'(z)| = 1.1289 at z = 1.4142
CPU_MACS = 1 << 29


def _mat(X, layout, rows_first):
    """operand in memory layout -> float64 logical matrix.  A: layout 0 [M,K], 1 [K,M] -> [M,K]; B: layout 0 [N,K], 1 [K,N] -> [K,N]."""
    X = X.double()
    if rows_first:
        return X if layout == 0 else X.t()
    return X.t() if layout == 0 else X


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def reference(A, B, a_layout=0, b_layout=0, alpha=1.0, bias=None, act=0, residual=None, c0=None, device=None):
    """-> (ref, T, extra) float64 [M, N]: the exact result, the term magnitudes, and the transcendental slack (GELU: RHO_GELU |z|)."""
    Am, Bm = _mat(A, a_layout, True), _mat(B, b_layout, False)
    M, K = Am.shape
    N = Bm.shape[1]
    if device is None:
        device = "cpu" if M * N * K <= CPU_MACS else A.device
    Am, Bm = Am.to(device), Bm.to(device)
    z = alpha * (Am @ Bm)
    T = abs(alpha) * (Am.abs() @ Bm.abs())
    del Am, Bm
    if bias is not None:
        b = bias.double().to(device)[None, :N]
        z = z + b
        T = T + b.abs()
    extra = torch.zeros_like(T)
    if act == 1:
        ref = _gelu(z)
        T = GELU_SLOPE * T
        extra = RHO_GELU * z.abs()
    elif act == 2:
        ref = z.clamp_min(0.0)
    else:
        ref = z
    for t in (residual, c0):
        if t is not None:
            t = t.double().to(device)
            ref = ref + t
            T = T + t.abs()
    return ref, T, extra


def exact_bf16(x):
    """float64 -> the exact round-to-nearest-even bf16 value, as float64 (normal range; integer arithmetic on the float64 bits)."""
    x = x.double().contiguous()
    bits = x.view(torch.int64)
    lsb = (bits >> 45) & 1
    r = ((bits + (1 << 44) - 1 + lsb) >> 45) << 45
    out = r.view(torch.float64)
    return torch.where(torch.isfinite(x) & (x != 0), out, x)


def _f32_out(v, down):
    """float64 -> a float32 value strictly beyond v on the outer side (one fp32 ulp past its rounding), as float64."""
    f = v.float()
    inf = torch.full_like(f, -math.inf if down else math.inf)
    return torch.nextafter(f, inf).double()


def bracket(lo64, hi64):
    """bf16 values [bf16(lo), bf16(hi)] (as float64) of float64 end points, each widened one fp32 ulp outward against double rounding."""
    lo = _f32_out(lo64, True).to(torch.bfloat16).double()
    hi = _f32_out(hi64, False).to(torch.bfloat16).double()
    return lo, hi


def _report(err, T, bad, what, got, ref, bound):
    if bool(bad.any()):
        idx = bad.nonzero()[:5].tolist()
        ex = [(i, float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound (index, got, ref, bound): {ex}")


def ratio(err, T):
    m = T > 0
    return float((err[m] / T[m]).max()) if bool(m.any()) else 0.0


def check_f32(got, ref, T, tau, extra=None, what="C"):
    """fp32 output: |got - ref| <= tau T (+ extra) for every element, no floor.  -> worst err / T."""
    g = got.double().to(ref.device)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = (g - ref).abs()
    bound = tau * T if extra is None else tau * T + extra
    _report(err, T, err > bound, what, g, ref, bound)
    return ratio(err, T)


def check_bf16(got, ref, T, tau, extra=None, what="C"):
    """bf16 output: bf16(ref - b) <= got <= bf16(ref + b), b = tau T (+ extra).  -> worst err / T of the unrounded distance."""
    g = got.double().to(ref.device)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    b = tau * T if extra is None else tau * T + extra
    lo, hi = bracket(ref - b, ref + b)
    bad = (g < lo) | (g > hi)
    if bool(bad.any()):
        idx = bad.nonzero()[:5].tolist()
        ex = [(i, float(g[tuple(i)]), float(ref[tuple(i)]), float(lo[tuple(i)]), float(hi[tuple(i)])) for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} bf16 elements outside [bf16(ref - tau T), bf16(ref + tau T)] "
                             f"(index, got, ref, lo, hi): {ex}")
    # distance beyond exact rounding, for the measurement of tau: 0 where got is the RNE of ref
    err = torch.where(g == exact_bf16(ref), torch.zeros_like(g), (g - ref).abs() - (exact_bf16(ref) - ref).abs()).clamp_min(0.0)
    return ratio(err, T)


def check(got, ref, T, tau, extra=None, what="C"):
    if got.dtype == torch.bfloat16:
        return check_bf16(got, ref, T, tau, extra, what)
    return check_f32(got, ref, T, tau, extra, what)


def check_exact(got, ref, what="C"):
    """exact-integer family: fp32 outputs equal ref bit for bit, bf16 outputs equal RNE(ref) bit for bit."""
    g = got.double().to(ref.device)
    want = exact_bf16(ref) if got.dtype == torch.bfloat16 else ref
    bad = ~(g == want)
    if bool(bad.any()):
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ from the exact result: "
                             f"{[(i, float(g[tuple(i)]), float(want[tuple(i)])) for i in idx]}")


def old_criterion(got, ref, tol):
    """the per-tensor criterion the older tests use: max|got - ref| <= tol max|ref|."""
    return float((got.double() - ref).abs().max()) <= tol * float(ref.abs().max())


# ------------------------------------------------------------------------------------------ input families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_ints(M, N, K, seed=0, kt=64, rows_span=8, cols_span=8, tile_span=3):
    """Exact-integer family: small integers (|x| <= 4, about a third zero) scaled by powers of two per row of A (2^ra), per column of B
    (2^cb) and per K-tile (on A).  -> A [M, K], B [N, K] (float32, exactly representable in bf16), ra [M], cb [N].  Every partial sum of
    element (i, j), in any order, is a multiple of 2^(ra_i + cb_j + min kt) below 2^21 of it (asserted), so every fp32 order is exact,
    with room for the epilogue terms of exact_epilogue()."""
    g = _gen(seed)
    ia = torch.randint(-4, 5, (M, K), generator=g).float()
    ib = torch.randint(-4, 5, (N, K), generator=g).float()
    ia[torch.rand(M, K, generator=g) < 0.22] = 0.0        # randint gives 1/9 zeros: about a third in all
    ib[torch.rand(N, K, generator=g) < 0.22] = 0.0
    ra = torch.randint(-rows_span, rows_span + 1, (M,), generator=g).float()
    cb = torch.randint(-cols_span, cols_span + 1, (N,), generator=g).float()
    tk = torch.randint(0, tile_span + 1, ((K + kt - 1) // kt,), generator=g).float().repeat_interleave(kt)[:K]
    worst = float((ia.abs() * torch.exp2(tk - tk.min())[None]).sum(1).max()) * 4.0
    assert worst < 2.0 ** 21, f"exact_ints: partial sums reach {worst} units"
    A = ia * torch.exp2(ra)[:, None] * torch.exp2(tk)[None]
    B = ib * torch.exp2(cb)[:, None]
    return A, B, ra, cb


def exact_epilogue(ra, cb, seed=0):
    """bias / residual / C0 for the exact family, on the product's own units: R_ij, C0_ij = int 2^(ra_i + cb_j), bias_j = int 2^(min ra + cb_j).
    With rows_span <= 1 in exact_ints (units of one column within 2^2 of each other) alpha in {1, 0.5, -2} times the product plus these
    stays below 2^24 of the smallest unit: every fp32 epilogue order is exact too."""
    assert float(ra.max() - ra.min()) <= 2.0, "exact_epilogue: rows_span <= 1"
    g = _gen(seed + 7)
    M, N = ra.numel(), cb.numel()
    unit = torch.exp2(ra[:, None] + cb[None, :])
    bias = torch.randint(-4, 5, (N,), generator=g).float() * torch.exp2(ra.min() + cb)
    res = torch.randint(-4, 5, (M, N), generator=g).float() * unit
    c0 = torch.randint(-4, 5, (M, N), generator=g).float() * unit
    return bias, res, c0


def graded(M, N, K, seed=0, span=8, cancel_rows=0):
    """Graded family: N(0,1) operands, rows of A and columns of B scaled by 2^U(-span, span).  cancel_rows > 0: B's second half of K
    duplicates its first, and in every cancel_rows-th row of A the second half negates the first, so those rows of ref are exactly 0
    while E is large."""
    g = _gen(seed + 11)
    A = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-span, span + 1, (M, 1), generator=g).float())
    B = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-span, span + 1, (N, 1), generator=g).float())
    if cancel_rows:
        h = K // 2
        B[:, h:2 * h] = B[:, :h]
        A[::cancel_rows, h:2 * h] = -A[::cancel_rows, :h]
    return A, B


def bench_like(M, N, K, seed=0):
    """the existing tests' scales: activations N(0,1), weights 0.05 N(0,1)."""
    g = _gen(seed + 13)
    return torch.randn(M, K, generator=g), 0.05 * torch.randn(N, K, generator=g)
