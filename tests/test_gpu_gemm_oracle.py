"""GPU: every form of egomi_gemm (csrc/gemm.hip, gemm_fast.hip, gemm_tn.hip) against the float64 oracle of tests/gemm_oracle.py, bounded per
element (fp32: |got - ref| <= tau T; bf16: inside [bf16(ref - tau T), bf16(ref + tau T)]; exact-integer inputs: bit for bit).

Every case also checks the harness rules: overwritten outputs are prefilled with NaN inside a window of a larger buffer (ldc > N, a column
offset, a guard row above and below) whose sentinel bits must come back unchanged; the slack of every strided input (columns past K or N
up to the leading dimension, the columns beside a column slice, the rows past K of a k-major operand) holds NaN; a second launch gives the
same bits; the route the library recorded (egomi_gemm_last_route) is the form the case was written for; the plan queries
(egomi_gemm_tail_plan, egomi_gemm_tn_tail_plan, egomi_gemm_slab_count) agree with what the launch recorded.

EGOMI_GEMM_ORACLE_LOG=<file>: the worst err / T per form is written there as JSON (the measurement behind tau in gemm_oracle.py)."""
import ctypes
import json
import os
import re

import pytest
import torch

from tests import gemm_oracle as G

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN_BITS = {BF: 0x7FC0, F32: 0x7FC00000}
SENT_BITS = {BF: 0x7F8F, F32: 0x7FA0BEEF}             # guard pattern: a NaN no kernel writes
IVIEW = {BF: torch.int16, F32: torch.int32}
WORST = {}
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from egoscaler_amd import ops as O
    yield O
    log = os.environ.get("EGOMI_GEMM_ORACLE_LOG")
    if log:
        with open(log, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.fixture()
def tall(ops):
    from egoscaler_amd import _lib
    L = _lib.lib()

    def set_mode(m):
        assert L.egomi_gemm_set_tall(ctypes.c_int(m)) == 0
    yield set_mode
    L.egomi_gemm_set_tall(ctypes.c_int(-1))             # process-wide: restored whatever the test did


def _note(form, r, kind="bf16_mfma"):
    key = f"{kind}:{form}"
    WORST[key] = max(WORST.get(key, 0.0), r)


# ------------------------------------------------------------------------------------------ buffers
def _fill_bits(t, bits):
    """fill with a bit pattern (t float, or its integer view)"""
    v = t.view(IVIEW[t.dtype]) if t.dtype in IVIEW else t
    v.fill_(bits - (1 << (8 * t.element_size())) if bits >= 1 << (8 * t.element_size() - 1) else bits)


class Window:
    """[rows, cols] output view inside a sentinel-filled buffer: one guard row above and below, 8 columns before, >= 24 after."""

    def __init__(self, rows, cols, dtype, init=None):
        self.col0, self.rows, self.cols = 8, rows, cols
        self.ld = (self.col0 + cols + 24 + 7) // 8 * 8
        self.buf = torch.empty(rows + 2, self.ld, dtype=dtype, device=DEV)
        _fill_bits(self.buf, SENT_BITS[dtype])
        self.view = self.buf[1:rows + 1, self.col0:self.col0 + cols]
        if init is None:
            _fill_bits(self.view, NAN_BITS[dtype])
        else:
            self.view.copy_(init)

    def guards_intact(self):
        bits = self.buf.view(IVIEW[self.buf.dtype]).clone()
        bits[1:self.rows + 1, self.col0:self.col0 + self.cols] = 0
        want = torch.zeros_like(bits)
        _fill_bits(want, SENT_BITS[self.buf.dtype])
        want[1:self.rows + 1, self.col0:self.col0 + self.cols] = 0
        return torch.equal(bits, want)


def operand(X, dtype, slack=16, col_off=0, extra_rows=0):
    """device copy of the memory image X [R, C] as a strided view: NaN in the columns past C up to the leading dimension, in the col_off
    columns before it, and in extra_rows rows below it (the rows past K of a k-major operand, inside the same allocation)."""
    R, C = X.shape
    ld = (col_off + C + slack + 7) // 8 * 8
    buf = torch.full((R + extra_rows, ld), float("nan"), dtype=dtype, device=DEV)
    v = buf[:R, col_off:col_off + C]
    v.copy_(X.to(dtype))
    return v


def _ld(t):
    return t.stride(0)


def desc(ops, A, B, C, M, N, K, a_layout=0, b_layout=0, bias=None, residual=None, alpha=1.0, act=0, accumulate=False, ws=None,
         tickets=0, split_k=0, force_generic=False, epilogue=0, C2=None, batch=1, batch_inner=1, strides=(0,) * 6):
    d = ops.GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = _ld(A), _ld(B), _ld(C)
    d.ldr = _ld(residual) if residual is not None else 0
    d.a_layout, d.b_layout = a_layout, b_layout
    d.ab_dtype, d.c_dtype = ops.dt(A.dtype), ops.dt(C.dtype)
    d.batch, d.batch_inner = batch, batch_inner
    d.sA0, d.sA1, d.sB0, d.sB1, d.sC0, d.sC1 = strides
    d.alpha, d.accumulate, d.act, d.force_generic = alpha, int(accumulate), act, int(force_generic)
    if ws is not None:
        d.workspace, d.workspace_bytes, d.split_k, d.ws_tickets_zeroed = ws.data_ptr(), ws.numel() * ws.element_size(), split_k, tickets
    else:
        d.split_k = split_k
    if epilogue:
        d.epilogue, d.C2, d.ldc2 = epilogue, C2.data_ptr(), _ld(C2)
    return d


def launch(ops, d):
    from egoscaler_amd import _lib
    _lib.check(_lib.lib().egomi_gemm(ctypes.byref(d), ops.S()), "egomi_gemm")
    route = ops.gemm_last_route()
    torch.cuda.synchronize()
    return route


def workspace(kind):
    """None; 'ws': 64 MiB plain scratch; 'tickets': 64 MiB whose first 4 KB are zero ticket words (ws_tickets_zeroed = 2, too small for the
    persistent form: K-sliced tail rows are combined in-launch); 'persist': room for the persistent form."""
    if kind is None:
        return None, 0
    nbytes = {"ws": 64 << 20, "tickets": 64 << 20, "persist": 4096 + 256 * 2 * 262144}[kind]
    return torch.zeros(nbytes // 4, dtype=F32, device=DEV), (2 if kind in ("tickets", "persist") else 0)


def operands(fam, M, N, K, seed=0):
    """logical A [M, K], B [N, K] float32 of an input family (tests/gemm_oracle.py), plus the exact family's row / column exponents."""
    if fam == "exact":
        return G.exact_ints(M, N, K, seed=seed, rows_span=1)
    if fam == "graded":
        return G.graded(M, N, K, seed=seed) + (None, None)
    if fam == "cancel":
        return G.graded(M, N, K, seed=seed, cancel_rows=5) + (None, None)
    return G.bench_like(M, N, K, seed=seed) + (None, None)


def images(Al, Bl, a_layout, b_layout):
    return (Al if a_layout == 0 else Al.t().contiguous()), (Bl if b_layout == 0 else Bl.t().contiguous())


def run_case(ops, M, N, K, *, fam="graded", a_layout=0, b_layout=0, ab=BF, out=BF, epi=(), alpha=1.0, act=0, ws_kind=None, split_k=0,
             force_generic=False, kmajor_pad=0, col_off=0, form=None, tail=None, splitk=None, na=None, tau=None, seed=0, repeat=True):
    """One product through egomi_gemm with the harness of this module; -> (route, C window view, ref, T)."""
    Al, Bl, ra, cb = operands(fam, M, N, K, seed)
    bias = res = c0 = None
    if fam == "exact" and epi:
        bias, res, c0 = G.exact_epilogue(ra, cb, seed)
    elif epi:
        g = torch.Generator().manual_seed(seed + 99)
        s = float(Al.abs().max() * Bl.abs().max()) * 2.0
        bias, res, c0 = s * torch.randn(N, generator=g), s * torch.randn(M, N, generator=g), s * torch.randn(M, N, generator=g)
    Ai, Bi = images(Al, Bl, a_layout, b_layout)
    A = operand(Ai, ab, extra_rows=kmajor_pad if a_layout == 1 else 0)
    B = operand(Bi, ab, col_off=col_off, extra_rows=kmajor_pad if b_layout == 1 else 0)
    bias_d = operand(bias[None], ab)[0] if "bias" in epi else None
    res_d = operand(res, out) if "residual" in epi else None
    acc = "accumulate" in epi
    win = Window(M, N, out, init=c0.to(out) if acc else None)
    c0_used = win.view.clone() if acc else None
    ws, tick = workspace(ws_kind)
    d = desc(ops, A, B, win.view, M, N, K, a_layout, b_layout, bias=bias_d, residual=res_d, alpha=alpha, act=act, accumulate=acc, ws=ws,
             tickets=tick, split_k=split_k, force_generic=force_generic)
    route = launch(ops, d)
    got = win.view.clone()
    assert win.guards_intact(), "a write outside the output window"
    if tick:
        assert int(ws[:1024].count_nonzero()) == 0, "ticket words not returned to zero"
    # the route the case was written for, and the plan queries against what the launch recorded
    name, sk, row0, slices, Na = route
    if form is not None:
        assert name == form, f"took {route}, written for {form}"
    if splitk is not None:
        assert (sk > 1) == splitk, route
    if tail is not None:
        assert (slices > 0) == tail, route
    if na is not None:
        assert (Na > 0) == na, route
    from egoscaler_amd import _lib
    L = _lib.lib()
    p0, ps = ctypes.c_int(-1), ctypes.c_int(-1)
    if name == "8phase" and L.egomi_gemm_tail_plan(ctypes.byref(d), ctypes.byref(p0), ctypes.byref(ps)) == 0:
        assert (p0.value, ps.value) == ((row0, slices) if slices else (M, 0)), (route, p0.value, ps.value)
    if name in ("kmajor", "kmajor_tall") and L.egomi_gemm_tn_tail_plan(ctypes.byref(d), ctypes.byref(p0), ctypes.byref(ps)) == 0:
        assert (p0.value, ps.value) == ((row0, slices) if slices else (M, 0)), (route, p0.value, ps.value)
    # the oracle, from the exact values the kernel received
    ref, T, extra = G.reference(Ai.to(ab), Bi.to(ab), a_layout, b_layout, alpha=alpha, bias=bias_d, act=act, residual=res_d, c0=c0_used)
    if tau is None:
        tau = G.TAU_F32_MFMA if ab == F32 else G.TAU_BF16_MFMA
    if fam == "exact" and act != 1:
        G.check_exact(got, ref)
    else:
        _note(name, G.check(got, ref, T, tau, extra if act == 1 else None), "f32_mfma" if ab == F32 else "bf16_mfma")
    if repeat:
        if acc:
            win.view.copy_(c0_used)
        if tick:
            ws[1024:].zero_()
        launch(ops, d)
        assert torch.equal(win.view.view(IVIEW[out]), got.view(IVIEW[out])), "a second launch changed the result"
    return route, got, ref, T


# ------------------------------------------------------------------------------------------ generic kernel
GENERIC = [(100, 70, 50, 0, 0), (100, 70, 50, 0, 1), (100, 70, 50, 1, 0), (100, 70, 50, 1, 1), (129, 257, 97, 1, 1), (16, 8, 300, 0, 0)]


@pytest.mark.parametrize("M,N,K,la,lb", GENERIC)
@pytest.mark.parametrize("ab,out", [(BF, BF), (BF, F32), (F32, F32)])
@pytest.mark.parametrize("fam", ["exact", "graded", "cancel"])
def test_generic_all_layouts(ops, M, N, K, la, lb, ab, out, fam):
    run_case(ops, M, N, K, fam=fam, a_layout=la, b_layout=lb, ab=ab, out=out, form="generic")


@pytest.mark.parametrize("ab,out", [(BF, BF), (BF, F32), (F32, F32)])
@pytest.mark.parametrize("alpha,act", [(0.5, 0), (-2.0, 2), (1.0, 2)])
def test_generic_epilogue_exact(ops, ab, out, alpha, act):
    run_case(ops, 100, 72, 130, fam="exact", ab=ab, out=out, epi=("bias", "residual", "accumulate"), alpha=alpha, act=act, form="generic")


@pytest.mark.parametrize("ab,out", [(BF, BF), (F32, F32)])
def test_generic_gelu(ops, ab, out):
    run_case(ops, 100, 72, 130, fam="graded", ab=ab, out=out, epi=("bias", "residual"), alpha=0.5, act=1, form="generic")


@pytest.mark.parametrize("ab,out", [(BF, BF), (BF, F32), (F32, F32)])
def test_generic_batched(ops, ab, out):
    """batch = 6 = 3 x batch_inner 2, every operand a strided stack (the unfused attention products of engine.py)."""
    Z0, Z1, M, N, K = 3, 2, 40, 56, 72
    Al, Bl, _, _ = G.exact_ints(Z0 * Z1 * M, N * Z0 * Z1, K, rows_span=1)
    Al, Bl = Al.view(Z0, Z1, M, K), Bl.view(Z0, Z1, N, K)
    A = torch.full((Z0, Z1, M, K + 8), float("nan"), dtype=ab, device=DEV)
    B = torch.full((Z0, Z1, N, K + 8), float("nan"), dtype=ab, device=DEV)
    A[..., :K], B[..., :K] = Al.to(ab), Bl.to(ab)
    win = Window(Z0 * Z1 * M, N, out)
    sC0, sC1 = 2 * M * win.ld, M * win.ld
    d = desc(ops, A[0, 0, :, :K], B[0, 0, :, :K], win.view, M, N, K, batch=Z0 * Z1, batch_inner=Z1,
             strides=(A.stride(0), A.stride(1), B.stride(0), B.stride(1), sC0, sC1))
    assert launch(ops, d)[0] == "generic"
    assert win.guards_intact()
    for z0 in range(Z0):
        for z1 in range(Z1):
            ref, T, _ = G.reference(Al[z0, z1].to(ab), Bl[z0, z1].to(ab))
            r0 = (z0 * Z1 + z1) * M
            G.check_exact(win.view[r0:r0 + M], ref)


# ------------------------------------------------------------------------------------------ 128x128, 256x128, gemv, m256, skinny split-K
FAST = [  # M, N, K, ws, form, split
    (600, 520, 1024, None, "128x128", False), (129, 4096, 1024, None, "128x128", False), (128, 2056, 1088, None, "128x128", False),
    (64, 1024, 4096, "ws", "128x128", True), (17, 4096, 4096, "ws", "128x128", True), (512, 2048, 2048, "ws", "128x128", True),
    (512, 4096, 2048, "ws", "128x128", True), (513, 4096, 2048, "ws", "128x128", False), (4104, 384, 1536, "ws", "128x128", True),
    (32512, 256, 2048, None, "128x128", False),
    (2049, 8200, 576, None, "256x128", False), (2048, 8192, 1024, None, "256x128", False),
    (16, 4096, 4096, "ws", "gemv_m16", True), (8, 4104, 1024, None, "gemv_m16", False), (1, 16384, 2048, "ws", "gemv_m16", True),
    (200, 8192, 1024, "ws", "m256", True), (256, 8200, 1024, None, "m256", False), (257, 8192, 1024, "ws", "128x128", True),
]


@pytest.mark.parametrize("M,N,K,ws,form,split", FAST)
@pytest.mark.parametrize("out", [BF, F32])
def test_fast_forms(ops, M, N, K, ws, form, split, out):
    for fam in ("exact", "cancel"):
        run_case(ops, M, N, K, fam=fam, out=out, ws_kind=ws, form=form, splitk=split)


@pytest.mark.parametrize("M,N,K,form", [(600, 520, 1024, "128x128"), (2049, 8200, 576, "256x128"), (8, 4096, 4096, "gemv_m16"),
                                        (200, 8192, 1024, "m256")])
def test_fast_forms_epilogues(ops, M, N, K, form):
    run_case(ops, M, N, K, fam="exact", out=F32, epi=("bias", "residual", "accumulate"), alpha=-2.0, act=2, form=form)
    run_case(ops, M, N, K, fam="graded", out=BF, epi=("bias", "residual"), alpha=0.5, act=1, form=form)


def test_gemv_last_split_with_ragged_step_count(ops):
    """gemv_m16 with K / 128 = 33 steps over an explicit 4 slices: the last slice is short."""
    run_case(ops, 12, 4096, 4224, fam="exact", ws_kind="ws", split_k=4, form="gemv_m16", splitk=True)
    run_case(ops, 12, 4096, 4224, fam="graded", out=F32, ws_kind="ws", split_k=4, form="gemv_m16", splitk=True)


def _slab_case(ops, M, N, K, form):
    """EGOMI_EPI_SLABS on a skinny product: the fp32 sum of the slabs obeys the fp32 rule, each slab its own K range (per = ceil(nt / S))."""
    from egoscaler_amd import _lib
    Al, Bl, _, _ = G.graded(M, N, K) + (None, None)
    A, B = operand(Al, BF), operand(Bl, BF)
    win = Window(M, N, BF)
    ws, _ = workspace("ws")
    ws.fill_(float("nan"))
    d = desc(ops, A, B, win.view, M, N, K, ws=ws)
    d.epilogue = 2
    S = _lib.lib().egomi_gemm_slab_count(ctypes.byref(d))
    assert S >= 2
    route = launch(ops, d)
    assert route[0] == form and route[1] == S, (route, S)
    assert bool(win.view.isnan().all()) and win.guards_intact(), "EGOMI_EPI_SLABS must not touch C"
    slabs = ws[:S * M * N].view(S, M, N)
    ref, T, _ = G.reference(Al.to(BF), Bl.to(BF))
    _note(form + "_slabs", G.check_f32(slabs.double().sum(0), ref, T, G.TAU_BF16_MFMA, what="sum of slabs"))
    step = 128 if form == "gemv_m16" else 64
    nt = K // step
    per = -(-nt // S)
    for s in range(S):                                  # gemv_m16 cuts its 128-K steps as floor(T s / S), the others in ceil(nt / S) K-tiles
        k0, k1 = ((nt * s // S) * step, (nt * (s + 1) // S) * step) if form == "gemv_m16" else (s * per * step, min(K, (s + 1) * per * step))
        r, t, _ = G.reference(Al[:, k0:k1].to(BF), Bl[:, k0:k1].to(BF))
        G.check_f32(slabs[s], r, t, G.TAU_BF16_MFMA, what=f"slab {s} of {S}")


@pytest.mark.parametrize("M,N,K,form", [(64, 1024, 4096, "128x128"), (8, 4096, 4096, "gemv_m16"), (8, 4096, 4224, "gemv_m16"),
                                        (256, 8192, 2048, "m256")])
def test_skinny_slabs(ops, M, N, K, form):
    _slab_case(ops, M, N, K, form)


# ------------------------------------------------------------------------------------------ 256x256 8-phase, persistent, tall, split
BIG = [  # M, N, K, ws, split_k, tall mode, form, tail
    (4097, 2056, 2112, None, 0, 0, "8phase", False), (4097, 2296, 2112, "ws", 35, 0, "8phase", True),
    (4097, 2056, 2112, "tickets", 35, 0, "8phase", True), (4352, 4096, 2048, "ws", 0, 0, "8phase", None),
    (32513, 256, 2048, None, 0, 0, "8phase", False), (1280, 4096, 32320, "ws", 0, 0, "8phase", True),
    (8192, 8192, 1024, None, 0, 0, "8phase", False),
    (4097, 2056, 2048, "persist", 0, 0, "persistent", False), (5536, 4096, 4096, "persist", 0, 0, "persistent", False),
    (2824, 3072, 2048, None, 0, 2, "tall", False), (3168, 2048, 8192, "ws", 0, 2, "tall", False),
    (5536, 4096, 4096, "ws", 0, 1, "tall", False), (5536, 11008, 2048, "ws", 0, 1, "split", None),
]


@pytest.mark.parametrize("M,N,K,ws,sk,mode,form,tail", BIG)
def test_big_forms(ops, tall, M, N, K, ws, sk, mode, form, tail):
    tall(mode)
    fams = ("exact", "cancel") if M * N * K <= 40e9 else ("bench",)
    for i, fam in enumerate(fams):
        run_case(ops, M, N, K, fam=fam, out=BF if i == 0 else F32, ws_kind=ws, split_k=sk, form=form, tail=tail,
                 na=True if form == "split" else None)


@pytest.mark.parametrize("form,mode,M,N,K,ws,sk", [("8phase", 0, 4097, 2056, 2112, "ws", 35), ("tall", 2, 2824, 3072, 2048, None, 0),
                                                   ("persistent", 0, 4097, 2056, 2048, "persist", 0)])
def test_big_forms_epilogues(ops, tall, form, mode, M, N, K, ws, sk):
    """bias, GELU / ReLU, alpha, residual and accumulate: the 352x256 form falls back to the general epilogue for them."""
    tall(mode)
    run_case(ops, M, N, K, fam="exact", out=F32, epi=("bias", "residual", "accumulate"), alpha=-2.0, act=2, ws_kind=ws, split_k=sk, form=form)
    run_case(ops, M, N, K, fam="exact", out=BF, epi=("bias", "residual"), alpha=0.5, act=0, ws_kind=ws, split_k=sk, form=form)
    run_case(ops, M, N, K, fam="graded", out=BF, epi=("bias",), alpha=0.5, act=1, ws_kind=ws, split_k=sk, form=form)


def test_device_reference_matches_cpu(ops):
    """the float64 oracle on the device (bench-size products) against the CPU, once, on a mid-size product."""
    Al, Bl = G.bench_like(1024, 768, 2048)
    a, b = Al.to(BF), Bl.to(BF)
    r0, t0, _ = G.reference(a, b, device="cpu")
    r1, t1, _ = G.reference(a.cuda(), b.cuda(), device=DEV)
    assert float((r1.cpu() - r0).abs().max()) <= 1e-12 * float(t0.max())
    assert float((t1.cpu() - t0).abs().max()) <= 1e-12 * float(t0.max())


@pytest.mark.parametrize("M,N,K,ws,sk", [(4097, 2056, 2112, "ws", 35), (4352, 4096, 4096, "tickets", 0), (4352, 4096, 4096, "ws", 0)])
def test_large_tail_slabs(ops, tall, M, N, K, ws, sk):
    """EGOMI_EPI_SLABS on a large product: whole tiles get the epilogue, the K-sliced tail rows stay as fp32 slabs whose sum obeys the fp32
    rule and whose slices each cover their own K range; plan == launch."""
    from egoscaler_amd import _lib
    tall(0)
    Al, Bl = G.graded(M, N, K, cancel_rows=7)
    A, B = operand(Al, BF), operand(Bl, BF)
    win = Window(M, N, BF)
    wsb, tick = workspace(ws)
    d = desc(ops, A, B, win.view, M, N, K, ws=wsb, tickets=tick, split_k=sk)
    p0, ps = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().egomi_gemm_tail_plan(ctypes.byref(d), ctypes.byref(p0), ctypes.byref(ps)) == 0
    d.epilogue = 2
    route = launch(ops, d)
    row0, S = p0.value, ps.value
    assert route[0] == "8phase" and (route[2], route[3]) == ((row0, S) if S else (M, 0)), (route, row0, S)
    assert win.guards_intact()
    ref, T, _ = G.reference(A, B)
    G.check_bf16(win.view[:row0], ref[:row0], T[:row0], G.TAU_BF16_MFMA, what="whole tiles")
    assert bool(win.view[row0:].isnan().all()), "the tail rows are left to the consumer"
    if S:
        base = 1024 if tick else 0
        slabs = wsb[base:base + S * (M - row0) * N].view(S, M - row0, N)
        _note("8phase_slabs", G.check_f32(slabs.double().sum(0), ref[row0:], T[row0:], G.TAU_BF16_MFMA, what="sum of tail slabs"))
        nt = K // 64
        per = -(-nt // S)
        for s in range(S):
            k0, k1 = s * per * 64, min(K, (s + 1) * per * 64)
            r, t, _ = G.reference(A[row0:, k0:k1], B[:, k0:k1])
            G.check_f32(slabs[s], r, t, G.TAU_BF16_MFMA, what=f"tail slab {s} of {S}")


# ------------------------------------------------------------------------------------------ SwiGLU epilogues
def _il_split(gu):
    """interleaved-32 gate|up [M, N] -> gate, up [M, N/2]"""
    M, N = gu.shape
    v = gu.view(M, N // 64, 2, 32)
    return v[:, :, 0].reshape(M, N // 2), v[:, :, 1].reshape(M, N // 2)


SWIGLU = [("8phase", 0, 4096, 2048, 2048, None, 0), ("8phase", 0, 4097, 2304, 2112, "ws", 35), ("tall", 2, 2824, 3072, 2048, None, 0),
          ("split", 1, 5536, 22016, 2048, "ws", 0)]


@pytest.mark.parametrize("form,mode,M,N,K,ws,sk", SWIGLU)
def test_swiglu_forward(ops, tall, form, mode, M, N, K, ws, sk):
    tall(mode)
    Al, Bl = G.bench_like(M, N, K)
    A, B = operand(Al, BF), operand(Bl, BF)
    gu, act = Window(M, N, BF), Window(M, N // 2, BF)
    wsb, tick = workspace(ws)
    d = desc(ops, A, B, gu.view, M, N, K, ws=wsb, tickets=tick, split_k=sk, epilogue=1, C2=act.view)
    route = launch(ops, d)
    assert route[0] == form, route
    assert gu.guards_intact() and act.guards_intact()
    ref, T, _ = G.reference(A, B)
    _note(form + "_swiglu", G.check_bf16(gu.view, ref, T, G.TAU_BF16_MFMA, what="gate|up"))
    # the kernel rounds silu(gate) to bf16 before the product (HF's bf16 arithmetic): got = RNE(a u), a one of the bf16 neighbours of silu(g)
    g, u = _il_split(gu.view.double())
    a = g * torch.sigmoid(g)
    alo, ahi = G.bracket(a - G.RHO_SILU * a.abs(), a + G.RHO_SILU * a.abs())
    lo, hi = G.bracket(torch.minimum(alo * u, ahi * u), torch.maximum(alo * u, ahi * u))
    got = act.view.double()
    bad = ~((lo <= got) & (got <= hi))
    assert not bool(bad.any()), f"silu(gate) up: {int(bad.sum())} elements outside the bracket, first {bad.nonzero()[:3].tolist()}"
    want = torch.empty(M, N // 2, dtype=BF, device=DEV)
    ops.swiglu_il(gu.view, want)
    assert torch.equal(want, act.view)


@pytest.mark.parametrize("form,mode,M,N,K,ws,sk", [("8phase", 0, 4096, 2048, 2048, None, 0), ("8phase", 0, 4097, 2304, 2112, "ws", 35),
                                                   ("tall", 2, 2824, 3072, 2048, None, 0), ("split", 1, 5536, 11008, 2048, "ws", 0)])
def test_swiglu_backward(ops, tall, form, mode, M, N, K, ws, sk):
    """the product is d(act) [M, N]; C = d(gate|up) [M, 2N] from the kernel's bf16-rounded d(act) pushed through SwiGLU's derivative."""
    tall(mode)
    Al, Bl = G.bench_like(M, N, K)
    A, B = operand(Al, BF), operand(Bl, BF)
    gu = operand(torch.randn(M, 2 * N, generator=torch.Generator().manual_seed(5)), BF)
    dgu = Window(M, 2 * N, BF)
    wsb, tick = workspace(ws)
    d = desc(ops, A, B, dgu.view, M, N, K, ws=wsb, tickets=tick, split_k=sk, epilogue=3, C2=gu)
    route = launch(ops, d)
    assert route[0] == form, route
    assert dgu.guards_intact()
    dref, T, _ = G.reference(A, B)
    delta = G.TAU_BF16_MFMA * T + 2.0 ** -8 * (dref.abs() + G.TAU_BF16_MFMA * T)    # the kernel's bf16 rounding of d(act)
    g, u = _il_split(gu.double())
    sig = torch.sigmoid(g)
    dsg = sig * (1.0 + g * (1.0 - sig))                                            # silu'(g)
    rg, ru = dref * u * dsg, dref * g * sig
    # silu'(g) cancels near g = -1.28: its fp32 error is relative to the magnitude of its terms, sigma (1 + |g|)
    bg = (u * dsg).abs() * delta + G.RHO_SILU * ((dref * u).abs() * sig * (1.0 + g.abs()) + rg.abs())
    bu = (g * sig).abs() * delta + G.RHO_SILU * ru.abs()
    og, ou = _il_split(dgu.view.double())
    z = torch.zeros_like(rg)
    G.check_bf16(og, rg, z, 0.0, bg, what="d gate")
    G.check_bf16(ou, ru, z, 0.0, bu, what="d up")
    dact = torch.empty(M, N, dtype=BF, device=DEV)                          # the same route without the epilogue: the same bits
    launch(ops, desc(ops, A, B, dact, M, N, K, ws=wsb, tickets=tick, split_k=sk))
    want = torch.empty(M, 2 * N, dtype=BF, device=DEV)
    ops.swiglu_il_bwd(dact, gu, want)
    assert torch.equal(want, dgu.view)


# ------------------------------------------------------------------------------------------ k-major (gemm_tn.hip)
KMAJOR = [  # M, N, K, a_layout, out, ws, col_off, mode, form, tail
    (2048, 2048, 5508, 1, F32, None, 0, -1, "kmajor", False), (2048, 2056, 5564, 1, BF, "ws", 8, -1, "kmajor", None),
    (2304, 2048, 4100, 1, F32, "ws", 16, -1, "kmajor", None), (4096, 4104, 1280, 1, F32, "ws", 0, -1, "kmajor", None),
    (32008, 4096, 1280, 1, F32, "ws", 0, -1, "kmajor", None),
    (2048, 2048, 2048, 0, BF, None, 8, 0, "kmajor", False), (4097, 4096, 4096, 0, BF, "ws", 0, 0, "kmajor", None),
    (5536, 4096, 4096, 0, BF, "ws", 0, -1, "kmajor_tall", False), (5536, 11008, 2048, 0, BF, "ws", 0, -1, "kmajor_split", None),
]


@pytest.mark.parametrize("M,N,K,la,out,ws,off,mode,form,tail", KMAJOR)
def test_kmajor_forms(ops, tall, M, N, K, la, out, ws, off, mode, form, tail):
    """weight gradients (a_layout = b_layout = 1, fp32 and bf16 output, ragged K: K % 64 in {4, 60}, padded logits) and data gradients
    (a_layout 0, b_layout 1), operands as column slices, NaN in the 64 rows past K of every k-major allocation."""
    if mode >= 0:
        tall(mode)
    fams = ("exact", "cancel") if M * N * K <= 40e9 else ("bench",)
    for fam in fams:
        run_case(ops, M, N, K, fam=fam, a_layout=la, b_layout=1, out=out, ws_kind=ws, col_off=off, kmajor_pad=64, form=form, tail=tail,
                 na=True if form == "kmajor_split" else None)
    if out == F32:
        run_case(ops, M, N, K, fam="exact", a_layout=la, b_layout=1, out=F32, epi=("accumulate",), ws_kind=ws, kmajor_pad=64, form=form)


# ------------------------------------------------------------------------------------------ census
def test_census_every_form_code_is_reached(ops, tall):
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egomi.h")).read()
    n = int(re.search(r"#define EGOMI_ROUTE_FORMS (\d+)", txt).group(1))
    assert sorted(ops.GEMM_FORMS) == list(range(n))
    reps = [  # form, kwargs
        ("generic", dict(M=100, N=70, K=50)), ("128x128", dict(M=600, N=520, K=1024)), ("256x128", dict(M=2048, N=8192, K=512)),
        ("gemv_m16", dict(M=8, N=4096, K=1024)), ("m256", dict(M=200, N=8192, K=1024)),
        ("8phase", dict(M=4096, N=2048, K=2048, mode=0)), ("persistent", dict(M=4096, N=2048, K=2048, ws_kind="persist", mode=0)),
        ("tall", dict(M=2816, N=3072, K=2048, mode=2)), ("split", dict(M=5536, N=11008, K=2048, ws_kind="ws", mode=1)),
        ("kmajor", dict(M=2048, N=2048, K=2048, a_layout=1, b_layout=1)),
        ("kmajor_tall", dict(M=5536, N=4096, K=2048, b_layout=1, ws_kind="ws", mode=1)),
        ("kmajor_split", dict(M=5536, N=11008, K=2048, b_layout=1, ws_kind="ws", mode=1)),
    ]
    seen = {"none"}
    for form, kw in reps:
        kw = dict(kw)
        tall(kw.pop("mode", -1))
        M, N, K = kw.pop("M"), kw.pop("N"), kw.pop("K")
        route = run_case(ops, M, N, K, fam="exact", form=form, repeat=False, **kw)[0]
        seen.add(route[0])
    assert seen == set(ops.GEMM_FORMS.values()), sorted(set(ops.GEMM_FORMS.values()) - seen)
