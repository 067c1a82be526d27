"""GPU: the int4 decode-weight kernels of csrc/w4.hip.  egomi_quantize_rows_int4 is bit-equal to the torch restatement run on the host
(decode.w4_quantize); egomi_gemm_w4 is EXACT where every partial sum is exact in fp32 (integer activations, weights that are codes times a
power of two per group), meets the float64 product of the dequantized weights within the bound of fp32 accumulation plus one bf16 rounding
on random values, in every epilogue; its slab count is egomi_gemm_w4_slab_count's, every operand may end an allocation, a repeated or
captured launch gives the same bits, and shapes or arguments it cannot take are refused with egomi_gemm_w8's error codes."""
import ctypes
import types

import pytest
import torch

from egoscaler_amd import ops
from egoscaler_amd.decode import w4_dequantize, w4_quantize as _w4_quantize, w4_unpack
from egoscaler_amd.engine import Engine
from egoscaler_amd._lib import c_i, c_i64, call, lib
from egoscaler_amd.ops import P, S
from tests.test_gpu_w8_kernels import E_BADARG, E_SHAPE, E_UNSUPPORTED, U, _check, _w, _x, at_end

pytestmark = pytest.mark.gpu

# (N, K): one ragged group; N % 64 != 0 with a 96-wide group; one full tile and group; a 32-wide last group past a full one; the tiny
# model's down_proj (two groups + 96); several tiles and groups
SMALL = [(4, 32), (60, 96), (64, 128), (68, 160), (704, 352), (384, 1024)]
BIG = [(4096, 4096), (4096, 11008)]                                       # 7B o_proj and down_proj, M = 8 only
MS = [1, 3, 16, 17, 40]


def w4_quantize(w):
    """The restatement on the host (IEEE division), back on the device."""
    c, s = _w4_quantize(w.cpu())
    return c.to(w.device), s.to(w.device)


def _ws():
    return torch.empty(64 << 20, dtype=torch.uint8, device="cuda")


def _slab_sum(ws, n, M, N):
    slabs = ws[:n * M * N * 4].view(torch.float32).view(n, M, N)
    tot = slabs[0].clone()
    for i in range(1, n):
        tot += slabs[i]
    return tot


# ---------------------------------------------------------------------------------------------------- quantizer
@pytest.mark.parametrize("N", [4, 68])
@pytest.mark.parametrize("K", [32, 96, 128, 160, 352, 4096, 11008])
def test_quantize_rows_bit_equal_to_restatement(N, K):
    w = _w(N, K, N + K)
    w[1] = 0                                                              # zero row: every scale 1, every code 0
    w[2, K // 2] = 300.0                                                  # one outlier: the rest of its group rounds to code 0
    w[3] = -w[3].abs()
    w[0, :32] = 0                                                         # zeros inside a group
    packed, s = ops.quantize_rows_int4(w)
    rp, rs = w4_quantize(w)
    assert packed.shape == (N, K // 2) and s.shape == (-(-K // 128), N)
    assert torch.equal(packed, rp) and torch.equal(s, rs)
    assert bool((s[:, 1] == 1.0).all()) and bool((w4_unpack(packed, K)[1] == 0).all())
    big = _w(N, K + 64, 5)                                                # a strided view of rows (ldw > K)
    packed, s = ops.quantize_rows_int4(big[:, :K])
    rp, rs = w4_quantize(big[:, :K])
    assert torch.equal(packed, rp) and torch.equal(s, rs)


def test_quantize_interleaved_gate_up_stack():
    eng = types.SimpleNamespace(gu_il=True)
    for Fd, d in ((352, 128), (11008, 4096)):
        gate, up = _w(Fd, d, 1), _w(Fd, d, 2)
        gu = Engine.stack_gate_up(eng, gate, up)
        packed, s = ops.quantize_rows_int4(gu)
        rp, rs = w4_quantize(gu)
        assert torch.equal(packed, rp) and torch.equal(s, rs)
        p_gate, s_gate = w4_quantize(gate)                                # rows quantize on their own: interleaving moves rows and scale columns
        assert torch.equal(packed.view(Fd // 32, 2, 32, d // 2)[:, 0].reshape(Fd, d // 2), p_gate)
        assert torch.equal(s.view(-1, Fd // 32, 2, 32)[:, :, 0].reshape(-1, Fd), s_gate)


# ---------------------------------------------------------------------------------------------------- exact case
def _exact_case(M, N, K, seed):
    """x: integers in [-4, 4].  W = code * 2^e with e in {-3 .. 0} per (row, group) and a +-7 in every group, so s = 2^e exactly and the
    codes are W / s.  Every product and partial sum is a multiple of 2^-3 below 4 * 7 * 11008 < 2^19: at most 22 bits, exact in fp32 in
    any order.  The residual is a multiple of 2^-3 too, so the fp32 sum with it is exact and only the bf16 rounding remains."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    NG = -(-K // 128)
    rows = torch.arange(N, device="cuda")
    code = torch.randint(-7, 8, (N, K), generator=g, device="cuda")
    for gi in range(NG):                                                  # amax 7 in every group
        k0, k1 = 128 * gi, min(K, 128 * gi + 128)
        col = torch.randint(k0, k1, (N,), generator=g, device="cuda")
        code[rows, col] = torch.where(torch.rand(N, generator=g, device="cuda") < 0.5, -7, 7)
    e = torch.randint(-3, 1, (N, NG), generator=g, device="cuda")
    sc = torch.exp2(e.double())
    w = code.double() * sc.repeat_interleave(128, 1)[:, :K]
    x = torch.randint(-4, 5, (M, K), generator=g, device="cuda").double()
    res = torch.randint(-64, 65, (M, N), generator=g, device="cuda").double() / 8
    return x, w, code, sc, res


def _run_exact(M, N, K, ws):
    x64, w64, code, sc, res64 = _exact_case(M, N, K, 1000 * M + N + K)
    x, w, res = x64.to(torch.bfloat16), w64.to(torch.bfloat16), res64.to(torch.bfloat16)
    assert torch.equal(x.double(), x64) and torch.equal(w.double(), w64) and torch.equal(res.double(), res64)
    packed, s = ops.quantize_rows_int4(w)
    assert torch.equal(s.double(), sc.t()) and torch.equal(w4_unpack(packed, K).long(), code)
    ref = x64 @ w64.T
    r16, rr16 = ref.to(torch.bfloat16), (ref + res64).to(torch.bfloat16)
    assert torch.equal(ops.mm_w4(x, packed, s), r16), (M, N, K, "none")
    assert torch.equal(ops.mm_w4(x, packed, s, residual=res), rr16), (M, N, K, "residual")
    assert torch.equal(ops.mm_w4(x, packed, s, workspace=ws), r16), (M, N, K, "none + workspace")
    assert torch.equal(ops.mm_w4(x, packed, s, residual=res, workspace=ws), rr16), (M, N, K, "residual + workspace")
    n = ops.mm_w4_slabs(x, packed, s, ws)
    assert n == lib().egomi_gemm_w4_slab_count(c_i(M), c_i(N), c_i(K), c_i64(ws.numel())) and n >= 1
    assert torch.equal(_slab_sum(ws, n, M, N).double(), ref), (M, N, K, "slabs")


@pytest.mark.parametrize("N,K", SMALL)
def test_gemm_w4_exact_case_small(N, K):
    ws = _ws()
    for M in MS:
        _run_exact(M, N, K, ws)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,K", BIG)
def test_gemm_w4_exact_case_7b(N, K):
    _run_exact(8, N, K, _ws())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- random values
def _ref(x, packed, s, K):
    """float64 y = x . dequantized^T and the accumulation bound (K + NG + 2) u E, E = sum_k |x| (|code| + 16) s: fp32 accumulation in any
    order of the K products, the NG scale products and fmas; + 16 covers a kernel that multiplies the offset nibble and subtracts."""
    NG = s.shape[0]
    sf = s.t().double().repeat_interleave(128, 1)[:, :K]
    code = w4_unpack(packed, K).double()
    xd = x.double()
    return xd @ (code * sf).T, (K + NG + 2) * U * (xd.abs() @ ((code.abs() + 16) * sf).T)


@pytest.mark.parametrize("N,K", SMALL)
def test_gemm_w4_every_epilogue_against_float64(N, K):
    packed, s = ops.quantize_rows_int4(_w(N, K, N + K))
    ws = _ws()
    for M in MS + ([64, 256] if (N, K) == (384, 1024) else []):
        x = _x(M, K, M)
        ref, accb = _ref(x, packed, s, K)
        _check(ops.mm_w4(x, packed, s), ref, accb)                        # NONE, no workspace: no split
        _check(ops.mm_w4(x, packed, s, workspace=ws), ref, accb)          # NONE, the planned split + ordered combine
        res = _x(M, N, M + 1)
        _check(ops.mm_w4(x, packed, s, residual=res), ref, accb, res)
        _check(ops.mm_w4(x, packed, s, residual=res, workspace=ws), ref, accb, res)
        n = ops.mm_w4_slabs(x, packed, s, ws)                             # SLABS
        assert n == lib().egomi_gemm_w4_slab_count(c_i(M), c_i(N), c_i(K), c_i64(ws.numel())) and n >= 1
        tot = _slab_sum(ws, n, M, N)
        assert bool(((tot.double() - ref).abs() <= accb * (1 + (n + 1) / (K + 2)) + 1e-30).all())      # + the n - 1 slab additions
    torch.cuda.synchronize()


def test_dequantize_matches_unpack_times_scale():
    packed, s = ops.quantize_rows_int4(_w(68, 352, 9))
    d = w4_dequantize(packed, s, 352)
    assert d.shape == (68, 352) and float((d - _w(68, 352, 9).float()).abs().max()) <= float(s.max()) * (0.5 + 2.0 ** -21)


# ---------------------------------------------------------------------------------------------------- bounds, replay, refusals
@pytest.mark.parametrize("M,N,K", [(3, 68, 352), (40, 384, 128), (8, 4096, 11008)])
def test_gemm_w4_operands_at_the_end_of_their_allocations(M, N, K):
    keep = []
    w = _w(N, K, 3)
    packed, s = ops.quantize_rows_int4(w)
    x, res = _x(M, K, 4), _x(M, N, 5)
    ws = _ws()
    y0 = ops.mm_w4(x, packed, s, residual=res, workspace=ws)
    n = ops.mm_w4_slabs(x, packed, s, ws)
    sl0 = ws[:n * M * N * 4].clone()
    y1 = ops.mm_w4(x, packed, s, residual=res)                            # the unsplit form
    xe, pe, se, re_ = at_end(x, keep), at_end(packed, keep), at_end(s, keep), at_end(res, keep)
    oe = at_end(torch.zeros(M, N, dtype=torch.bfloat16, device="cuda"), keep)
    wse = at_end(torch.zeros(n * M * N * 4, dtype=torch.uint8, device="cuda"), keep)     # exactly the slabs' bytes: the same plan
    assert ops.mm_w4_slabs(xe, pe, se, wse, count_only=True) == n
    ops.mm_w4(xe, pe, se, out=oe, residual=re_, workspace=wse)
    assert torch.equal(oe, y0)
    ops.mm_w4(xe, pe, se, out=oe, residual=re_)
    assert torch.equal(oe, y1)
    assert ops.mm_w4_slabs(xe, pe, se, wse) == n
    assert torch.equal(wse, sl0)
    we = at_end(w, keep)                                                  # the quantizer: rows, codes and scales at the end
    pq = at_end(torch.zeros_like(packed), keep)
    sq = at_end(torch.zeros_like(s), keep)
    call("egomi_quantize_rows_int4", P(we), c_i64(K), c_i(N), c_i(K), P(pq), c_i64(K // 2), P(sq), S())
    assert torch.equal(pq, packed) and torch.equal(sq, s)
    torch.cuda.synchronize()


def test_gemm_w4_repeated_and_captured_launches_are_bit_equal():
    for M, N, K in ((8, 4096, 11008), (40, 384, 1024), (5, 128, 352)):
        packed, s = ops.quantize_rows_int4(_w(N, K, 6))
        x = _x(M, K, 7)
        ws = _ws()
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        ops.mm_w4(x, packed, s, out=out, workspace=ws)
        a = out.clone()
        n = ops.mm_w4_slabs(x, packed, s, ws)
        sa = ws[:n * M * N * 4].clone()
        for _ in range(3):
            ops.mm_w4(x, packed, s, out=out, workspace=ws)
            assert torch.equal(out, a)
            ops.mm_w4_slabs(x, packed, s, ws)
            assert torch.equal(ws[:n * M * N * 4], sa)
        out.zero_()
        ws.zero_()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                ops.mm_w4(x, packed, s, out=out, workspace=ws)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


def test_gemm_w4_bad_shapes_and_arguments_are_refused():
    L = lib()
    L.egomi_gemm_w4.restype = ctypes.c_int
    M, N, K = 4, 128, 128
    x = torch.zeros(600, 256, dtype=torch.bfloat16, device="cuda")
    codes = torch.zeros(256, 128, dtype=torch.uint8, device="cuda")
    s = torch.ones(2, 256, device="cuda")
    out = torch.zeros(600, 256, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    nul = ctypes.c_void_p(None)

    def call(xp=P(x), ldx=256, cp=P(codes), ldw=128, sp=P(s), op=P(out), ldo=256, rp=nul, ldr=0, M_=M, N_=N, K_=K, epi=0, wp=P(ws), wb=ws.numel()):
        r = L.egomi_gemm_w4(xp, c_i64(ldx), cp, c_i64(ldw), sp, op, c_i64(ldo), rp, c_i64(ldr), c_i(M_), c_i(N_), c_i(K_), c_i(epi), wp, c_i64(wb), S())
        torch.cuda.synchronize()
        return r
    assert call() == 0 and call(epi=2) == 0
    assert call(M_=513) == E_UNSUPPORTED                                  # more rows than the decode bound
    assert call(N_=66) == E_UNSUPPORTED                                   # N % 4
    assert call(K_=100) == E_UNSUPPORTED                                  # K % 32
    assert call(epi=1) == E_UNSUPPORTED                                   # no SwiGLU epilogue here
    assert call(M_=0) == E_SHAPE and call(K_=0) == E_SHAPE
    assert call(ldx=64) == E_SHAPE and call(ldw=32) == E_SHAPE and call(ldo=64) == E_SHAPE
    assert call(ldw=72) == E_SHAPE                                        # code rows must stay 16-B aligned
    assert call(xp=ctypes.c_void_p(x.data_ptr() + 2)) == E_SHAPE
    assert call(sp=ctypes.c_void_p(s.data_ptr() + 4)) == E_SHAPE          # the scales are read 16 bytes at a time
    for kw in (dict(xp=nul), dict(cp=nul), dict(sp=nul), dict(op=nul), dict(epi=2, wp=nul), dict(epi=2, rp=P(out), ldr=256)):
        assert call(**kw) == E_BADARG, kw
    assert call(epi=2, wb=M * N * 4 - 1) == E_UNSUPPORTED                 # not one slab fits
    sc = lambda M_, N_, K_, wb: L.egomi_gemm_w4_slab_count(c_i(M_), c_i(N_), c_i(K_), c_i64(wb))
    assert sc(513, 128, 128, 1 << 20) == 0 and sc(4, 66, 128, 1 << 20) == 0 and sc(4, 128, 100, 1 << 20) == 0 and sc(4, 128, 128, 100) == 0
    assert sc(4, 128, 128, 1 << 20) >= 1
    L.egomi_quantize_rows_int4.restype = ctypes.c_int
    q = lambda wp=P(x), ldw=256, N_=4, K_=128, cp=P(codes), ldc=128, sp=P(s): L.egomi_quantize_rows_int4(wp, c_i64(ldw), c_i(N_), c_i(K_), cp, c_i64(ldc), sp, S())
    assert q() == 0
    assert q(wp=nul) == E_BADARG and q(cp=nul) == E_BADARG and q(sp=nul) == E_BADARG
    assert q(N_=0) == E_SHAPE and q(ldw=64) == E_SHAPE and q(ldc=32) == E_SHAPE
    assert q(K_=100) == E_UNSUPPORTED
    torch.cuda.synchronize()
