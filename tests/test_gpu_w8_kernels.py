"""GPU: the fp8 decode-weight kernels of csrc/w8.hip.  egomi_quantize_rows_fp8 is bit-equal to the torch restatement (decode.w8_quantize);
egomi_gemm_w8 meets the float64 product x . (code * s)^T within the bound of fp32 accumulation plus one bf16 rounding in every epilogue, its
slab count is egomi_gemm_w8_slab_count's, every operand may end an allocation, a repeated or captured launch gives the same bits, and shapes
or arguments it cannot take are refused with an error code."""
import ctypes
import types

import pytest
import torch

from egoscaler_amd import ops
from egoscaler_amd.decode import w8_quantize as _w8_quantize
from egoscaler_amd.engine import Engine
from egoscaler_amd._lib import c_i, c_i64, lib
from egoscaler_amd.ops import P, S

pytestmark = pytest.mark.gpu

SEG = 2 << 20
E_BADARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -4
U = 2.0 ** -24                                                            # fp32 unit roundoff
# 7B projections (q|k|v, o_proj, gate|up, down_proj) and the tiny model's (d = 128, ffn = 352)
SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (384, 128), (128, 128), (704, 128), (128, 352)]
MS = [1, 2, 8, 16, 32, 64, 256, 512]


def at_end(src, keep):
    """A copy of `src` whose last byte is the last byte of a fresh device allocation of its own (test_gpu_bounds.py's pattern)."""
    n, es = src.numel(), src.element_size()
    nbytes = max(16 << 20, -(-n * es // SEG) * SEG)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    buf = torch.empty(nbytes // es, dtype=src.dtype, device="cuda")
    keep.append(buf)
    t = buf[buf.numel() - n:].view(src.shape)
    t.copy_(src)
    return t


def w8_quantize(w):
    """The restatement on the host (IEEE division; torch's device division of amax / 448 is not correctly rounded), back on the device."""
    c, s = _w8_quantize(w.cpu())
    return c.to(w.device), s.to(w.device)


def _w(N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(torch.bfloat16)


def _x(M, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("K", [32, 96, 128, 352, 4096, 11008])
def test_quantize_rows_bit_equal_to_restatement(K):
    w = _w(257, K, K)
    w[3] = 0                                                              # zero row: s = 1, codes 0
    w[7] = (w[7].float() * 2.0 ** -120).to(torch.bfloat16)                # amax subnormal in bf16
    w[9, K // 2] = 300.0                                                  # one outlier: the rest flush towards subnormals
    w[11] = -w[11].abs()
    codes, s = ops.quantize_rows_fp8(w)
    rc, rs = w8_quantize(w)
    assert torch.equal(codes, rc) and torch.equal(s, rs)
    assert float(s[3]) == 1.0 and bool((codes[3] == 0).all())
    # a strided view of rows (ldw > K)
    big = _w(64, K + 64, 5)
    codes, s = ops.quantize_rows_fp8(big[:, :K])
    rc, rs = w8_quantize(big[:, :K])
    assert torch.equal(codes, rc) and torch.equal(s, rs)


def test_quantize_interleaved_gate_up_stack():
    eng = types.SimpleNamespace(gu_il=True)
    for Fd, d in ((352, 128), (11008, 4096)):
        gate, up = _w(Fd, d, 1), _w(Fd, d, 2)
        gu = Engine.stack_gate_up(eng, gate, up)
        codes, s = ops.quantize_rows_fp8(gu)
        rc, rs = w8_quantize(gu)
        assert torch.equal(codes, rc) and torch.equal(s, rs)
        c_gate, s_gate = w8_quantize(gate)                                # rows quantize on their own: interleaving moves them only
        assert torch.equal(codes.view(Fd // 32, 2, 32, d)[:, 0].reshape(Fd, d), c_gate)
        assert torch.equal(s.view(Fd // 32, 2, 32)[:, 0].reshape(Fd), s_gate)


def _ref(x, codes, s):
    """float64 y = x . (code * s)^T and the bound of fp32 accumulation in any order: (K + 2) u sum_k |x w| (scale product included)."""
    wd = codes.view(torch.float8_e4m3fn).double() * s.double()[:, None]
    xd = x.double()
    return xd @ wd.T, (x.shape[1] + 2) * U * (xd.abs() @ wd.abs().T)


def _check(y, ref, acc_bound, res=None):
    y = y.double()
    tgt = ref if res is None else ref + res.double()
    # fp32 accumulation, then (residual: one fp32 addition) and one bf16 rounding (half an ulp: 2^-8 relative)
    bound = acc_bound + (0 if res is None else U * tgt.abs()) + 2.0 ** -8 * tgt.abs() + 1e-30
    assert bool(((y - tgt).abs() <= bound).all()), float(((y - tgt).abs() / bound).max())
    assert float((y - tgt).norm() / tgt.norm()) < 1e-2


@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_w8_every_epilogue_against_float64(N, K):
    w = _w(N, K, N + K)
    codes, s = ops.quantize_rows_fp8(w)
    ws = torch.empty(128 << 20, dtype=torch.uint8, device="cuda")
    for M in MS:
        x = _x(M, K, M)
        ref, accb = _ref(x, codes, s)
        y = ops.mm_w8(x, codes, s)                                        # NONE, no workspace: no split
        _check(y, ref, accb)
        y2 = ops.mm_w8(x, codes, s, workspace=ws)                         # NONE, the planned split + ordered combine
        _check(y2, ref, accb)
        res = _x(M, N, M + 1)
        y3 = ops.mm_w8(x, codes, s, residual=res, workspace=ws)           # RESIDUAL
        _check(y3, ref, accb, res)
        n = ops.mm_w8_slabs(x, codes, s, ws)                              # SLABS
        assert n == lib().egomi_gemm_w8_slab_count(c_i(M), c_i(N), c_i(K), c_i64(ws.numel())) and n >= 1
        slabs = ws[:n * M * N * 4].view(torch.float32).view(n, M, N)
        tot = slabs[0].clone()
        for i in range(1, n):
            tot += slabs[i]
        assert bool(((tot.double() - ref).abs() <= accb * (1 + (n + 1) / (K + 2)) + 1e-30).all())      # + the n - 1 slab additions
        del slabs, tot
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K", [(8, 12288, 4096), (256, 4096, 11008), (3, 704, 352), (40, 384, 128)])
def test_gemm_w8_operands_at_the_end_of_their_allocations(M, N, K):
    keep = []
    codes, s = ops.quantize_rows_fp8(_w(N, K, 3))
    x, res = _x(M, K, 4), _x(M, N, 5)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    y0 = ops.mm_w8(x, codes, s, residual=res, workspace=ws)
    n = ops.mm_w8_slabs(x, codes, s, ws)
    sl0 = ws[:n * M * N * 4].clone()
    xe, ce, se, re_ = at_end(x, keep), at_end(codes, keep), at_end(s, keep), at_end(res, keep)
    oe = at_end(torch.zeros(M, N, dtype=torch.bfloat16, device="cuda"), keep)
    wse = at_end(torch.zeros(n * M * N * 4, dtype=torch.uint8, device="cuda"), keep)     # exactly the slabs' bytes: the same plan
    assert ops.mm_w8_slabs(xe, ce, se, wse, count_only=True) == n
    ops.mm_w8(xe, ce, se, out=oe, residual=re_, workspace=wse)
    assert torch.equal(oe, y0)
    assert ops.mm_w8_slabs(xe, ce, se, wse) == n
    assert torch.equal(wse, sl0)
    torch.cuda.synchronize()


def test_gemm_w8_repeated_and_captured_launches_are_bit_equal():
    for M, N, K in ((8, 4096, 11008), (256, 12288, 4096), (5, 128, 352)):
        codes, s = ops.quantize_rows_fp8(_w(N, K, 6))
        x = _x(M, K, 7)
        ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        ops.mm_w8(x, codes, s, out=out, workspace=ws)
        a = out.clone()
        n = ops.mm_w8_slabs(x, codes, s, ws)
        sa = ws[:n * M * N * 4].clone()
        for _ in range(3):
            ops.mm_w8(x, codes, s, out=out, workspace=ws)
            assert torch.equal(out, a)
            ops.mm_w8_slabs(x, codes, s, ws)
            assert torch.equal(ws[:n * M * N * 4], sa)
        out.zero_()
        ws.zero_()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                ops.mm_w8(x, codes, s, out=out, workspace=ws)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


def test_gemm_w8_bad_shapes_and_arguments_are_refused():
    L = lib()
    L.egomi_gemm_w8.restype = ctypes.c_int
    M, N, K = 4, 128, 128
    x = torch.zeros(600, 256, dtype=torch.bfloat16, device="cuda")
    codes = torch.zeros(256, 256, dtype=torch.uint8, device="cuda")
    s = torch.ones(256, device="cuda")
    out = torch.zeros(600, 256, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    nul = ctypes.c_void_p(None)

    def call(xp=P(x), ldx=256, cp=P(codes), ldw=256, sp=P(s), op=P(out), ldo=256, rp=nul, ldr=0, M_=M, N_=N, K_=K, epi=0, wp=P(ws), wb=ws.numel()):
        r = L.egomi_gemm_w8(xp, c_i64(ldx), cp, c_i64(ldw), sp, op, c_i64(ldo), rp, c_i64(ldr), c_i(M_), c_i(N_), c_i(K_), c_i(epi), wp, c_i64(wb), S())
        torch.cuda.synchronize()
        return r
    assert call() == 0 and call(epi=2) == 0
    assert call(M_=513) == E_UNSUPPORTED                                  # more rows than the decode bound
    assert call(N_=66) == E_UNSUPPORTED                                   # N % 4
    assert call(K_=100) == E_UNSUPPORTED                                  # K % 32
    assert call(epi=1) == E_UNSUPPORTED                                   # no SwiGLU epilogue here
    assert call(M_=0) == E_SHAPE and call(K_=0) == E_SHAPE
    assert call(ldx=64) == E_SHAPE and call(ldw=64) == E_SHAPE and call(ldo=64) == E_SHAPE
    assert call(ldw=136) == E_SHAPE                                       # code rows must stay 16-B aligned
    assert call(xp=ctypes.c_void_p(x.data_ptr() + 2)) == E_SHAPE
    for kw in (dict(xp=nul), dict(cp=nul), dict(sp=nul), dict(op=nul), dict(epi=2, wp=nul), dict(epi=2, rp=P(out), ldr=256)):
        assert call(**kw) == E_BADARG, kw
    assert call(epi=2, wb=M * N * 4 - 1) == E_UNSUPPORTED                 # not one slab fits
    sc = lambda M_, N_, K_, wb: L.egomi_gemm_w8_slab_count(c_i(M_), c_i(N_), c_i(K_), c_i64(wb))
    assert sc(513, 128, 128, 1 << 20) == 0 and sc(4, 66, 128, 1 << 20) == 0 and sc(4, 128, 100, 1 << 20) == 0 and sc(4, 128, 128, 100) == 0
    assert sc(4, 128, 128, 1 << 20) >= 1
    L.egomi_quantize_rows_fp8.restype = ctypes.c_int
    q = lambda wp=P(x), ldw=256, N_=4, K_=128, cp=P(codes), ldc=256, sp=P(s): L.egomi_quantize_rows_fp8(wp, c_i64(ldw), c_i(N_), c_i(K_), cp, c_i64(ldc), sp, S())
    assert q() == 0
    assert q(wp=nul) == E_BADARG and q(cp=nul) == E_BADARG and q(sp=nul) == E_BADARG
    assert q(N_=0) == E_SHAPE and q(ldw=64) == E_SHAPE and q(ldc=64) == E_SHAPE
    torch.cuda.synchronize()
