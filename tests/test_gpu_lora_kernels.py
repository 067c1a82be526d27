"""GPU: the LoRA kernels of csrc/lora.hip against torch restatements: ragged M, every supported r, stacked adapters, the interleaved-32
gate|up column map, transposed operands, operands at the very end of their allocations, repeated calls bit-equal, bad arguments."""
import ctypes

import pytest
import torch

from egoscaler_amd import ops
from egoscaler_amd._lib import EgomiError

pytestmark = pytest.mark.gpu
TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}


def _il_cols(n):
    c = torch.arange(n)
    return 64 * (c // 32) + c % 32


SEG = 2 << 20
_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def _tail(shape, dtype, g):
    """Random values in a tensor whose last byte is the last byte of a device allocation of its own (>= 16 MB, a multiple of 2 MB,
    requested from an empty cache: the test_gpu_bounds.py pattern).  Every operand of every test here is placed so."""
    src = torch.randn(shape, generator=g).to(dtype)
    n, es = src.numel(), src.element_size()
    nbytes = max(16 << 20, -(-n * es // SEG) * SEG)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    buf = torch.empty(nbytes // es, dtype=dtype, device="cuda")
    _KEEP.append(buf)
    t = buf[buf.numel() - n:].view(shape)
    t.copy_(src)
    return t


def _close(a, b, dtype):
    err = float((a.float() - b.float()).abs().max())
    ref = float(b.float().abs().max()) + 1e-6
    assert err <= TOL[dtype] * ref, (err, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("r", [8, 16, 24, 32, 40, 48, 56, 64])
@pytest.mark.parametrize("M", [1, 37, 300])
def test_down_up_every_r(dtype, r, M):
    g = torch.Generator().manual_seed(r * 1000 + M)
    K, N = {1: 200, 37: 1024, 300: 1100}[M], 136     # K % 32 != 0: the fp32-FMA form; 1024 (bf16): the MFMA form; > 512: K slices in order
    x, A, B = _tail((M, K), dtype, g), _tail((r, K), dtype, g), _tail((N, r), dtype, g)
    T = torch.empty(M, r, dtype=dtype, device="cuda")
    ops.lora_down(x, A, T)
    _close(T, x.float() @ A.float().t(), dtype)
    y0 = _tail((M, N), dtype, g)
    y = y0.clone()
    ops.lora_up(T, B, y, 0.5)
    _close(y, y0.float() + 0.5 * T.float() @ B.float().t(), dtype)
    U = torch.empty(M, r, dtype=dtype, device="cuda")
    ops.lora_down(y0, B, U, q_trans=True)                                     # U = dY B
    _close(U, y0.float() @ B.float(), dtype)
    dx0 = _tail((M, K), dtype, g)
    dx = dx0.clone()
    ops.lora_up(U, A, dx, 2.0, q_trans=True)                                  # dX += s U A
    _close(dx, dx0.float() + 2.0 * U.float() @ A.float(), dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stacked_and_interleaved(dtype):
    g = torch.Generator().manual_seed(1)
    M, K, F, r = 77, 128, 96, 16
    x = _tail((M, K), dtype, g)
    Acat = _tail((3 * r, K), dtype, g)
    T = torch.empty(M, 3 * r, dtype=dtype, device="cuda")
    ops.lora_down(x, Acat, T)                                                 # three adapters that share x: one pass
    _close(T, x.float() @ Acat.float().t(), dtype)
    gu0 = _tail((M, 2 * F), dtype, g)                                         # interleaved-32 gate|up
    gu = gu0.clone()
    Bg, Bu = _tail((F, r), dtype, g), _tail((F, r), dtype, g)
    ops.lora_up(T[:, :r], Bg, gu, 1.5, il=True)
    ops.lora_up(T[:, r:2 * r], Bu, gu[:, 32:], 1.5, il=True)
    ref = gu0.float().clone()
    c = _il_cols(F).cuda()
    ref[:, c] += 1.5 * T[:, :r].float() @ Bg.float().t()
    ref[:, c + 32] += 1.5 * T[:, r:2 * r].float() @ Bu.float().t()
    _close(gu, ref, dtype)
    U = torch.empty(M, r, dtype=dtype, device="cuda")
    ops.lora_down(gu0[:, 32:], Bu, U, q_trans=True, il=True)
    _close(U, gu0.float()[:, c + 32] @ Bu.float(), dtype)
    G = torch.zeros(F, r, dtype=torch.float32, device="cuda")
    ops.lora_wgrad(gu0[:, 32:], T[:, r:2 * r], G, 0.5, il=True, Pd=F)
    _close(G, 0.5 * gu0.float()[:, c + 32].t() @ T[:, r:2 * r].float(), torch.float32 if dtype == torch.float32 else dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [5, 256, 257, 1000])
def test_wgrad_overwrite_accumulate_and_bits(dtype, M):
    g = torch.Generator().manual_seed(M)
    r, K, N = 16, 300, 200
    U, x = _tail((M, r), dtype, g), _tail((M, K), dtype, g)
    dY, T = _tail((M, N), dtype, g), _tail((M, r), dtype, g)
    dA = torch.full((r, K), float("nan"), device="cuda")
    ops.lora_wgrad(U, x, dA, 0.25)                                            # overwrite: NaN in the buffer must not survive
    _close(dA, 0.25 * U.float().t() @ x.float(), torch.float32)
    first = dA.clone()
    ops.lora_wgrad(U, x, dA, 0.25, accumulate=True)
    _close(dA, 2 * first, torch.float32)
    dB = torch.zeros(N, r, device="cuda")
    ops.lora_wgrad(dY, T, dB, 1.0)
    _close(dB, dY.float().t() @ T.float(), torch.float32)
    again = torch.zeros(N, r, device="cuda")
    ops.lora_wgrad(dY, T, again, 1.0)
    assert torch.equal(dB, again)                                             # fixed order, no atomics
    T2 = torch.empty(M, r, dtype=dtype, device="cuda")
    T3 = torch.empty(M, r, dtype=dtype, device="cuda")
    ops.lora_down(x, _tail((r, K), dtype, torch.Generator().manual_seed(9)), T2)
    ops.lora_down(x, _tail((r, K), dtype, torch.Generator().manual_seed(9)), T3)
    assert torch.equal(T2, T3)


def test_merge_rounds_once():
    g = torch.Generator().manual_seed(3)
    N, K, r = 96, 160, 8
    W, A, B = _tail((N, K), torch.bfloat16, g), _tail((r, K), torch.bfloat16, g), _tail((N, r), torch.bfloat16, g)
    out = W.clone()
    ops.lora_up(B, A, out, 2.0, q_trans=True)
    ref = (W.float() + 2.0 * (B.float() @ A.float())).to(torch.bfloat16)
    d = (out.float() - ref.float()).abs()
    assert float(d.max()) <= float(ref.float().abs().max()) * 2 ** -8       # at most one bf16 ulp apart (fp32 sum order)
    assert float((out != ref).float().mean()) < 0.01


def _raw(name, *args):
    from egoscaler_amd import _lib
    return getattr(_lib.lib(), name)(*args)


def test_bad_arguments():
    c_p, c_i, c_f, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    p = c_p(x.data_ptr())
    s = c_p(torch.cuda.current_stream().cuda_stream)
    down = lambda R, il=0, dtype=1, K=64: _raw("egomi_lora_down", p, c_i64(128), p, c_i64(64), c_i(0), p, c_i64(64), c_i(4), c_i(K), c_i(R),
                                                c_f(1.0), c_i(il), c_p(None), c_i64(0), c_i(dtype), s)
    up = lambda R, il=0, N=64: _raw("egomi_lora_up", p, c_i64(64), p, c_i64(64), c_i(0), p, c_i64(128), c_i(4), c_i(N), c_i(R), c_f(1.0),
                                    c_i(il), c_i(1), s)
    assert down(12) == -4 and down(4) == -4 and down(200) == -4 and down(8, dtype=2) == -4 and down(8, il=1, K=48) == -4
    assert up(12) == -4 and up(8, il=1, N=48) == -4
    assert down(8) == 0 and up(8) == 0
    assert down(8, K=600) == -2                                              # two K slices need a workspace
    assert _raw("egomi_lora_down", c_p(None), c_i64(64), p, c_i64(64), c_i(0), p, c_i64(64), c_i(4), c_i(64), c_i(8), c_f(1.0), c_i(0),
                c_p(None), c_i64(0), c_i(1), s) == -1
    w = lambda P, Q: _raw("egomi_lora_wgrad", p, c_i64(4096), p, c_i64(4096), p, c_i64(4096), c_i(4), c_i(P), c_i(Q), c_f(1.0), c_i(0),
                          c_i(0), c_p(None), c_i64(0), c_i(1), s)
    assert w(256, 256) == -4                                                 # not a LoRA shape: both sides wide
    with pytest.raises(ValueError):
        ops.lora_down(x, x[:8].float(), torch.empty(64, 8, device="cuda"))
    with pytest.raises(EgomiError):
        ops.lora_down(x, x[:12], torch.empty(64, 12, dtype=torch.bfloat16, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K", [96, 1056])
def test_widest_call_r192(dtype, K):
    """R = 192: three stacked adapters of r = 64, the widest lora_down / lora_up the engine issues (lora_up then needs > 64 KiB of LDS)."""
    g = torch.Generator().manual_seed(K)
    M, R = 301, 192
    x, A, U = _tail((M, K), dtype, g), _tail((R, K), dtype, g), _tail((M, R), dtype, g)
    T = torch.empty(M, R, dtype=dtype, device="cuda")
    ops.lora_down(x, A, T)
    _close(T, x.float() @ A.float().t(), dtype)
    dx0 = _tail((M, K), dtype, g)
    dx = dx0.clone()
    ops.lora_up(U, A, dx, 0.25, q_trans=True)
    _close(dx, dx0.float() + 0.25 * U.float() @ A.float(), dtype)


def test_wrapper_rejects_short_operands():
    x = torch.zeros(10, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        ops.lora_down(x, torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda"), torch.empty(12, 8, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        ops.lora_down(x, torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda"), torch.empty(10, 8, dtype=torch.bfloat16, device="cuda"), il=True)
    with pytest.raises(ValueError):
        ops.lora_up(torch.zeros(10, 8, dtype=torch.bfloat16, device="cuda"), torch.zeros(64, 8, dtype=torch.bfloat16, device="cuda"), x[:, :32], 1.0)
    with pytest.raises(ValueError):
        ops.lora_wgrad(x[:, :16], torch.zeros(10, 8, dtype=torch.bfloat16, device="cuda"), torch.zeros(64, 8, device="cuda"), 1.0)
