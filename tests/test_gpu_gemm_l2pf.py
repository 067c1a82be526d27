"""GPU: the L2 touches of the 352x256 and the 256x256 per-tile GEMM kernels (csrc/gemm_fast.hip FastArgs::l2pf, egomi_gemm_set_l2_prefetch) change no bit.

The touches read cache lines a few K-tiles ahead of the LDS-DMA ring and throw the data away; what they cost or break can only be the counted vmcnt
waits of the two kernels (a wait that lets a fragment read overtake its DMA shows as wrong numbers) — so every output of a launch at distance
D in {1, 4, 8} must equal, bit for bit, the output at D = 0, where the kernels run the code they ran before the feature.  Shapes are the smallest that
reach each path (egomi_gemm_set_tile(8) sends products of a few tiles to the 256-row forms; the route of every launch is asserted):
  * 352x256 form (egomi_gemm_set_tall(2)), K = 2048 (32 K-tiles): M = 360 = two tile rows, the second one ragged; N = 264 (ragged column tile) and 256
  * its k-major B instantiation: the smallest product gemm_tn.hip hands to it (>= 64 tiles of 256x256)
  * 256x256 form: M = N = 264 (2 x 2 ragged tiles) at K = 128 and 192 = 2 and 3 K-tiles, so that every D lies beyond the last tile; whole tiles, and the
    second tile row cut into 2 K-slices (one K-tile and one or two per block)
each with bf16 and fp32 output and with every epilogue its form takes: plain, residual, EGOMI_EPI_SLABS, SwiGLU, SwiGLU backward (the fused ones need
N % 256 == 0: N = 256).  Where the touches may read is tests/test_gemm_l2pf_host.py's subject; here every operand lies in the interior of a larger
allocation (8 rows above and below, 32 columns left and right), so that this test could not read outside anything even if that rule were off by a row."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DISTANCES = (1, 4, 8)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from egoscaler_amd import ops as O
    return O


@pytest.fixture()
def knobs(ops):
    """setters of the three process-wide switches; all three are restored whatever the test did"""
    from egoscaler_amd import _lib
    L = _lib.lib()

    def set_all(tile, tall):
        assert L.egomi_gemm_set_tile(ctypes.c_int(tile)) == 0
        assert L.egomi_gemm_set_tall(ctypes.c_int(tall)) == 0
    try:
        yield set_all, (lambda d: L.egomi_gemm_set_l2_prefetch(ctypes.c_int(d)))
    finally:
        L.egomi_gemm_set_l2_prefetch(ctypes.c_int(-1))
        L.egomi_gemm_set_tall(ctypes.c_int(-1))
        L.egomi_gemm_set_tile(ctypes.c_int(-1))


def interior(rows, cols, dtype, seed, scale=1.0, fill=None):
    """[rows, cols] view in the interior of a larger allocation whose every element is finite -> (view, whole buffer)"""
    g = torch.Generator().manual_seed(seed)
    buf = (torch.randn(rows + 16, cols + 64, generator=g) * scale).to(dtype).cuda() if fill is None else \
        torch.full((rows + 16, cols + 64), fill, dtype=dtype, device="cuda")
    return buf[8:8 + rows, 32:32 + cols], buf


def run(ops, A, B, M, N, K, *, out, epi, b_layout=0, ws_bytes=0, split_k=0):
    """one egomi_gemm -> (route, [every buffer the launch may have written])"""
    from egoscaler_amd import _lib
    d = ops.GemmDesc()
    wide = 2 * N if epi == "swiglu_bwd" else N                       # SwiGLU backward: C = d(gate|up) [M, 2N]
    C, Cbuf = interior(M, wide, out, 0, fill=3.0)
    outs = [Cbuf]
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = A.stride(0), B.stride(0), C.stride(0)
    d.a_layout, d.b_layout, d.ab_dtype, d.c_dtype, d.batch, d.batch_inner, d.alpha = 0, b_layout, ops.dt(BF), ops.dt(out), 1, 1, 1.0
    keep = []
    if epi == "residual":
        R, rb = interior(M, N, out, 5)
        d.residual, d.ldr = R.data_ptr(), R.stride(0)
        keep.append(rb)
    elif epi == "slabs":
        d.epilogue = 2
    elif epi == "swiglu":
        C2, c2b = interior(M, N // 2, BF, 0, fill=3.0)
        d.epilogue, d.C2, d.ldc2 = 1, C2.data_ptr(), C2.stride(0)
        outs.append(c2b)
    elif epi == "swiglu_bwd":
        GU, gub = interior(M, 2 * N, BF, 6)
        d.epilogue, d.C2, d.ldc2 = 3, GU.data_ptr(), GU.stride(0)
        keep.append(gub)
    if ws_bytes:
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        d.workspace, d.workspace_bytes, d.split_k = ws.data_ptr(), ws_bytes, split_k
        outs.append(ws)
    _lib.check(_lib.lib().egomi_gemm(ctypes.byref(d), ops.S()), "egomi_gemm")
    route = ops.gemm_last_route()
    torch.cuda.synchronize()
    return route, outs


def same_bits_at_every_distance(ops, set_d, M, N, K, form, tail, **kw):
    b_layout = kw.get("b_layout", 0)
    A, _a = interior(M, K, BF, 1)
    B, _b = interior(K, N, BF, 2, scale=0.05) if b_layout else interior(N, K, BF, 2, scale=0.05)
    set_d(0)
    route0, want = run(ops, A, B, M, N, K, **kw)
    assert route0[0] == form and (route0[3] > 0) == tail, route0
    assert bool((want[0][8:8 + M, 32:32 + N].float() != 3.0).any()), "the launch wrote its output"
    for D in DISTANCES:
        set_d(D)
        route, got = run(ops, A, B, M, N, K, **kw)
        assert route == route0, (D, route, route0)                  # the distance is no part of the route
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), f"D = {D}: buffer {i} differs from D = 0"


TALL_EPIS = [(264, BF, "plain"), (264, F32, "plain"), (264, BF, "residual"), (264, F32, "residual"), (264, BF, "slabs"),
             (256, BF, "plain"), (256, F32, "plain"), (256, BF, "residual"), (256, F32, "residual"), (256, BF, "slabs"),
             (256, BF, "swiglu"), (256, BF, "swiglu_bwd")]


@pytest.mark.parametrize("N,out,epi", TALL_EPIS)
def test_tall_form_same_bits(ops, knobs, N, out, epi):
    set_all, set_d = knobs
    set_all(8, 2)
    same_bits_at_every_distance(ops, set_d, 360, N, 2048, "tall", False, out=out, epi=epi)


def test_tall_form_k_major_same_bits(ops, knobs):
    set_all, set_d = knobs
    set_all(-1, 2)
    same_bits_at_every_distance(ops, set_d, 2824, 1536, 2048, "kmajor_tall", False, out=BF, epi="plain", b_layout=1)


P8_EPIS = [(264, BF, "plain"), (264, F32, "plain"), (264, BF, "residual"), (264, F32, "residual"), (264, BF, "slabs"),
           (256, BF, "swiglu"), (256, BF, "swiglu_bwd")]


@pytest.mark.parametrize("K", (128, 192))
@pytest.mark.parametrize("sliced", (False, True))
@pytest.mark.parametrize("N,out,epi", P8_EPIS)
def test_256_form_same_bits(ops, knobs, N, out, epi, sliced, K):
    set_all, set_d = knobs
    set_all(8, 0)
    kw = dict(ws_bytes=8 << 20, split_k=1 * 16 + 2) if sliced else {}           # split_k = rows * 16 + S: the last tile row in 2 K-slices
    if epi == "slabs" and not sliced:
        kw = dict(ws_bytes=8 << 20, split_k=1)                                   # EGOMI_EPI_SLABS wants a scratch; split_k = 1: and no sliced rows
    same_bits_at_every_distance(ops, set_d, 264, N, K, "8phase", sliced, out=out, epi=epi, **kw)
