"""CPU: the addresses of the GEMM kernels' L2 touches (csrc/gemm_fast.hip l2pf_addr; no kernel is launched, no GPU is touched).

In tile step t the 352x256 and the 256x256 per-tile kernels read 4 bytes of every 128-B line of K-tile min(t + D, last) of their A and B panels and
throw them away (egomi_gemm_set_l2_prefetch).  A wrong address there is the one way the feature can fault, and no result would show it: the data is never
used.  egomi_gemm_l2pf_span walks the rule the kernels call over every tile, wave, lane and tile step of a descriptor and reports the smallest and the
largest byte offset read in A and in B.  Every 4-byte read must lie inside the operand:
  A [M, K] row stride lda                : [0, ((M - 1) lda + K) 2)
  B [N, K] row stride ldb (b_layout 0)   : [0, ((N - 1) ldb + K) 2)
  B [K, N] row stride ldb (b_layout 1)   : [0, ((K - 1) ldb + N) 2)
for ragged tiles (M, N no multiple of the tile), one and several tiles, leading dimensions beyond the row, and distances beyond the tile count
(K = 128, 192: 2 and 3 K-tiles)."""
import ctypes
import itertools

import pytest

from egoscaler_amd import _lib
from egoscaler_amd.ops import GemmDesc, BF16

MS = (352, 360, 704, 1224, 5536)
NS = (256, 264, 4096)
KS = (128, 192, 2048, 4096)
DS = (1, 4, 8)


def desc(M, N, K, pad, b_layout):
    d = GemmDesc()
    d.A = d.B = d.C = 256
    d.M, d.N, d.K = M, N, K
    d.lda = K + pad
    d.ldb = (N if b_layout else K) + pad
    d.ldc = N
    d.a_layout, d.b_layout = 0, b_layout
    d.ab_dtype, d.c_dtype, d.batch, d.alpha = BF16, BF16, 1, 1.0
    return d


def span(d, tall, dist):
    out = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    rc = _lib.lib().egomi_gemm_l2pf_span(ctypes.byref(d), tall, dist, out)
    return rc, list(out)


@pytest.mark.parametrize("tall", (1, 0))
@pytest.mark.parametrize("b_layout", (0, 1))
def test_every_touch_reads_inside_its_operand(tall, b_layout):
    seen = 0
    for M, N, K, pad, D in itertools.product(MS, NS, KS, (0, 8), DS):
        d = desc(M, N, K, pad, b_layout)
        rc, (a0, a1, b0, b1) = span(d, tall, D)
        if b_layout == 1 and (not tall or N % 256):              # the k-major B exists in the 352x256 form only, whole column tiles
            assert rc != 0, (M, N, K, pad, D)
            continue
        assert rc == 0, (M, N, K, pad, D, rc)
        end_a = ((M - 1) * d.lda + K) * 2
        end_b = ((K - 1) * d.ldb + N) * 2 if b_layout else ((N - 1) * d.ldb + K) * 2
        assert 0 <= a0 <= a1 and a1 + 4 <= end_a, (M, N, K, pad, D, a0, a1, end_a)
        assert 0 <= b0 <= b1 and b1 + 4 <= end_b, (M, N, K, pad, D, b0, b1, end_b)
        # the last K-tile of the last row is touched (the walk is not vacuous), and nothing ahead of K-tile min(D, last) in the 352x256 form
        last = K // 64 - 1
        assert a1 == ((M - 1) * d.lda + last * 64) * 2, (M, N, K, pad, D, a1)
        if tall:
            assert a0 == min(D, last) * 128, (M, N, K, pad, D, a0)
        seen += 1
    assert seen == (len(MS) * len(KS) * 2 * len(DS)) * (len(NS) if not b_layout else 2 if tall else 0)


def test_distance_zero_touches_nothing_and_bad_arguments_are_refused():
    d = desc(5536, 4096, 4096, 0, 0)
    for tall in (0, 1):
        assert span(d, tall, 0) == (0, [-1, -1, -1, -1])
    assert span(d, 1, -1)[0] != 0
    assert _lib.lib().egomi_gemm_l2pf_span(None, 1, 4, (ctypes.c_int64 * 4)()) != 0
    assert _lib.lib().egomi_gemm_l2pf_span(ctypes.byref(d), 1, 4, None) != 0
    d.K = 100                                                     # no whole K-tiles
    assert span(d, 1, 4)[0] != 0


def test_a_distance_beyond_the_limit_is_the_limit():
    d = desc(704, 264, 4096, 8, 0)
    assert span(d, 1, 8) == span(d, 1, 100)


def test_the_setter_takes_every_documented_value():
    L = _lib.lib()
    try:
        for v in (0, 1, 4, 8, 100, -1):
            assert L.egomi_gemm_set_l2_prefetch(v) == 0
    finally:
        L.egomi_gemm_set_l2_prefetch(-1)
