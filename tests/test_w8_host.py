"""CPU: the fp8 decode weights' C ABI (csrc/w8.hip) is declared and exported, and the torch restatement of its quantizer (decode.w8_quantize,
what egomi_quantize_rows_fp8 is bit-equal to) keeps codes within +-448, gives zero rows scale 1 and zero codes, flushes entries far below the
row's amax to e4m3fn subnormals or zero, and agrees with the KV cache's restatement applied row by row."""
import ctypes
import os
import re

import torch

from egoscaler_amd import build as B
from egoscaler_amd.decode import kv8_quantize, w8_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("egomi_quantize_rows_fp8", "egomi_gemm_w8", "egomi_gemm_w8_slab_count")


def test_w8_entry_points_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egomi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(B.build())
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), n
        assert hasattr(lib, n), n


def _values(codes):
    return codes.view(torch.float8_e4m3fn).float()


def test_codes_bounded_and_amax_maps_to_448():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 352, generator=g) * 0.02).to(torch.bfloat16)
    codes, s = w8_quantize(w)
    v = _values(codes)
    assert codes.dtype == torch.uint8 and s.dtype == torch.float32 and codes.shape == w.shape and s.shape == (64,)
    assert bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 448.0
    assert torch.equal(v.abs().amax(1), torch.full((64,), 448.0))          # every row's amax lands on the largest code
    deq = v * s[:, None]
    assert float(((deq - w.float()).abs() / w.float().abs().amax(1, keepdim=True)).max()) <= 2.0 ** -4 * 448 / 256 + 1e-6


def test_zero_rows_scale_one_zero_codes():
    w = torch.zeros(3, 128, dtype=torch.bfloat16)
    w[1, 5] = 1.0
    codes, s = w8_quantize(w)
    assert float(s[0]) == 1.0 and float(s[2]) == 1.0 and float(s[1]) == float(torch.tensor(1.0) / 448.0)
    assert bool((codes[0] == 0).all()) and bool((codes[2] == 0).all())
    assert int(codes[1, 5]) == 0x7E and int((codes[1] != 0).sum()) == 1


def test_outlier_flushes_small_entries_like_e4m3fn():
    # amax 448 -> s = 1: entries are coded as they are; e4m3fn's smallest subnormal is 2^-9, anything below 2^-10 becomes (signed) zero
    w = torch.tensor([[448.0, 1.0, 2.0 ** -7, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -11, -2.0 ** -12]], dtype=torch.bfloat16)
    codes, s = w8_quantize(w)
    assert float(s[0]) == 1.0
    c = codes[0].tolist()
    assert c[0] == 0x7E and c[1] == 0x38                                  # 1.0: exponent 7, mantissa 0
    assert c[2] == 0x04                                                   # 2^-7 = 4 * 2^-9: subnormal
    assert c[3] == 0x01 and c[4] == 0x02                                  # 2^-9; 1.5 * 2^-9 ties to even (2 * 2^-9)
    assert c[5] == 0x00 and c[6] == 0x00 and c[7] == 0x80                  # 2^-10 ties to 0; below flushes to +-0
    # a row with one huge entry: the ordinary entries lose their precision to the outlier's scale
    g = torch.Generator().manual_seed(1)
    row = (torch.randn(1, 4096, generator=g) * 0.02).to(torch.bfloat16)
    row[0, 7] = 8192.0
    codes, s = w8_quantize(row)
    v = _values(codes)[0]
    small = torch.ones(4096, dtype=torch.bool)
    small[7] = False
    assert float(v[small].abs().max()) < 2.0 ** -6                         # all of them subnormal or zero
    assert int((v[small] == 0).sum()) > 0


def test_agrees_with_kv8_restatement_row_wise():
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(96, 4096, generator=g) * torch.logspace(-30, 3, 96)[:, None]).to(torch.bfloat16)
    w[3] = 0
    w[5, :100] = 2.0 ** -133                                              # a subnormal bf16 amax
    c1, s1 = w8_quantize(w)
    c2, s2 = kv8_quantize(w)
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
