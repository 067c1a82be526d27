"""CPU: the fp8 KV cache's C ABI is declared and exported, and its torch restatement (decode.kv8_quantize, what the kernels of csrc/kv8.hip
are bit-equal to) produces the known e4m3fn codes: 448 at the head's amax, ties to even, zero heads with scale 1."""
import ctypes
import os
import re

import torch

from egoscaler_amd import build as B
from egoscaler_amd.decode import kv8_dequantize, kv8_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("egomi_kv_append_fp8", "egomi_qkv_finish_fp8", "egomi_attn_decode_fp8", "egomi_attn_decode_rows_fp8")


def test_fp8_entry_points_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egomi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(B.build())
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), n
        assert hasattr(lib, n), n


def test_restatement_codes():
    # amax 1 -> s = 1/448: x / s = 448 x
    x = torch.tensor([[1.0, -1.0, 0.0, -0.0, 0.999, 0.5, 2.0 ** -7, 0.9]])
    codes, s = kv8_quantize(x)
    assert torch.equal(s, torch.tensor([1.0]) / 448.0)
    c = codes[0].tolist()
    assert c[0] == 0x7E and c[1] == 0xFE                                  # 448 = 1.75 * 2^8: exponent 15, mantissa 6
    assert c[2] == 0x00 and c[3] == 0x80                                  # signed zero kept
    assert c[4] == 0x7E                                                   # 447.55 rounds up to 448
    assert c[5] == 0x76                                                   # 224 = 1.75 * 2^7: exponent 14
    assert c[6] == 0x46                                                   # 3.5 = 1.75 * 2^1: exponent 8
    assert c[7] == 0x7D                                                   # 403.2 -> 416 = 1.625 * 2^8 (above the 400 midpoint)
    # ties to even: amax 448 -> s = 1; 17 lies between 16 (mantissa 0) and 18 (mantissa 1) -> 16; 19 between 18 and 20 -> 20
    codes, s = kv8_quantize(torch.tensor([[448.0, 17.0, 19.0, 0.0009765625, 0.0029296875]]))
    assert float(s[0]) == 1.0
    c = codes[0].tolist()
    assert c[0] == 0x7E and c[1] == 0x58 and c[2] == 0x5A
    assert c[3] == 0x00 and c[4] == 0x02                                  # subnormals: 2^-10 ties to 0, 3 * 2^-10 ties to 2 * 2^-9
    # zero heads: scale 1, codes 0
    codes, s = kv8_quantize(torch.zeros(2, 3, 64))
    assert bool((s == 1.0).all()) and bool((codes == 0).all())
    # round trip of every finite code through its own scale
    allc = torch.arange(256, dtype=torch.uint8)
    finite = allc[(allc & 0x7F) != 0x7F]
    v = finite.view(torch.float8_e4m3fn).float()
    v[0] = 448.0                                                          # pin the head's amax so that s = 1
    codes, s = kv8_quantize(v[None])
    assert float(s[0]) == 1.0
    assert torch.equal(codes[0][1:], finite[1:])
    assert torch.equal(kv8_dequantize(codes, s)[0], v)
