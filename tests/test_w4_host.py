"""CPU: the int4 decode weights (csrc/w4.hip).  The C ABI is declared and exported; the torch restatement of the quantizer
(decode.w4_quantize / w4_unpack / w4_dequantize, what egomi_quantize_rows_int4 is bit-equal to) keeps its error within half a scale step,
gives zero groups scale 1 and codes 0, handles the ragged last group, packs K / 2 bytes per row in the stated nibble order, rounds ties to
even and never leaves [-7, 7]; groups whose amax is 7 * 2^e get s = 2^e exactly; four simulated kernel defects each miss the GPU test's
float bound by a wide margin; and the driver accepts --decode_weight_dtype int4."""
import ctypes
import os
import re

import pytest
import torch

from egoscaler_amd import build as B
from egoscaler_amd.decode import w4_dequantize, w4_quantize, w4_unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("egomi_quantize_rows_int4", "egomi_gemm_w4", "egomi_gemm_w4_slab_count")
RAGGED = [32, 96, 160, 352]
U = 2.0 ** -24


def _w(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)


def _full_scales(s, K):
    return s.t().repeat_interleave(128, 1)[:, :K]


def test_w4_entry_points_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egomi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(B.build())
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), n
        assert hasattr(lib, n), n


@pytest.mark.parametrize("K", RAGGED + [128, 4096])
def test_error_within_half_a_step_sizes_and_code_range(K):
    N = 12
    w = _w(N, K, K)
    packed, s = w4_quantize(w)
    NG = -(-K // 128)
    assert packed.dtype == torch.uint8 and packed.shape == (N, K // 2) and packed.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (NG, N) and s.is_contiguous()
    codes = w4_unpack(packed, K)
    assert codes.dtype == torch.int8 and codes.shape == (N, K) and int(codes.min()) >= -7 and int(codes.max()) <= 7
    nib = torch.stack([packed & 15, packed >> 4])
    assert int(nib.min()) >= 1                                            # nibble 0 (code -8) never occurs
    sf = _full_scales(s, K).double()
    # every group's amax lands on +-7, and s is amax / 7 rounded to fp32
    for g in range(NG):
        blk = slice(128 * g, min(K, 128 * g + 128))
        assert torch.equal(codes[:, blk].abs().amax(1), torch.full((N,), 7, dtype=torch.int8))
        assert torch.equal(s[g], w[:, blk].float().abs().amax(1) / 7.0)
    # |W - code * s| <= s / 2 in exact arithmetic; s and the quotient W / s are each rounded to fp32 (relative 2^-24), which can carry a
    # quotient of magnitude <= 7 across a tie by 7 * 2^-24 steps on each count: (1/2 + 2^-20) s covers both
    d = codes.double() * sf
    assert torch.equal(w4_dequantize(packed, s, K), d.float())            # the fp32 product, rounded once
    assert bool(((w.double() - d).abs() <= sf * (0.5 + 2.0 ** -20)).all())


def test_power_of_two_scales_are_exact_and_the_half_step_is_reached():
    """A group whose amax is 7 * 2^e gets s = 2^e exactly; then W / s is exact, bf16(code * s) is exact, the error bound is exactly s / 2
    and an entry 2.5 * 2^e reaches it (the tie goes to the even code 2)."""
    K = 352
    g = torch.Generator().manual_seed(4)
    e = torch.randint(-9, -2, (6, 3), generator=g)
    sc = torch.exp2(e.float()).repeat_interleave(128, 1)[:, :K]
    w = (torch.randn(6, K, generator=g).clamp_(-2.5, 2.5) * 2.5 * sc)
    w[:, 0::128] = 7 * sc[:, 0::128]
    w[:, 1::128] = 2.5 * sc[:, 1::128]
    w[:, 2::128] = -3.5 * sc[:, 2::128]
    w[:, 3::128] = 0.5 * sc[:, 3::128]
    w[:, 4::128] = -6.5 * sc[:, 4::128]
    w = w.to(torch.bfloat16)
    packed, s = w4_quantize(w)
    assert torch.equal(s, torch.exp2(e.float()).t().contiguous())
    codes = w4_unpack(packed, K)
    assert codes[:, 0::128].eq(7).all() and codes[:, 1::128].eq(2).all() and codes[:, 2::128].eq(-4).all()      # ties to even
    assert codes[:, 3::128].eq(0).all() and codes[:, 4::128].eq(-6).all()
    d = w4_dequantize(packed, s, K)
    assert torch.equal(d.to(torch.bfloat16).float(), d)                   # bf16(code * s) is exact
    err = (w.float() - d).abs()
    assert bool((err <= sc / 2).all()) and bool((err[:, 1::128] == sc[:, 1::128] / 2).all())


def test_zero_groups_scale_one_codes_zero():
    w = _w(5, 352, 1)
    w[1] = 0
    w[2, 128:256] = 0
    w[3, 256:] = 0                                                        # the ragged group
    packed, s = w4_quantize(w)
    codes = w4_unpack(packed, 352)
    assert bool((s[:, 1] == 1.0).all()) and bool((codes[1] == 0).all()) and bool((packed[1] == 0x88).all())
    assert float(s[1, 2]) == 1.0 and bool((codes[2, 128:256] == 0).all()) and float(s[0, 2]) != 1.0
    assert float(s[2, 3]) == 1.0 and bool((codes[3, 256:] == 0).all())


def test_ragged_groups_are_quantized_on_their_own_columns():
    for K in RAGGED:
        w = _w(8, K, 10 + K)
        packed, s = w4_quantize(w)
        last = 128 * ((K - 1) // 128)
        p2, s2 = w4_quantize(w[:, last:].contiguous())                    # the last group alone
        assert torch.equal(s[-1], s2[0]) and torch.equal(packed[:, last // 2:], p2)
        wide = torch.cat([w, torch.full((8, 32), 5.0, dtype=torch.bfloat16)], 1) if K % 128 else None
        if wide is not None:                                              # 32 more columns join the last group and change its scale only
            p3, s3 = w4_quantize(wide)
            assert torch.equal(s3[:-1], s[:-1]) and torch.equal(p3[:, :last // 2], packed[:, :last // 2]) and not torch.equal(s3[-1], s[-1])


def test_unpack_inverts_the_packing_and_the_stated_nibble_order():
    g = torch.Generator().manual_seed(7)
    N, K = 9, 160
    packed = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    codes = w4_unpack(packed, K)
    # csrc/w4.hip: byte b of a row holds column 2 b in its low nibble and column 2 b + 1 in its high nibble
    assert torch.equal((packed & 15).long() - 8, codes[:, 0::2].long()) and torch.equal((packed >> 4).long() - 8, codes[:, 1::2].long())
    # pack(unpack) is the identity wherever the nibbles are codes (1 .. 15): go through w4_quantize with scale 1 (amax 7)
    c = torch.randint(-7, 8, (N, K), generator=g)
    c[:, 0::128] = 7
    p, s = w4_quantize(c.to(torch.bfloat16))
    assert bool((s == 1.0).all()) and torch.equal(w4_unpack(p, K).long(), c)


def test_ties_round_to_even():
    w = torch.zeros(1, 32)
    w[0, :16] = torch.tensor([7.0, 0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, -0.5, -1.5, -2.5, -3.5, -4.5, -5.5, -6.5, -7.0])
    packed, s = w4_quantize(w.to(torch.bfloat16))
    assert float(s[0, 0]) == 1.0
    assert w4_unpack(packed, 32)[0, :16].tolist() == [7, 0, 2, 2, 4, 4, 6, 6, 0, -2, -2, -4, -4, -6, -6, -7]


# -- simulated defects against the GPU test's float bound --------------------------------------------------------------------------------
def _bound_case(K, seed=0):
    """tests/test_gpu_w4_kernels.py's random case on the host: float64 target and the bound (K + NG + 2) u E + 2^-8 |target|,
    E = sum_k |x| (|code| + 16) s."""
    N, M = 68, 5
    g = torch.Generator().manual_seed(seed)
    w = _w(N, K, seed + 1)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    packed, s = w4_quantize(w)
    codes, sf = w4_unpack(packed, K).double(), _full_scales(s, K).double()
    tgt = x @ (codes * sf).T
    bound = (K + s.shape[0] + 2) * U * (x.abs() @ ((codes.abs() + 16) * sf).T) + 2.0 ** -8 * tgt.abs() + 1e-30
    return x, packed, s, codes, sf, tgt, bound


@pytest.mark.parametrize("K", [32, 352])
def test_simulated_defects_miss_the_float_bound(K):
    x, packed, s, codes, sf, tgt, bound = _bound_case(K)
    N, NG = codes.shape[0], s.shape[0]
    worst = lambda y: float(((y - tgt).abs() / bound).max())
    assert worst(x @ (codes * sf).T) == 0.0 and worst((x @ (codes * sf).T).to(torch.bfloat16).double()) <= 1.0
    defects = {}
    swapped = (packed << 4) | (packed >> 4)                               # the two nibbles of every byte swapped
    defects["nibbles swapped"] = x @ (w4_unpack(swapped, K).double() * sf).T
    if NG > 1:                                                            # the ragged last group on the previous group's scale
        s_prev = s.clone()
        s_prev[-1] = s[-2]
        defects["last group's scale"] = x @ (codes * _full_scales(s_prev, K).double()).T
    s_t = s.t().contiguous().view(NG, N)                                  # the scales read [N, NG] instead of [NG, N]
    if NG > 1:
        defects["scales transposed"] = x @ (codes * _full_scales(s_t, K).double()).T
    defects["sign offset forgotten"] = x @ ((codes + 8) * sf).T
    assert len(defects) == (4 if NG > 1 else 2)                           # K = 32 has one group: the two scale defects need K = 352
    for name, y in defects.items():
        assert worst(y) > 20.0, (name, worst(y))
        assert float((y - tgt).norm() / tgt.norm()) > 1e-2, name


def test_driver_accepts_int4():
    from egoscaler_amd import driver
    assert driver.parse_args(["eval", "--tiny", "--decode_weight_dtype", "int4"]).decode_weight_dtype == "int4"
    assert driver.parse_args(["eval", "--tiny"]).decode_weight_dtype == "auto"
