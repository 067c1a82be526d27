"""GPU: the query window of the fused attention kernels (include/egomi.h, egomi_attn_desc.q_rows) against the same kernels without it.

Contract for q_rows = R, 0 < R < S, with dout zero at rows < S - R: o and lse at rows >= S - R, and dq|dk|dv at EVERY row, are
torch.equal to the q_rows = 0 call on the same inputs; dq is zero below the window; nothing outside the operands is written.  The kernels
only skip whole blocks they already compute, so nothing here needs a tolerance.  delta is filled with a non-zero sentinel before every
call: a dK/dV sweep that reads a word this call did not write gives dS = -P * 3 and fails the equality."""
import pytest
import torch

from egoscaler_amd import _lib
from egoscaler_amd import ops
from tests.test_gpu_attention_oracle import make_mask, make_qkv

pytestmark = pytest.mark.gpu
HD = 128

# (B, S, H, mask, R): a window inside one block, straddling a block edge (S = 692: blocks hang from S32 = 704, so R = 128 lies in two),
# skipped ranks, the ragged first block, left padding, right padding of the last keys; (4, 692, 2): H * B % 8 == 0, so group 3 really groups
CASES = [(2, 692, 2, "tail", R) for R in (1, 31, 128, 153, 257, 691)] + \
        [(1, 129, 2, None, 2), (1, 129, 2, None, 128), (3, 692, 2, "left", 153), (2, 257, 2, "last32", 130), (1, 33, 1, None, 5),
         (4, 692, 2, "tail", 153)]
FWD_RUNS = [(3, 0, 0), (3, 3, 0), (4, 0, 0), (4, 0, 3)]           # (form, group, capped grid: several items per persistent block)


@pytest.fixture
def lib():
    L = _lib.lib()
    try:
        yield L
    finally:                                          # the defaults, whatever a failing test selected
        L.egomi_attn_set_fwd_form(4)
        L.egomi_attn_set_fwd_group(0)
        L.egomi_attn_set_fwd_blocks(0)
        L.egomi_attn_set_bwd_form(3)


def _mask(kind, B, S):
    if kind == "last32":                               # padtile-style: the last sample's last 32 keys are padding
        km = torch.ones(B, S, dtype=torch.uint8)
        km[-1, S - 32:] = 0
        return km
    return make_mask(kind, B, S)


def _wide(src, extra, fill):
    buf = torch.full((src.shape[0], src.shape[1] + extra), fill, dtype=src.dtype, device="cuda")
    buf[:, :src.shape[1]] = src.cuda()
    return buf[:, :src.shape[1]], buf


def _inputs(B, S, H, mask, R):
    d = H * HD
    qkv, _ = _wide(make_qkv(B, S, H, HD, "normal", 1000 * B + S + 7 * H + R), 40, -5.0)
    km = _mask(mask, B, S)
    g = torch.Generator().manual_seed(S + R)
    dout = torch.randn(B, S, d, generator=g).bfloat16()
    if R < S:
        dout[:, :S - R] = 0
    dout, _ = _wide(dout.view(B * S, d), 24, -6.0)
    return qkv, None if km is None else km.cuda(), dout


def _fwd(qkv, km, B, S, H, q_rows):
    d = H * HD
    obuf = torch.full((B * S, d + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, H, S), 7.0, dtype=torch.float32, device="cuda")
    ops.attn_fwd(qkv, B, S, H, HD, HD ** -0.5, obuf[:, :d], lse, causal=True, key_mask=km, q_rows=q_rows)
    torch.cuda.synchronize()
    return obuf, lse


def _bwd(qkv, km, o, lse, dout, B, S, H, rope, q_rows):
    d = H * HD
    dbuf = torch.full((B * S, 3 * d + 24), 3.0, dtype=torch.bfloat16, device="cuda")
    delta = torch.full((B, H, S), 3.0, dtype=torch.float32, device="cuda")        # stale words: see the module docstring
    ops.attn_bwd(qkv, o, lse, dout, dbuf[:, :3 * d], delta, B, S, H, HD, HD ** -0.5, causal=True, key_mask=km, rope=rope, q_rows=q_rows)
    torch.cuda.synchronize()
    return dbuf


@pytest.mark.parametrize("B,S,H,mask,R", CASES, ids=lambda v: str(v))
def test_window_equals_the_full_call(lib, B, S, H, mask, R):
    d = H * HD
    qkv, km, dout = _inputs(B, S, H, mask, R)
    win = slice(S - R, S)
    o_full = o_win = None
    for form, group, blocks in FWD_RUNS:
        assert lib.egomi_attn_set_fwd_form(form) == 0 and lib.egomi_attn_set_fwd_group(group) == 0 and lib.egomi_attn_set_fwd_blocks(blocks) == 0
        tag = f"fwd form {form} group {group} blocks {blocks}"
        o0, l0 = _fwd(qkv, km, B, S, H, 0)
        o1, l1 = _fwd(qkv, km, B, S, H, R)
        assert torch.equal(o0.view(B, S, -1)[:, win, :d], o1.view(B, S, -1)[:, win, :d]), tag                          # (a)
        assert torch.equal(l0[:, :, win], l1[:, :, win]), tag
        assert bool((o1[:, d:] == 7.0).all()) and bool((o0[:, d:] == 7.0).all()), tag                                  # (d)
        assert bool(torch.isfinite(o1.float()).all()) and not bool(torch.isnan(l1).any()), tag        # lse of a row that sees no key is +inf
        if form == 4 and blocks == 0:
            o_full, l_full, o_win, l_win = o0, l0, o1, l1
    cos, sin = ops.rope_tables(max(S, 8), HD, 10000.0)
    for form in (1, 2, 3):
        assert lib.egomi_attn_set_bwd_form(form) == 0
        for rope in (None, (cos.cuda(), sin.cuda())):
            tag = f"bwd form {form}{' rope' if rope else ''}"
            g0 = _bwd(qkv, km, o_full[:, :d], l_full, dout, B, S, H, rope, 0)
            g1 = _bwd(qkv, km, o_full[:, :d], l_full, dout, B, S, H, rope, R)
            assert torch.equal(g0, g1), tag                                                                             # (b), (d): sentinel columns included
            assert bool((g1[:, 3 * d:] == 3.0).all()) and bool(torch.isfinite(g1.float()).all()), tag
            assert bool((g1.view(B, S, -1)[:, :S - R, :d] == 0).all()), tag                                             # (c)
            if form == 3:
                # as the engine calls it: o and lse from the windowed forward, their rows below the first computed block still the fill
                g2 = _bwd(qkv, km, o_win[:, :d], l_win, dout, B, S, H, rope, R)
                assert torch.equal(g0, g2), tag + " (windowed forward's o, lse)"


@pytest.mark.parametrize("extra", [0, 5])
def test_window_of_the_whole_sequence_is_no_window(lib, extra):
    B, S, H = 2, 257, 2
    d = H * HD
    qkv, km, dout = _inputs(B, S, H, "tail", S)
    for form, group, blocks in FWD_RUNS:
        assert lib.egomi_attn_set_fwd_form(form) == 0 and lib.egomi_attn_set_fwd_group(group) == 0 and lib.egomi_attn_set_fwd_blocks(blocks) == 0
        o0, l0 = _fwd(qkv, km, B, S, H, 0)
        o1, l1 = _fwd(qkv, km, B, S, H, S + extra)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), (form, group, blocks)
    for form in (1, 2, 3):
        assert lib.egomi_attn_set_bwd_form(form) == 0
        g0 = _bwd(qkv, km, o0[:, :d], l0, dout, B, S, H, None, 0)
        g1 = _bwd(qkv, km, o0[:, :d], l0, dout, B, S, H, None, S + extra)
        assert torch.equal(g0, g1), form
