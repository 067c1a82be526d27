"""GPU: every form of the fused attention kernels (csrc/attention.hip: forward forms 1-4 with both block orders and a capped persistent grid,
backward forms 1-3 with and without the inverse-RoPE epilogue, head_dim 128 and 64) and the decode attention kernel (every form of
attn_decode.hip) against the float64 oracle of tests/attn_oracle.py, element by element: |got - ref| <= TAU * E + PHI * max(E), E the magnitude of
the terms that make up the element (the bounds and their measurements are in attn_oracle.py's docstring).  Each case's reference is computed
once and shared by every form.  The backward is handed the oracle's O (bf16) and LSE (fp32), so it is judged on exact inputs.

Rows that see no key (left padding under causal masking) must come out exactly 0 with LSE = +inf, and their dout must add nothing to dQ,
dK or dV.  Kernel forms are selected only through the egomi_attn_set_* setters; the `lib` fixture restores the defaults."""
import math

import pytest
import torch

from egoscaler_amd import _lib
from egoscaler_amd import decode as D
from egoscaler_amd import ops
from tests import attn_oracle as A

pytestmark = pytest.mark.gpu

WORST = {}                # kind -> (worst ratio, case): printed at the end of the module (-s) — the source of the bounds in attn_oracle.py


def _note(kind, r, case):
    if r > WORST.get(kind, (-1.0, ""))[0]:
        WORST[kind] = (r, case)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kind, (r, case) in sorted(WORST.items()):
        print(f"attn-oracle worst {kind:10s} {r:.3e}  ({case})")


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


def check(kind, got, ref, e, case):
    r = A.ratio(got, ref, e)
    _note(kind, r, case)
    _note(kind + "@phi/10", A.ratio(got, ref, e, A.PHI / 10), case)      # how much of the margin the floor provides
    assert r <= A.TAU, f"{kind} {case}: worst (err - PHI max E) / E = {r:.3e} > TAU {A.TAU}"


def check_lse(got, ref, smax, case):
    r = A.lse_ratio(got, ref, smax)
    _note("lse", r, case)
    assert r <= A.LSE_TOL, f"lse {case}: worst err / (1 + max|s|) = {r:.3e} > {A.LSE_TOL}"


# ------------------------------------------------------------------------------------------ inputs
def make_mask(kind, B, S):
    if kind is None:
        return None
    km = torch.ones(B, S, dtype=torch.uint8)
    if kind == "pad1":                                 # right padding of one key
        km[-1, S - 1] = 0
    elif kind == "padtile":                            # right padding of exactly the last 32-key tile (S % 32 == 0)
        km[-1, S - 32:] = 0
    elif kind == "tail":
        km[-1, S - max(1, S // 5):] = 0
    elif kind == "allbut1":                            # every key but the first
        km[-1, 1:] = 0
    elif kind == "holes":
        km[0, 2:4] = 0
        km[0, S // 3:S // 3 + 40] = 0
        km[-1, S // 2] = 0
    elif kind == "left":                               # left padding: under causal masking, rows that see no key
        km[-1, :max(1, S // 7)] = 0
        if B > 2:
            km[1, :S // 2] = 0
    return km


def make_qkv(B, S, H, hd, dist, seed):
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    x = torch.randn(B * S, 3 * d, generator=g).view(B, S, 3, H, hd)
    t = torch.arange(S, dtype=torch.float32)
    if dist in ("peaked", "signature"):                # scores spread over about +-30 (the stale-max bound F3_THR and the rescale)
        x[:, :, :2] *= 2.3
    elif dist == "growing":                            # a maximum that climbs by ~5 nats per 32 keys: every tile rescales
        x[:, :, 0, :, 0] = 8.0
        x[:, :, 1, :, 0] = (5.0 / 32.0) * t[None, :, None] * math.sqrt(hd) / 8.0
    elif dist == "first":                              # key 0 dominates every row by ~20 nats
        x[:, :, 0, :, 0] = 8.0
        x[:, :, 1, :, 0] = 0.0
        x[:, 0, 1, :, 0] = 20.0 * math.sqrt(hd) / 8.0
    if dist == "signature":                            # V carries a per-key signature: a misrouted tile shows in O
        j = torch.arange(hd, dtype=torch.float32)
        x[:, :, 2] = torch.cos(0.37 * (t[:, None] + 1) * (j[None, :] + 1) + 0.1 * t[:, None])[None, :, None, :] * (1 + t / S)[None, :, None, None]
    return x.reshape(B * S, 3 * d).bfloat16()


# (B, S, H, hd, causal, mask, dist)
SWEEP = [(1, s, 2, 128, True, None, "normal") for s in (1, 31, 32, 33, 127, 128, 129, 256, 257, 513, 692, 1023, 1024, 1025, 2048, 4096)]
CASES = SWEEP + [
    (2, 31, 2, 128, False, None, "normal"), (1, 129, 3, 128, False, "holes", "normal"), (1, 1025, 1, 128, False, "tail", "normal"),
    (2, 692, 2, 128, True, "pad1", "normal"), (2, 256, 2, 128, True, "padtile", "normal"), (2, 692, 2, 128, True, "allbut1", "normal"),
    (2, 692, 2, 128, True, "holes", "normal"), (3, 692, 2, 128, True, "left", "normal"), (2, 300, 2, 128, False, "left", "normal"),
    (2, 1025, 1, 128, True, "left", "normal"), (2, 128, 2, 128, False, "allbut1", "normal"),
    (1, 692, 2, 128, True, None, "peaked"), (2, 257, 2, 128, True, "tail", "growing"), (1, 1025, 1, 128, True, None, "growing"),
    (1, 692, 2, 128, True, None, "first"), (2, 513, 2, 128, False, "holes", "first"), (1, 692, 2, 128, True, None, "signature"),
    (2, 300, 2, 128, False, None, "signature"),
    (8, 692, 32, 128, True, "tail", "normal"),          # the bench's attention shape: the persistent blocks walk several items each
    # head_dim 64: forms 1 and 2 forward, the first-form backward
    (2, 513, 6, 64, False, None, "normal"),              # the PointBERT blocks under --unfreeze_pc_encoder
    (1, 1, 1, 64, True, None, "normal"), (1, 33, 2, 64, True, None, "normal"), (2, 128, 2, 64, False, "padtile", "normal"),
    (1, 257, 2, 64, True, None, "peaked"), (3, 692, 2, 64, True, "left", "normal"), (2, 300, 3, 64, False, "holes", "signature"),
    (1, 1025, 1, 64, True, "tail", "growing"),
]


def _id(c):
    B, S, H, hd, causal, mask, dist = c
    return f"B{B}-S{S}-H{H}-hd{hd}-{'causal' if causal else 'full'}-{mask or 'nomask'}-{dist}"


class Case:
    """Inputs and float64 references of one case, built once; `layout`: q|k|v, O, dout and dq|dk|dv as views into wider buffers."""

    def __init__(self, B, S, H, hd, causal, mask, dist, scale=None, layout=False):
        self.B, self.S, self.H, self.hd, self.causal, self.layout = B, S, H, hd, causal, layout
        self.name = _id((B, S, H, hd, causal, mask, dist)) + ("-wide" if layout else "")
        self.scale = hd ** -0.5 if scale is None else scale
        d = self.d = H * hd
        seed = B * 7919 + S * 31 + H * 7 + hd + len(dist) + (0 if mask is None else len(mask) * 101)
        self.qkv = make_qkv(B, S, H, hd, dist, seed)
        g = torch.Generator().manual_seed(seed + 1)
        self.dout = torch.randn(B * S, d, generator=g).bfloat16()
        self.km = make_mask(mask, B, S)
        q, k, v = A.split_qkv(self.qkv, B, S, H, hd)
        self.fw = A.forward(q, k, v, self.scale, causal, self.km)
        self.o_in = A.bhsd_to_rows(self.fw["o"]).bfloat16()                 # what the backward is handed
        self.lse_in = self.fw["lse"].float()
        self.bw = A.backward(q, k, v, A.rows_to_bhsd(self.o_in, B, S, H, hd), A.rows_to_bhsd(self.dout, B, S, H, hd),
                             self.scale, causal, self.km)
        self.dead_rows = self.fw["dead"]                                    # [B, S]

    @property
    def kmc(self):
        return None if self.km is None else self.km.cuda()

    # device operands: plain, or views into wider buffers whose extra columns hold a sentinel
    def wide(self, src, extra, fill):
        if not self.layout:
            return src.cuda(), None
        buf = torch.full((src.shape[0], src.shape[1] + extra), fill, dtype=src.dtype, device="cuda")
        buf[:, :src.shape[1]] = src.cuda()
        return buf[:, :src.shape[1]], buf

    def out_buf(self, cols, fill):
        extra = 24 if self.layout else 0
        buf = torch.full((self.B * self.S, cols + extra), fill, dtype=torch.bfloat16, device="cuda")
        return buf[:, :cols], buf


def _sentinel_ok(buf, cols, fill):
    return buf is None or bool((buf[:, cols:] == fill).all())


_CACHE = {}


def get_case(c, **kw):
    key = (c, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE.clear()                                  # one case alive at a time (the bench shape's references are large)
        _CACHE[key] = Case(*c, **kw)
    return _CACHE[key]


FWD_RUNS = {128: [(1, 0, 0), (2, 0, 0), (3, 0, 0), (3, 3, 0), (4, 0, 0), (4, 0, 3)], 64: [(1, 0, 0), (2, 0, 0)]}     # (form, group, capped grid)


def run_forward(lib, cs):
    qkv, qbuf = cs.wide(cs.qkv, 40, -5.0)
    B, S, H, hd = cs.B, cs.S, cs.H, cs.hd
    ref_o = A.bhsd_to_rows(cs.fw["o"])
    e_o = A.bhsd_to_rows(cs.fw["e_o"])
    for form, group, blocks in FWD_RUNS[hd]:
        assert lib.egomi_attn_set_fwd_form(form) == 0 and lib.egomi_attn_set_fwd_group(group) == 0 and lib.egomi_attn_set_fwd_blocks(blocks) == 0
        out, obuf = cs.out_buf(cs.d, 7.0)
        lse = torch.full((B, H, S), 7.0, dtype=torch.float32, device="cuda")
        ops.attn_fwd(qkv, B, S, H, hd, cs.scale, out, lse, causal=cs.causal, key_mask=cs.kmc)
        torch.cuda.synchronize()
        tag = f"{cs.name} fwd form {form} group {group} blocks {blocks}"
        o = out.cpu()
        assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any()), tag
        check("o", o, ref_o, e_o, tag)
        check_lse(lse.cpu(), cs.fw["lse"], cs.fw["smax"], tag)
        if bool(cs.dead_rows.any()):                   # rows that see no key: exactly 0 and +inf
            dead = cs.dead_rows.reshape(-1)
            assert bool((o[dead].float() == 0).all()), tag
            assert bool((lse.cpu().permute(0, 2, 1)[cs.dead_rows] == float("inf")).all()), tag
        assert _sentinel_ok(obuf, cs.d, 7.0) and _sentinel_ok(qbuf, 3 * cs.d, -5.0), tag


def run_backward(lib, cs, rope):
    B, S, H, hd, d = cs.B, cs.S, cs.H, cs.hd, cs.d
    qkv, _ = cs.wide(cs.qkv, 40, -5.0)
    o_in, _ = cs.wide(cs.o_in, 24, -6.0)
    dout, _ = cs.wide(cs.dout, 24, -6.0)
    lse = cs.lse_in.cuda()
    rp, refs = None, {n: cs.bw[n] for n in ("dq", "dk", "dv")}
    es = {n: cs.bw["e_" + n] for n in ("dq", "dk", "dv")}
    if rope:
        cos, sin = ops.rope_tables(max(S, 8), hd, 10000.0)
        rp = (cos.cuda(), sin.cuda())
        for n in ("dq", "dk"):
            refs[n], es[n] = A.rope_inverse(refs[n], es[n], cos, sin)
    refs = {n: A.bhsd_to_rows(t) for n, t in refs.items()}
    es = {n: A.bhsd_to_rows(t) for n, t in es.items()}
    dead = cs.dead_rows.reshape(-1)
    for form in ((1, 2, 3) if hd == 128 else (3,)):     # head_dim 64 runs the first-form kernels whatever the setting
        assert lib.egomi_attn_set_bwd_form(form) == 0
        tag = f"{cs.name} bwd form {form}{' rope' if rope else ''}"
        dqkv, dbuf = cs.out_buf(3 * d, 3.0)
        delta = torch.full((B, H, S), 3.0, dtype=torch.float32, device="cuda")
        ops.attn_bwd(qkv, o_in, lse, dout, dqkv, delta, B, S, H, hd, cs.scale, causal=cs.causal, key_mask=cs.kmc, rope=rp)
        torch.cuda.synchronize()
        got = dqkv.cpu()
        assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(delta).all()), tag
        for i, n in enumerate(("dq", "dk", "dv")):
            check(n, got[:, i * d:(i + 1) * d], refs[n], es[n], tag)
        check("delta", delta.cpu(), cs.bw["delta"], cs.bw["e_delta"], tag)
        assert _sentinel_ok(dbuf, 3 * d, 3.0), tag
        if bool(dead.any()):                            # the dout of rows that see no key adds nothing anywhere
            assert bool((got[dead, :d].float() == 0).all()), tag
            dz = cs.dout.clone()
            dz[dead] = 0
            dz, _ = cs.wide(dz, 24, -6.0)
            dqkv2, _ = cs.out_buf(3 * d, 3.0)
            ops.attn_bwd(qkv, o_in, lse, dz, dqkv2, delta, B, S, H, hd, cs.scale, causal=cs.causal, key_mask=cs.kmc, rope=rp)
            torch.cuda.synchronize()
            assert torch.equal(dqkv2.cpu(), got), tag


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_attention_forms_against_float64(lib, c):
    cs = get_case(c)
    run_forward(lib, cs)
    run_backward(lib, cs, rope=False)
    if cs.hd == 128:
        run_backward(lib, cs, rope=True)


@pytest.mark.parametrize("c,scale", [((2, 300, 2, 128, True, "left", "normal"), 0.07), ((1, 692, 2, 128, False, "holes", "peaked"), 0.05),
                                     ((2, 200, 3, 64, True, "tail", "normal"), 0.2)], ids=lambda x: str(x) if not isinstance(x, tuple) else _id(x))
def test_attention_strided_operands_and_other_scales(lib, c, scale):
    """q|k|v, O, dout and dq|dk|dv as views into wider buffers (ld_qkv > 3 H hd, ld_o > H hd, ld_dqkv > 3 H hd) whose extra columns must
    keep their sentinel; softmax scales other than head_dim ** -0.5."""
    cs = get_case(c, scale=scale, layout=True)
    run_forward(lib, cs)
    run_backward(lib, cs, rope=False)
    if cs.hd == 128:
        run_backward(lib, cs, rope=True)


# ------------------------------------------------------------------------------------------ decode attention
def _decode_inputs(B, H, hd, Smax, T, seed, n_phys=None):
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    qrows = (torch.randn(B, 3 * d, generator=g) * 1.5).bfloat16()
    P_ = B if n_phys is None else n_phys
    kc = (torch.randn(P_, H, Smax, hd, generator=g) * 1.5).bfloat16()
    vc = torch.randn(P_, H, Smax, hd, generator=g).bfloat16()
    kc[:, :, T:] = float("nan")                          # never read: keys at or beyond T_len
    vc[:, :, T:] = float("nan")
    km = torch.ones(B, Smax, dtype=torch.uint8)
    for b in range(B):                                   # per-sample left padding (every third sample: none); sample 1 sees no key when T is small
        km[b, :min(T, (b * 37) % (T + 1))] = 0 if b % 3 else 1
    return qrows, kc, vc, km


def _decode_check(got, o, e, B, H, hd, km, T, tag):
    got = got[:, :H * hd].reshape(B, H, hd)
    assert bool(torch.isfinite(got.float()).all()), tag
    check("decode", got, o, e, tag)
    dead = ~km[:, :T].bool().any(-1)
    if bool(dead.any()):
        assert bool((got[dead].float() == 0).all()), tag


DECODE = [(3, 2, hd, 800, T) for hd in (64, 128) for T in (1, 63, 64, 65, 257, 700, 800)] + [(256, 4, 128, 320, 300), (256, 2, 64, 320, 129)]


@pytest.mark.parametrize("B,H,hd,Smax,T", DECODE)
def test_attn_decode_against_float64(B, H, hd, Smax, T):
    d = H * hd
    qrows, kc, vc, km = _decode_inputs(B, H, hd, Smax, T, B + H + hd + T)
    scale = hd ** -0.5
    q = qrows[:, :d].double().reshape(B, H, hd)
    o, e = A.decode(q, kc.double(), vc.double(), scale, T, km)
    out = torch.full((B, d + 8), 9.0, dtype=torch.bfloat16, device="cuda")
    D.attn_decode(qrows.cuda(), 3 * d, kc.cuda(), vc.cuda(), km.cuda(), out, B, H, hd, Smax, T, scale)
    torch.cuda.synchronize()
    _decode_check(out.cpu(), o, e, B, H, hd, km, T, f"attn_decode B{B} H{H} hd{hd} T{T}")
    assert bool((out[:, d:] == 9.0).all())

    # fp8 cache: the float64 attention of the dequantised cache
    k8, ks = D.kv8_quantize(kc[:, :, :T])
    v8, vs = D.kv8_quantize(vc[:, :, :T])
    k8f = torch.full((B, H, Smax, hd), 0x7F, dtype=torch.uint8)    # 0x7F: NaN in e4m3fn, never read
    v8f = k8f.clone()
    ksf, vsf = torch.full((B, H, Smax), float("nan")), torch.full((B, H, Smax), float("nan"))
    k8f[:, :, :T], v8f[:, :, :T], ksf[:, :, :T], vsf[:, :, :T] = k8, v8, ks, vs
    kd = torch.zeros(B, H, Smax, hd, dtype=torch.float64)
    vd = torch.zeros_like(kd)
    kd[:, :, :T], vd[:, :, :T] = D.kv8_dequantize(k8, ks).double(), D.kv8_dequantize(v8, vs).double()
    o8, e8 = A.decode(q, kd, vd, scale, T, km)
    out8 = torch.full((B, d), 9.0, dtype=torch.bfloat16, device="cuda")
    D.attn_decode_fp8(qrows.cuda(), 3 * d, k8f.cuda(), v8f.cuda(), ksf.cuda(), vsf.cuda(), km.cuda(), out8, B, H, hd, Smax, T, scale)
    torch.cuda.synchronize()
    _decode_check(out8.cpu(), o8, e8, B, H, hd, km, T, f"attn_decode_fp8 B{B} H{H} hd{hd} T{T}")


@pytest.mark.parametrize("nb,items,H,hd,Smax,T", [(4, 2, 2, 128, 300, 257), (3, 2, 3, 64, 128, 65), (4, 1, 2, 128, 64, 1), (2, 3, 2, 64, 800, 700)])
def test_attn_decode_rows_against_float64(nb, items, H, hd, Smax, T):
    """The row-table variants: key t of logical row r from physical row kv_row[r, t], a table that mixes parents at every key."""
    B = nb * items
    d = H * hd
    qrows, kc, vc, km = _decode_inputs(B, H, hd, Smax, T, nb * 100 + T, n_phys=B)
    g = torch.Generator().manual_seed(T)
    base = (torch.arange(B) // nb * nb)[:, None]
    kv_row = (base + torch.randint(0, nb, (B, Smax + 5), generator=g)).to(torch.int32)
    scale = 0.9 * hd ** -0.5
    q = qrows[:, :d].double().reshape(B, H, hd)
    o, e = A.decode(q, kc.double(), vc.double(), scale, T, km, kv_row)
    out = torch.full((B, d), 9.0, dtype=torch.bfloat16, device="cuda")
    D.attn_decode_rows(qrows.cuda(), 3 * d, kc.cuda(), vc.cuda(), kv_row.cuda(), B, km.cuda(), out, B, nb, H, hd, Smax, T, scale)
    torch.cuda.synchronize()
    _decode_check(out.cpu(), o, e, B, H, hd, km, T, f"attn_decode_rows nb{nb} items{items} hd{hd} T{T}")

    k8, ks = D.kv8_quantize(kc[:, :, :T])
    v8, vs = D.kv8_quantize(vc[:, :, :T])
    k8f = torch.full((B, H, Smax, hd), 0x7F, dtype=torch.uint8)
    v8f = k8f.clone()
    ksf, vsf = torch.full((B, H, Smax), float("nan")), torch.full((B, H, Smax), float("nan"))
    k8f[:, :, :T], v8f[:, :, :T], ksf[:, :, :T], vsf[:, :, :T] = k8, v8, ks, vs
    kd = torch.zeros(B, H, Smax, hd, dtype=torch.float64)
    vd = torch.zeros_like(kd)
    kd[:, :, :T], vd[:, :, :T] = D.kv8_dequantize(k8, ks).double(), D.kv8_dequantize(v8, vs).double()
    o8, e8 = A.decode(q, kd, vd, scale, T, km, kv_row)
    out8 = torch.full((B, d), 9.0, dtype=torch.bfloat16, device="cuda")
    D.attn_decode_rows_fp8(qrows.cuda(), 3 * d, k8f.cuda(), v8f.cuda(), ksf.cuda(), vsf.cuda(), kv_row.cuda(), B, km.cuda(), out8, B, nb, H, hd,
                           Smax, T, scale)
    torch.cuda.synchronize()
    _decode_check(out8.cpu(), o8, e8, B, H, hd, km, T, f"attn_decode_rows_fp8 nb{nb} items{items} hd{hd} T{T}")
