"""GPU: the fp8 (e4m3fn) KV-cache kernels of csrc/kv8.hip and the fp8 forms of csrc/attn_decode.hip.  kv_append_fp8 / qkv_finish_fp8 are bit-equal to the torch restatement
(decode.kv8_quantize) of what kv_append / qkv_finish store; attn_decode_fp8 matches fp32 attention over the dequantised cache and ignores
poisoned (NaN-coded) keys beyond T_len or under the mask; attn_decode_rows_fp8 follows its row table; every operand may end an allocation."""
import ctypes

import pytest
import torch

from egoscaler_amd import decode as D, ops
from egoscaler_amd._lib import c_f, c_i, c_i64, lib
from egoscaler_amd.ops import P, S

pytestmark = pytest.mark.gpu

SEG = 2 << 20
E_BADARG, E_SHAPE, E_UNSUPPORTED = -1, -2, -4


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


def _rows(n, d, hd, seed, dtype):
    """[n, 3d] rows (q|k|v), rows of growing magnitude, with special heads: k and v head 1 all zero, and in row 1 a k head 0 whose values
    round up to 448 (x / s = 447.9...)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3 * d, generator=g) * torch.logspace(-2, 1, n)[:, None]
    x[:, d + hd:d + 2 * hd] = 0.0
    x[:, 2 * d + hd:2 * d + 2 * hd] = 0.0
    x[1, d:d + hd] = 0.0
    x[1, d:d + 8] = torch.tensor([1.0, 0.99981, -0.99979, 0.5, 0.0, -1.0, 0.93, 0.96875])
    return x.to(dtype)


def _restate_cache(kc, lo, hi):
    return D.kv8_quantize(kc[:, :, lo:hi].cpu())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("pos0", [0, 7, 33])
def test_kv_append_fp8_bit_equal_to_restatement(dtype, hd, pos0):
    B, Sq, H, Smax = 3, 5, 2, 40
    d = H * hd
    rows = _rows(B * Sq, d, hd, hd + pos0, dtype).cuda()
    kc = torch.zeros(B, H, Smax, hd, dtype=dtype, device="cuda")
    vc = torch.zeros_like(kc)
    D.kv_append(rows[:, d:2 * d], rows[:, 2 * d:], 3 * d, kc, vc, B, Sq, H, hd, Smax, pos0)
    k8 = torch.full((B, H, Smax, hd), 0x5A, dtype=torch.uint8, device="cuda")
    v8 = torch.full_like(k8, 0x5A)
    ks = torch.full((B, H, Smax), -3.0, device="cuda")
    vs = torch.full_like(ks, -3.0)
    D.kv_append_fp8(rows[:, d:2 * d], rows[:, 2 * d:], 3 * d, k8, v8, ks, vs, B, Sq, H, hd, Smax, pos0)
    torch.cuda.synchronize()
    for c8, sc, ref in ((k8, ks, kc), (v8, vs, vc)):
        codes, scales = _restate_cache(ref, pos0, pos0 + Sq)
        assert torch.equal(c8[:, :, pos0:pos0 + Sq].cpu(), codes)
        assert torch.equal(sc[:, :, pos0:pos0 + Sq].cpu(), scales)
        outside = torch.ones(Smax, dtype=torch.bool)
        outside[pos0:pos0 + Sq] = False
        assert bool((c8[:, :, outside] == 0x5A).all()) and bool((sc[:, :, outside] == -3.0).all())   # nothing written elsewhere
    assert bool((ks[:, 1, pos0:pos0 + Sq] == 1.0).all()) and bool((vs[:, 1, pos0:pos0 + Sq] == 1.0).all())   # all-zero heads: s = 1, codes 0
    assert bool((k8[:, 1, pos0:pos0 + Sq] == 0).all()) and bool((v8[:, 1, pos0:pos0 + Sq] == 0).all())
    assert k8[0, 0, pos0 + 1, :8].tolist()[:2] == [0x7E, 0x7E] and k8[0, 0, pos0 + 1, 2] == 0xFE       # 448 = 0x7E, also reached by rounding up


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("pos", [0, 9, 38])
def test_qkv_finish_fp8_bit_equal_to_qkv_finish(dtype, hd, pos):
    B, H, Smax, slices = 4, 3, 40, 3
    d = H * hd
    g = torch.Generator().manual_seed(hd * 7 + pos)
    slabs = (torch.randn(slices, B, 3 * d, generator=g) * 0.7).cuda()
    slabs[:, :, d:d + hd] = 0.0                                          # an all-zero k head
    slabs[:, 0, 2 * d:2 * d + 4] = torch.tensor([1.0, 0.99981, -1.0, 0.0])[None, :].cuda() / slices
    cos, sin = ops.rope_tables(Smax, hd, 10000.0)
    cos, sin = cos.cuda(), sin.cuda()
    qkv1 = torch.full((B, 3 * d), 5.0, dtype=dtype, device="cuda")
    qkv2 = qkv1.clone()
    kc = torch.zeros(B, H, Smax, hd, dtype=dtype, device="cuda")
    vc = torch.zeros_like(kc)
    ops.qkv_finish(slabs, slices, qkv1, cos, sin, pos, kc, vc, B, H, hd, Smax)
    k8 = torch.zeros(B, H, Smax, hd, dtype=torch.uint8, device="cuda")
    v8 = torch.zeros_like(k8)
    ks = torch.zeros(B, H, Smax, device="cuda")
    vs = torch.zeros_like(ks)
    ops.qkv_finish_fp8(slabs, slices, qkv2, cos, sin, pos, k8, v8, ks, vs, B, H, hd, Smax)
    torch.cuda.synchronize()
    assert torch.equal(qkv1, qkv2)                     # q bit-equal; k|v columns untouched by both
    for c8, sc, ref in ((k8, ks, kc), (v8, vs, vc)):
        codes, scales = _restate_cache(ref, pos, pos + 1)
        assert torch.equal(c8[:, :, pos:pos + 1].cpu(), codes)
        assert torch.equal(sc[:, :, pos:pos + 1].cpu(), scales)
        assert int(c8.ne(0).sum()) == int(c8[:, :, pos].ne(0).sum()) and int(sc.ne(0).sum()) == int(sc[:, :, pos].ne(0).sum())
    assert bool((ks[:, 0, pos] == 1.0).all()) and bool((k8[:, 0, pos] & 0x7F == 0).all())           # zero head (RoPE may leave -0: 0x80)


def _cache(B, H, Smax, hd, T, dtype, seed):
    """fp8 cache filled over [0, T) through kv_append_fp8 from random K / V; q [B, 3d] rows."""
    d = H * hd
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(B * T, 3 * d, generator=g) * 1.5).to(dtype).cuda()
    q = (torch.randn(B, 3 * d, generator=g) * 1.5).to(dtype).cuda()
    k8 = torch.zeros(B, H, Smax, hd, dtype=torch.uint8, device="cuda")
    v8 = torch.zeros_like(k8)
    ks = torch.zeros(B, H, Smax, device="cuda")
    vs = torch.zeros_like(ks)
    D.kv_append_fp8(rows[:, d:2 * d], rows[:, 2 * d:], 3 * d, k8, v8, ks, vs, B, T, H, hd, Smax, 0)
    return q, k8, v8, ks, vs


def _ref_attn(q, k8, v8, ks, vs, km, B, H, hd, T):
    kk = D.kv8_dequantize(k8[:, :, :T].cpu(), ks[:, :, :T].cpu())
    vv = D.kv8_dequantize(v8[:, :, :T].cpu(), vs[:, :, :T].cpu())
    qq = q[:, :H * hd].float().cpu().view(B, H, 1, hd)
    sc = (qq @ kk.transpose(-1, -2)) * hd ** -0.5
    if km is not None:
        sc = sc.masked_fill(~km[:, None, None, :T].cpu().bool(), float("-inf"))
    return (torch.softmax(sc, -1) @ vv).reshape(B, H * hd)


def _mask(B, Smax):
    km = torch.ones(B, Smax, dtype=torch.uint8)
    km[:, 1::3] = 0
    km[1, 20:300] = 0
    return km.cuda()


@pytest.mark.parametrize("dtype,hd", [(torch.float32, 32), (torch.bfloat16, 128), (torch.bfloat16, 64), (torch.float32, 128)])
@pytest.mark.parametrize("T", [1, 63, 64, 700])
@pytest.mark.parametrize("masked", [False, True])
def test_attn_decode_fp8_matches_dequantised_attention_and_ignores_poison(dtype, hd, T, masked):
    B, H, Smax = 3, 2, 720
    d = H * hd
    q, k8, v8, ks, vs = _cache(B, H, Smax, hd, T, dtype, seed=T + hd)
    km = _mask(B, Smax) if masked else None
    out = torch.zeros(B, d, dtype=dtype, device="cuda")
    D.attn_decode_fp8(q, 3 * d, k8, v8, ks, vs, km, out, B, H, hd, Smax, T, hd ** -0.5)
    torch.cuda.synchronize()
    ref = _ref_attn(q, k8, v8, ks, vs, km, B, H, hd, T)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert float((out.float().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    # poison: every position >= T and every masked position: NaN codes and NaN scales
    bad = torch.zeros(B, Smax, dtype=torch.bool, device="cuda")
    bad[:, T:] = True
    if km is not None:
        bad |= km == 0
    bad4 = bad[:, None, :].expand(B, H, Smax)
    k8[bad4] = 0x7F
    v8[bad4] = 0xFF
    ks[bad4] = float("nan")
    vs[bad4] = float("nan")
    out2 = torch.full_like(out, 9.0)
    D.attn_decode_fp8(q, 3 * d, k8, v8, ks, vs, km, out2, B, H, hd, Smax, T, hd ** -0.5)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out2.float()).all())
    assert torch.equal(out2, out)


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 128), (torch.float32, 64), (torch.bfloat16, 32)])
@pytest.mark.parametrize("T", [1, 70, 300])
def test_attn_decode_rows_fp8_follows_the_row_table(dtype, hd, T):
    nb, Bi, H, Smax = 4, 2, 2, 320
    B = Bi * nb
    d = H * hd
    q, k8, v8, ks, vs = _cache(B, H, Smax, hd, Smax, dtype, seed=3 * T + hd)
    km = _mask(B, Smax)
    scale = hd ** -0.5
    # identity table: bit-equal to attn_decode_fp8
    ident = torch.arange(B, dtype=torch.int32, device="cuda")[:, None].expand(B, Smax).contiguous()
    o1, o2 = torch.zeros(B, d, dtype=dtype, device="cuda"), torch.ones(B, d, dtype=dtype, device="cuda")
    D.attn_decode_fp8(q, 3 * d, k8, v8, ks, vs, km, o1, B, H, hd, Smax, T, scale)
    D.attn_decode_rows_fp8(q, 3 * d, k8, v8, ks, vs, ident, B, km, o2, B, nb, H, hd, Smax, T, scale)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)
    # shuffled table, some entries out of range (masked keys): equal to attn_decode_fp8 over the gathered cache with those keys masked
    g = torch.Generator().manual_seed(T)
    tab = torch.randint(0, B, (B, Smax), generator=g, dtype=torch.int32)
    oor = torch.rand(B, Smax, generator=g) < 0.1
    oor[:, 0] = False
    tab[oor] = torch.where(torch.rand(int(oor.sum()), generator=g) < 0.5, -1, B).to(torch.int32)
    tab = tab.cuda()
    src = tab.clamp(0, B - 1).long()
    t_idx = torch.arange(Smax, device="cuda")
    gk8 = k8[src, :, t_idx[None, :]].permute(0, 2, 1, 3).contiguous()     # [B, Smax, H, hd] -> [B, H, Smax, hd]
    gv8 = v8[src, :, t_idx[None, :]].permute(0, 2, 1, 3).contiguous()
    gks = ks[src, :, t_idx[None, :]].permute(0, 2, 1).contiguous()
    gvs = vs[src, :, t_idx[None, :]].permute(0, 2, 1).contiguous()
    km2 = km.clone()
    km2[oor.cuda()] = 0
    o3, o4 = torch.zeros(B, d, dtype=dtype, device="cuda"), torch.ones(B, d, dtype=dtype, device="cuda")
    D.attn_decode_fp8(q, 3 * d, gk8, gv8, gks, gvs, km2, o3, B, H, hd, Smax, T, scale)
    D.attn_decode_rows_fp8(q, 3 * d, k8, v8, ks, vs, tab, B, km, o4, B, nb, H, hd, Smax, T, scale)
    torch.cuda.synchronize()
    assert torch.equal(o3, o4)
    assert bool(torch.isfinite(o4.float()).all())


@pytest.mark.parametrize("hd,T", [(128, 64), (128, 100), (64, 128), (32, 200)])
def test_kv8_operands_at_the_end_of_their_allocations(hd, T):
    """Every operand of the four kernels ends an allocation of its own; results bit-equal to ordinary allocations."""
    B, H, nb, slices = 4, 2, 2, 2
    Smax = T
    d = H * hd
    g = torch.Generator().manual_seed(hd + T)
    rows0 = torch.randn(B * (T - 1), 3 * d, generator=g).to(torch.bfloat16).cuda()
    slabs0 = torch.randn(slices, B, 3 * d, generator=g).cuda()
    qkv0 = torch.zeros(B, 3 * d, dtype=torch.bfloat16, device="cuda")
    cos0, sin0 = ops.rope_tables(Smax, hd, 10000.0)
    km0 = _mask(B, Smax)
    tab0 = (torch.arange(B, dtype=torch.int32)[:, None] // nb * nb + torch.randint(0, nb, (B, Smax), generator=g, dtype=torch.int32)).cuda()
    res = []
    for placed in (False, True):
        keep = []
        put = (lambda t: at_end(t, keep)) if placed else (lambda t: t.clone())
        rows, slabs, qkv, km, tab = put(rows0), put(slabs0), put(qkv0), put(km0), put(tab0)
        cos, sin = put(cos0.cuda()), put(sin0.cuda())
        k8 = put(torch.zeros(B, H, Smax, hd, dtype=torch.uint8, device="cuda"))
        v8 = put(torch.zeros(B, H, Smax, hd, dtype=torch.uint8, device="cuda"))
        ks = put(torch.zeros(B, H, Smax, device="cuda"))
        vs = put(torch.zeros(B, H, Smax, device="cuda"))
        o1 = put(torch.zeros(B, d, dtype=torch.bfloat16, device="cuda"))
        o2 = put(torch.zeros(B, d, dtype=torch.bfloat16, device="cuda"))
        D.kv_append_fp8(rows[:, d:2 * d], rows[:, 2 * d:], 3 * d, k8, v8, ks, vs, B, T - 1, H, hd, Smax, 0)
        ops.qkv_finish_fp8(slabs, slices, qkv, cos, sin, T - 1, k8, v8, ks, vs, B, H, hd, Smax)
        D.attn_decode_fp8(qkv, 3 * d, k8, v8, ks, vs, km, o1, B, H, hd, Smax, T, hd ** -0.5)
        D.attn_decode_rows_fp8(qkv, 3 * d, k8, v8, ks, vs, tab, B, km, o2, B, nb, H, hd, Smax, T, hd ** -0.5)
        torch.cuda.synchronize()
        res.append([t.clone() for t in (k8, v8, ks, vs, qkv, o1, o2)])
        del keep
    for a, b, nm in zip(res[0], res[1], ("k8", "v8", "ks", "vs", "qkv", "o1", "o2")):
        assert torch.equal(a, b), nm
    assert bool(torch.isfinite(res[1][5].float()).all()) and bool(torch.isfinite(res[1][6].float()).all())


def test_kv8_bad_arguments_are_refused():
    L = lib()
    for f in ("egomi_kv_append_fp8", "egomi_qkv_finish_fp8", "egomi_attn_decode_fp8", "egomi_attn_decode_rows_fp8"):
        getattr(L, f).restype = ctypes.c_int
    B, H, hd, Smax = 2, 2, 64, 16
    d = H * hd
    x = torch.zeros(B, 3 * d, dtype=torch.bfloat16, device="cuda")
    slabs = torch.zeros(1, B, 3 * d, device="cuda")
    cos, sin = (t.cuda() for t in ops.rope_tables(Smax, hd, 10000.0))
    c8 = torch.zeros(B, H, Smax, hd, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(B, H, Smax, device="cuda")
    out = torch.zeros(B, d, dtype=torch.bfloat16, device="cuda")
    tab = torch.zeros(B, Smax, dtype=torch.int32, device="cuda")
    nul = ctypes.c_void_p(None)

    def app(k=P(x), c=P(c8), s=P(sc), S_=1, hd_=hd, pos0=0, dt=1):
        return L.egomi_kv_append_fp8(k, P(x), c_i64(3 * d), c, P(c8), s, P(sc), c_i(B), c_i(S_), c_i(H), c_i(hd_), c_i(Smax), c_i(pos0), c_i(dt), S())

    def fin(q=P(x), c=P(c8), pos=0, dt=1, sl=1, hd_=hd):
        return L.egomi_qkv_finish_fp8(P(slabs), c_i(sl), q, c_i64(3 * d), P(cos), P(sin), c_i(pos), c, P(c8), P(sc), P(sc), c_i(B), c_i(H), c_i(hd_),
                                      c_i(Smax), c_i(dt), S())

    def att(q=P(x), c=P(c8), T=4, dt=1, hd_=hd, ldq=3 * d):
        return L.egomi_attn_decode_fp8(q, c_i64(ldq), c, P(c8), P(sc), P(sc), nul, c_i64(0), P(out), c_i64(d), c_i(B), c_i(H), c_i(hd_), c_i(Smax),
                                       c_i(T), c_f(0.1), c_i(dt), S())

    def rws(tb=P(tab), T=4, nb=2, n_phys=B, dt=1):
        return L.egomi_attn_decode_rows_fp8(P(x), c_i64(3 * d), P(c8), P(c8), P(sc), P(sc), tb, c_i64(Smax), c_i(n_phys), nul, c_i64(0), P(out),
                                            c_i64(d), c_i(B), c_i(nb), c_i(H), c_i(hd), c_i(Smax), c_i(T), c_f(0.1), c_i(dt), S())
    assert app() == 0 and fin() == 0 and att() == 0 and rws() == 0
    torch.cuda.synchronize()
    assert app(k=nul) == E_BADARG and app(c=nul) == E_BADARG and app(s=nul) == E_BADARG and app(dt=5) == E_BADARG
    assert app(S_=Smax + 1) == E_SHAPE and app(pos0=Smax) == E_SHAPE and app(pos0=-1) == E_SHAPE and app(hd_=48) == E_UNSUPPORTED
    assert fin(q=nul) == E_BADARG and fin(c=nul) == E_BADARG and fin(dt=5) == E_BADARG
    assert fin(pos=Smax) == E_SHAPE and fin(pos=-1) == E_SHAPE and fin(sl=0) == E_SHAPE and fin(hd_=48) == E_UNSUPPORTED
    assert att(q=nul) == E_BADARG and att(c=nul) == E_BADARG and att(dt=5) == E_BADARG
    assert att(T=0) == E_SHAPE and att(T=Smax + 1) == E_SHAPE and att(ldq=d - 8) == E_SHAPE and att(hd_=16) == E_UNSUPPORTED
    assert rws(tb=nul) == E_BADARG and rws(dt=5) == E_BADARG
    assert rws(nb=3) == E_SHAPE and rws(n_phys=0) == E_SHAPE and rws(T=Smax + 1) == E_SHAPE
