"""GPU: egomi_attn_suffix_shared (csrc/shared.hip) on its own, against the float64 oracle tests/attn_oracle.decode.  Every query
(b, j, t) is one oracle row over the concatenated cache of its candidate (prompt keys of clip b, then suffix keys of row b*K + j) with a
key mask that carries both the prompt mask and the causal cut (suffix keys <= t), judged per element with within(got, ref, e_o)
(TAU = 1.5e-2, PHI = 1e-3).
  * bf16 (MFMA form at hd 64 / 128, VALU form at hd 32) and fp32 (VALU form, hd 32 / 128); B = 3, H = 2; per (dtype, hd) the cases
    (K, T, S0) of CASES: K in {1, 3, 32}, T in {1, 31, 33, 70} (a partial tile, one query past a tile, several tiles), S0 in {1, 37, 540};
    Sp = S0 + 3, Tmax = T + 5; clip 1 has masked leading prompt keys, clip 2's prompt is fully masked; every operand at the end of its own
    allocation.
  * the same call twice is bit-equal; permuting a clip's candidates (queries and suffix rows together) permutes the output bit for bit;
    the T = 33 call on truncated data equals rows t < 33 of the T = 70 call and K = 3 of the same candidates equals those rows of K = 32,
    bit for bit (a row's bits do not depend on K, T, j or its neighbours in the tile).
  * NaN in every key / value the kernel must not read (suffix positions >= T, suffix positions > t for the rows t <= t*, prompt positions
    >= S0) changes no bit of the rows concerned.
  * argument checks.
Worst ratio (err - PHI max E) / E measured on an MI355X over all cases: see MEASURED below (TAU = 1.5e-2 is the bound)."""
import pytest
import torch

from egoscaler_amd import decode
from egoscaler_amd._lib import EgomiError
from tests import attn_oracle as ao
from tests.test_gpu_shared_attn_kernel import at_end

pytestmark = pytest.mark.gpu
MEASURED = "bf16 2.25e-3 (hd 64, K = 1, T = 70, S0 = 540; hd 128 2.0e-3, hd 32 1.8e-3), fp32 0 (under the PHI floor)"
FORMS = [(torch.bfloat16, 32), (torch.bfloat16, 64), (torch.bfloat16, 128), (torch.float32, 32), (torch.float32, 128)]
CASES = [(1, 70, 540), (3, 33, 37), (32, 31, 1), (3, 1, 540)]            # (K, T, S0): every value of every axis at least once
B, H = 3, 2


def _case(dtype, hd, K, T, S0, seed=0, Tmax=None):
    g = torch.Generator().manual_seed(1000 * hd + 10 * K + S0 + T + seed)
    Sp, Tmax, R, d = S0 + 3, T + 5 if Tmax is None else Tmax, B * K, H * hd
    t = dict(q=torch.randn(R, T, d, generator=g), kp=torch.randn(B, H, Sp, hd, generator=g), vp=torch.randn(B, H, Sp, hd, generator=g),
             ks=torch.randn(R, H, Tmax, hd, generator=g), vs=torch.randn(R, H, Tmax, hd, generator=g))
    t = {n: v.to(dtype) for n, v in t.items()}
    km = torch.ones(B, Sp, dtype=torch.uint8)
    km[1, :5] = 0                                                    # left padding (all of the prompt at S0 = 1)
    km[2, :] = 0                                                     # a prompt that shows nothing: the queries live on their suffix alone
    return t, km


def _oracle(t, km, K, T, S0, hd, chunk=256):
    """o, e_o float64 [R*T, H, hd]: one ao.decode row per query over its candidate's concatenated cache."""
    R = t["q"].shape[0]
    clip = torch.arange(R) // K
    kc = torch.cat([t["kp"][clip, :, :S0].double(), t["ks"][:, :, :T].double()], 2)      # [R, H, S0 + T, hd]
    vc = torch.cat([t["vp"][clip, :, :S0].double(), t["vs"][:, :, :T].double()], 2)
    q = t["q"][:, :T].double().reshape(R * T, H, hd)
    cand, pos = torch.arange(R * T) // T, torch.arange(R * T) % T
    mask = torch.cat([km[clip[cand], :S0], (torch.arange(T)[None, :] <= pos[:, None]).to(torch.uint8)], 1)
    rows = cand[:, None].expand(R * T, S0 + T)
    o, e = [], []
    for c0 in range(0, R * T, chunk):
        sl = slice(c0, c0 + chunk)
        oc, ec = ao.decode(q[sl], kc, vc, hd ** -0.5, S0 + T, key_mask=mask[sl], kv_row=rows[sl])
        o.append(oc)
        e.append(ec)
    return torch.cat(o), torch.cat(e)


def _run(t, km, K, T, S0, hd, keep, ends=False):
    R, d, Sp, Tmax = t["ks"].shape[0], H * hd, t["kp"].shape[2], t["ks"].shape[2]
    put = (lambda x: at_end(x.cuda(), keep)) if ends else (lambda x: x.cuda())
    dev = {n: put(v.contiguous()) for n, v in t.items() if n != "q"}
    q = put(t["q"][:, :T].reshape(R * T, d).contiguous())
    kmd = put(km)
    out = put(torch.full((R * T, d), 3.0, dtype=t["q"].dtype))
    decode.attn_suffix_shared(q, d, dev["kp"], dev["vp"], kmd, dev["ks"], dev["vs"], out, R // K, K, H, hd, Sp, S0, Tmax, T, hd ** -0.5)
    torch.cuda.synchronize()
    return out.view(R, T, d)


@pytest.mark.parametrize("dtype,hd", FORMS)
def test_suffix_attention_vs_float64_oracle(dtype, hd):
    worst = 0.0
    for K, T, S0 in CASES:
        t, km = _case(dtype, hd, K, T, S0)
        keep = []
        out = _run(t, km, K, T, S0, hd, keep, ends=True)
        ref, e = _oracle(t, km, K, T, S0, hd)
        r = ao.ratio(out.reshape(-1, H, hd), ref, e)
        print(f"suffix attn {str(dtype)[6:]} hd={hd} K={K} T={T} S0={S0}: worst ratio {r:.3e} (TAU {ao.TAU})")
        worst = max(worst, r)
        assert ao.within(out.reshape(-1, H, hd), ref, e), (K, T, S0, r)
    print(f"suffix attn {str(dtype)[6:]} hd={hd}: worst over cases {worst:.3e}")


@pytest.mark.parametrize("dtype,hd", FORMS)
def test_replay_is_bit_equal_and_rows_do_not_depend_on_K_T_or_slot(dtype, hd):
    K, T, S0 = 32, 70, 37
    t, km = _case(dtype, hd, K, T, S0, seed=7)
    keep = []
    a = _run(t, km, K, T, S0, hd, keep)
    assert torch.equal(a, _run(t, km, K, T, S0, hd, keep))
    g = torch.Generator().manual_seed(3)
    perm = torch.cat([b_ * K + torch.randperm(K, generator=g) for b_ in range(B)])
    assert not torch.equal(perm, torch.arange(B * K))
    tp = dict(t, q=t["q"][perm], ks=t["ks"][perm], vs=t["vs"][perm])
    assert torch.equal(_run(tp, km, K, T, S0, hd, keep), a[perm.cuda()])
    # T = 33 on the truncated queries (the same caches: keys 33 .. are now beyond T)
    assert torch.equal(_run(t, km, K, 33, S0, hd, keep), a[:, :33])
    # K = 3 of the same candidates: other tiles, other neighbours, the same bits
    sel = torch.cat([b_ * K + torch.arange(3) for b_ in range(B)])
    t3 = dict(t, q=t["q"][sel], ks=t["ks"][sel], vs=t["vs"][sel])
    assert torch.equal(_run(t3, km, 3, T, S0, hd, keep), a[sel.cuda()])
    # query (b, j, t) is the decode query of row b*K + j at T_len = t + 1 (include/egomi.h): the decode kernel's bits
    dev = {n: v.cuda() for n, v in t.items()}
    for ts in (0, 32, 69):
        q, out = dev["q"][:, ts].contiguous(), torch.empty(B * K, H * hd, dtype=dtype, device="cuda")
        decode.attn_decode_shared(q, H * hd, dev["kp"], dev["vp"], km.cuda(), dev["ks"], dev["vs"], out, B, K, H, hd, S0 + 3, S0, T + 5, ts + 1,
                                  hd ** -0.5)
        assert torch.equal(out, a[:, ts]), ts


@pytest.mark.parametrize("dtype,hd", FORMS)
def test_keys_that_must_not_be_read_are_not_read(dtype, hd):
    K, T, S0 = 3, 33, 37
    t, km = _case(dtype, hd, K, T, S0, seed=11)
    keep = []
    clean = _run(t, km, K, T, S0, hd, keep)
    assert bool(torch.isfinite(clean).all())
    nan = float("nan")
    bad = {n: v.clone() for n, v in t.items()}
    for n in ("kp", "vp"):
        bad[n][:, :, S0:] = nan                                      # prompt positions >= S0 (Sp = S0 + 3)
    for n in ("ks", "vs"):
        bad[n][:, :, T:] = nan                                       # suffix positions >= T (Tmax = T + 5)
    got = _run(bad, km, K, T, S0, hd, keep)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)
    for ts in (0, 16, 31):                                           # suffix positions > t*: rows t <= t* may not notice
        worse = {n: v.clone() for n, v in bad.items()}
        for n in ("ks", "vs"):
            worse[n][:, :, ts + 1:] = nan
        got = _run(worse, km, K, T, S0, hd, keep)[:, :ts + 1]
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean[:, :ts + 1]), ts


def test_argument_checks():
    hd, K, T, S0 = 32, 3, 4, 37
    t, km = _case(torch.float32, hd, K, T, S0)
    R, d, Sp, Tmax = B * K, H * hd, S0 + 3, T + 5
    dev = {n: v.cuda() for n, v in t.items()}
    q, kmd = dev["q"].reshape(R * T, d), km.cuda()
    out = torch.zeros(R * T, d, device="cuda")

    def call(**kw):
        a = dict(K=K, hd=hd, Sp=Sp, S0=S0, Tmax=Tmax, T=T)
        a.update(kw)
        decode.attn_suffix_shared(q, d, dev["kp"], dev["vp"], kmd, dev["ks"], dev["vs"], out, B, a["K"], H, a["hd"], a["Sp"], a["S0"], a["Tmax"],
                                  a["T"], hd ** -0.5)
    call()
    for bad in (dict(K=0), dict(K=33), dict(T=0), dict(T=Tmax + 1), dict(S0=0), dict(S0=Sp + 1)):
        with pytest.raises(EgomiError, match="shape"):
            call(**bad)
    with pytest.raises(EgomiError, match="not supported"):
        call(hd=16)
