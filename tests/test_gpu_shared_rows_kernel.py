"""GPU: egomi_attn_decode_shared_rows (csrc/shared.hip) on its own through the C-ABI, against the float64 oracle tests/attn_oracle.decode
on the per-row cache built on the CPU (the prompt keys of the row's clip, then the suffix keys gathered through the row table), judged per
element with that module's criterion within(got, ref, e_o) (TAU = 1.5e-2, PHI = 1e-3), as tests/test_gpu_shared_attn_kernel.py does and
on its _case geometry (B = 3, H = 2; clip 1 with masked leading prompt keys, clip 2 with a fully masked prompt; every operand at the end
of its own allocation).
  * bf16 (MFMA prompt phase at hd 64 / 128, VALU at hd 32) and fp32; hd 32 / 64 / 128; K in {1, 2, 4, 5, 32} beams per clip (32, 16, 8, 6
    and 1 suffix slices per query); S0 = 37 and 540; T_len in {1, 3, 53, 157} with Tmax = T_len + 5: one key, fewer keys than slices, and
    two lengths that are no multiple of the slice count or of 4.
  * tables: random rows over all of [0, n_phys) (other clips' rows included); a real beam tree (the rows of a clip share ancestor
    prefixes, built as egomi_beam_update builds it); random with entries at -1 and n_phys, which are masked keys.  The suffix caches carry
    one NaN row before physical row 0 and one after row n_phys - 1, the rows those entries would alias, so a read of either shows.  In
    that variant every entry of row 2 K is masked: with its clip's prompt fully masked the row sees no key and must give exactly 0.
  * the same call twice is bit-equal; permuting the beams of a clip (queries and table rows together) permutes the output rows bit for
    bit; two rows with equal query and equal table rows give equal bits.
  * argument checks return the documented codes.
Worst ratio (err - PHI max E) / E measured on an MI355X over all cases: see MEASURED below (TAU = 1.5e-2 is the bound)."""
import itertools

import pytest
import torch

from egoscaler_amd import decode
from egoscaler_amd._lib import EgomiError
from tests import attn_oracle as ao
from tests.test_gpu_shared_attn_kernel import _case, at_end

pytestmark = pytest.mark.gpu
MEASURED = "bf16 2.5e-3 (hd 64, K = 2, S0 = 37, suffix 3, tree table; hd 32 and hd 128 2.4e-3), fp32 0 (under the PHI floor)"
WORST = {}                                   # (dtype, hd) -> worst ratio over the cases run so far
S0S, TLS = (37, 540), (1, 3, 53, 157)


def _tables(K, Tl, R, seed):
    """{name: int32 [R, Tl]}: physical suffix row of every suffix key of every logical row."""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(0, R, (R, Tl), generator=g, dtype=torch.int32)
    tree = torch.zeros(R, Tl, dtype=torch.int32)
    own = torch.arange(R, dtype=torch.int32)
    for t in range(Tl):                                              # egomi_beam_update: gather the table by parent, then [r, t] = r
        parent = (own // K) * K + torch.randint(0, K, (R,), generator=g, dtype=torch.int32)
        tree = tree[parent.long()]
        tree[:, t] = own
    holes = torch.randint(0, R, (R, Tl), generator=g, dtype=torch.int32)
    hit = torch.rand(R, Tl, generator=g)
    holes[hit < 0.06] = -1
    holes[hit > 0.94] = R
    holes[0, 0] = -1
    holes[R - 1, Tl - 1] = R
    holes[2 * K] = torch.where(torch.arange(Tl) % 2 == 0, -1, R).int()          # with clip 2's masked prompt: a row without any key
    return {"random": rnd, "tree": tree, "holes": holes}


def _oracle(t, km, tab, K, S0, Tl, hd):
    """float64 reference on the per-row cache: prompt keys of the row's clip, then the suffix keys the table names."""
    R, H = t["q"].shape[0], t["kp"].shape[1]
    clip = torch.arange(R) // K
    ok = (tab >= 0) & (tab < R)
    rows = torch.where(ok, tab, torch.zeros_like(tab)).long()
    cols = torch.arange(Tl)[None, :]
    ks = t["ks"][rows, :, cols].permute(0, 2, 1, 3).double()          # [R, Tl, H, hd] -> [R, H, Tl, hd]
    vs = t["vs"][rows, :, cols].permute(0, 2, 1, 3).double()
    kc = torch.cat([t["kp"][clip, :, :S0].double(), ks], 2)
    vc = torch.cat([t["vp"][clip, :, :S0].double(), vs], 2)
    mask = torch.cat([km[clip, :S0], ok.to(torch.uint8)], 1)
    return ao.decode(t["q"].double().view(R, H, hd), kc, vc, hd ** -0.5, S0 + Tl, key_mask=mask)


def _guarded(x):
    """x [R, H, Tmax, hd] with one NaN row before row 0 and one after row R - 1: what table entries -1 and R would alias."""
    nan = torch.full_like(x[:1], float("nan"))
    return torch.cat([nan, x, nan], 0)


class _Dev:
    """The operands of one case on the device, each at the end of its own allocation; the suffix caches between their NaN guard rows."""

    def __init__(self, t, km, ends=True):
        self.keep = []
        self.put = (lambda x: at_end(x.cuda(), self.keep)) if ends else (lambda x: x.cuda())
        self.q, self.kp, self.vp, self.km = (self.put(x) for x in (t["q"], t["kp"], t["vp"], km))
        self.ks, self.vs = self.put(_guarded(t["ks"]))[1:-1], self.put(_guarded(t["vs"]))[1:-1]

    def run(self, tab, K_, S0_, Tl_, hd_, geom, q=None, **kw):
        """One call; kw overrides single arguments of it (the argument checks)."""
        B, H, Sp, Tmax, R, d = geom
        a = dict(n_phys=R, B=B, K=K_, H=H, hd=hd_, Sp=Sp, S0=S0_, Tmax=Tmax, T_len=Tl_)
        a.update(kw)
        q = self.q if q is None else q
        out = self.put(torch.full((R, d), 3.0, dtype=q.dtype))
        tabd = None if tab is None else self.put(tab)
        decode.attn_decode_shared_rows(q, d, self.kp, self.vp, self.km, self.ks, self.vs, tabd, a["n_phys"], out, a["B"], a["K"], a["H"], a["hd"],
                                       a["Sp"], a["S0"], a["Tmax"], a["T_len"], hd_ ** -0.5)
        torch.cuda.synchronize()
        return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("K", [1, 2, 4, 5, 32])
def test_shared_rows_attention_vs_float64_oracle(dtype, hd, K):
    worst = 0.0
    for S0, Tl in itertools.product(S0S, TLS):
        t, km, geom = _case(dtype, hd, K, S0, Tl)
        H, R = geom[1], geom[4]
        dev = _Dev(t, km)
        for name, tab in _tables(K, Tl, R, seed=hd + K + S0 + Tl).items():
            out = dev.run(tab, K, S0, Tl, hd, geom)
            ref, e = _oracle(t, km, tab, K, S0, Tl, hd)
            r = ao.ratio(out.view(-1, H, hd), ref, e)
            print(f"shared rows attn {str(dtype)[6:]} hd={hd} K={K} S0={S0} suffix={Tl} table={name}: worst ratio {r:.3e} (TAU {ao.TAU})")
            worst = max(worst, r)
            assert ao.within(out.view(-1, H, hd), ref, e), (S0, Tl, name, r)
            if name == "holes":                                      # masked prompt, every table entry masked: no key at all
                assert bool((out[2 * K] == 0).all()), (S0, Tl)
    WORST[dtype, hd] = max(WORST.get((dtype, hd), 0.0), worst)
    print(f"shared rows attn {str(dtype)[6:]} hd={hd} K={K}: worst over cases {worst:.3e}; {str(dtype)[6:]} hd={hd} over the K run so far "
          f"{WORST[dtype, hd]:.3e}")


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 128), (torch.bfloat16, 64), (torch.bfloat16, 32), (torch.float32, 32), (torch.float32, 128)])
@pytest.mark.parametrize("K,Tl", [(4, 157), (5, 53), (2, 3)])
def test_replay_is_bit_equal_and_rows_do_not_depend_on_their_slot(dtype, hd, K, Tl):
    S0 = 540
    t, km, geom = _case(dtype, hd, K, S0, Tl, seed=7)
    B, R = geom[0], geom[4]
    dev = _Dev(t, km, ends=False)
    for name, tab in _tables(K, Tl, R, seed=11).items():
        a = dev.run(tab, K, S0, Tl, hd, geom)
        b = dev.run(tab, K, S0, Tl, hd, geom)
        assert torch.equal(a, b), name
        g = torch.Generator().manual_seed(3)
        perm = torch.cat([b_ * K + torch.randperm(K, generator=g) for b_ in range(B)])
        while torch.equal(perm, torch.arange(R)):
            perm = torch.cat([b_ * K + torch.randperm(K, generator=g) for b_ in range(B)])
        c = dev.run(tab[perm], K, S0, Tl, hd, geom, q=t["q"][perm].cuda())            # the physical suffix rows stay where they are
        assert torch.equal(c, a[perm.cuda()]), name
        # row 1 takes row 0's query and table row: equal bits in another slot, and row 0 does not depend on its neighbour
        q2, tab2 = t["q"].clone(), tab.clone()
        q2[1], tab2[1] = q2[0], tab2[0]
        d = dev.run(tab2, K, S0, Tl, hd, geom, q=q2.cuda())
        assert torch.equal(d[1], d[0]) and torch.equal(d[0], a[0]), name


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 128), (torch.float32, 32)])
def test_row_without_any_key_gives_zero_and_no_suffix_is_allowed(dtype, hd):
    K, S0 = 4, 37
    t, km, geom = _case(dtype, hd, K, S0, 4)
    B, H, Sp, Tmax, R, d = geom
    dev = _Dev(t, km, ends=False)
    out = dev.run(None, K, S0, 0, hd, geom)                          # T_len = 0: the table may be NULL
    assert bool((out[2 * K:] == 0).all())                            # clip 2: prompt fully masked, no suffix
    clip = torch.arange(R) // K
    ref, e = ao.decode(t["q"].double().view(R, H, hd), t["kp"][clip].double(), t["vp"][clip].double(), hd ** -0.5, S0, key_mask=km[clip])
    assert ao.within(out.view(R, H, hd), ref, e)


def test_argument_checks():
    hd, K, S0, Tl = 32, 4, 37, 6
    t, km, geom = _case(torch.float32, hd, K, S0, Tl)
    R = geom[4]
    dev = _Dev(t, km, ends=False)
    tab = _tables(K, Tl, R, seed=1)["tree"]
    dev.run(tab, K, S0, Tl, hd, geom)
    Sp, Tmax = geom[2], geom[3]
    for bad in (dict(K=0), dict(K=33), dict(S0=Sp + 1), dict(S0=0), dict(T_len=Tmax + 1), dict(T_len=-1), dict(n_phys=0)):
        with pytest.raises(EgomiError, match="shape"):
            dev.run(tab, K, S0, Tl, hd, geom, **bad)
    with pytest.raises(EgomiError, match="shape"):                   # a table narrower than T_len
        dev.run(tab[:, :Tl - 1].contiguous(), K, S0, Tl, hd, geom)
    with pytest.raises(EgomiError, match="bad argument"):            # suffix keys without a table
        dev.run(None, K, S0, Tl, hd, geom)
    with pytest.raises(EgomiError, match="not supported"):
        dev.run(tab, K, S0, Tl, hd, geom, hd=16)
