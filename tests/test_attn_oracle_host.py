"""CPU: the per-element metric of tests/attn_oracle.py accepts an emulation of the attention kernels' rounding (bf16 P and dS, fp32 sums, bf16
outputs), rejects tile-sized defects of the kind a wrong kernel produces, and the older global-scale criterion (max err <= tol * max |ref|)
lets at least one of those defects through — the gap the GPU module tests/test_gpu_attention_oracle.py closes."""
import pytest
import torch

from tests import attn_oracle as A


def _bf(x):
    return x.to(torch.bfloat16).double()


def _inputs(B, S, H, hd, seed, dist="normal"):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * H * hd, generator=g)
    dout = torch.randn(B * S, H * hd, generator=g)
    if dist == "peaked":
        qkv[:, :2 * H * hd] *= 2.2                                       # scores spread over about +-30
    q, k, v = A.split_qkv(qkv.bfloat16(), B, S, H, hd)
    return q, k, v, A.rows_to_bhsd(dout.bfloat16(), B, S, H, hd)


def _emulate_fwd(q, k, v, scale, causal, km):
    """fp32 scores, P = exp(s - max) rounded to bf16 for the PV product, l summed from the fp32 P, fp32 accumulation, bf16 output."""
    B, H, S, hd = q.shape
    keep = A.visible(B, S, causal, km)
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    s = s.masked_fill(~keep, float("-inf"))
    m = s.amax(-1, keepdim=True)
    dead = torch.isinf(m)
    p = torch.exp(s - torch.where(dead, torch.zeros_like(m), m)).masked_fill(~keep, 0.0)
    l = p.sum(-1, keepdim=True)
    o = (p.bfloat16().float() @ v.float()) / torch.where(l > 0, l, torch.ones_like(l))
    lse = torch.where(dead[..., 0], torch.full_like(m[..., 0], float("inf")), m[..., 0] + torch.log(l[..., 0]))
    return _bf(o), lse.double()


def _emulate_bwd(q, k, v, o, dout, lse, scale, causal, km):
    B, H, S, hd = q.shape
    keep = A.visible(B, S, causal, km)
    f = lambda t: t.float()                                              # noqa: E731
    s = (f(q) @ f(k).transpose(-1, -2)) * scale
    p = torch.exp(s - f(lse)[..., None]).masked_fill(~keep, 0.0)
    dp = f(dout) @ f(v).transpose(-1, -2)
    delta = (f(dout) * f(o)).sum(-1, keepdim=True)
    ds = (p * (dp - delta)).bfloat16().float()
    dv = p.bfloat16().float().transpose(-1, -2) @ f(dout)
    dq = scale * (ds @ f(k))
    dk = scale * (ds.transpose(-1, -2) @ f(q))
    return dict(dq=_bf(dq), dk=_bf(dk), dv=_bf(dv), delta=delta[..., 0].double())


CASES = [(1, 692, 2, True, 128, None, "normal"), (2, 200, 3, True, 128, "tail", "normal"), (2, 129, 2, False, 64, "holes", "normal"),
         (1, 300, 2, True, 128, None, "peaked"), (2, 97, 1, True, 64, "left", "normal")]


def _mask(kind, B, S):
    if kind is None:
        return None
    km = torch.ones(B, S, dtype=torch.uint8)
    if kind == "tail":
        km[-1, S - S // 5:] = 0
    elif kind == "holes":
        km[0, 2:4] = 0
        km[-1, S // 2] = 0
    elif kind == "left":
        km[-1, :S // 4] = 0
    return km


@pytest.fixture(scope="module")
def case692():
    B, S, H, causal, hd = 1, 692, 2, True, 128
    q, k, v, dout = _inputs(B, S, H, hd, 692)
    scale = hd ** -0.5
    fw = A.forward(q, k, v, scale, causal)
    o_in = _bf(fw["o"])
    bw = A.backward(q, k, v, o_in, dout, scale, causal)
    return dict(q=q, k=k, v=v, dout=dout, scale=scale, causal=causal, fw=fw, bw=bw, o_in=o_in)


@pytest.mark.parametrize("B,S,H,causal,hd,mask,dist", CASES)
def test_metric_accepts_the_kernels_rounding(B, S, H, causal, hd, mask, dist):
    q, k, v, dout = _inputs(B, S, H, hd, S + hd, dist)
    km = _mask(mask, B, S)
    scale = hd ** -0.5
    fw = A.forward(q, k, v, scale, causal, km)
    o, lse = _emulate_fwd(q, k, v, scale, causal, km)
    assert A.ratio(o, fw["o"], fw["e_o"]) < A.TAU / 2
    assert A.lse_ratio(lse, fw["lse"], fw["smax"]) < A.LSE_TOL
    if mask == "left" and causal:                                        # rows that see no key: O = 0, LSE = +inf, in oracle and emulation
        dead = fw["dead"][-1]
        assert bool(dead.any())
        assert bool((fw["o"][-1][:, dead] == 0).all()) and bool((fw["lse"][-1][:, dead] == float("inf")).all())
    o_in = _bf(fw["o"])
    bw = A.backward(q, k, v, o_in, dout, scale, causal, km)
    em = _emulate_bwd(q, k, v, o_in, dout, fw["lse"].float(), scale, causal, km)
    for n in ("dq", "dk", "dv", "delta"):
        assert A.ratio(em[n], bw[n], bw["e_" + n]) < A.TAU / 2, n


def test_oracle_backward_equals_float64_autograd():
    B, S, H, hd = 2, 70, 2, 64
    q, k, v, dout = _inputs(B, S, H, hd, 5)
    km = _mask("left", B, S)
    scale = 0.11
    keep = A.visible(B, S, True, km)
    live = keep.any(-1, keepdim=True)
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = ((qq @ kk.transpose(-1, -2)) * scale).masked_fill(~keep, float("-inf"))
    p = torch.softmax(s.masked_fill(~live, 0.0), -1).masked_fill(~keep, 0.0)
    o = p @ vv
    o.backward(dout)
    bw = A.backward(q, k, v, o.detach(), dout, scale, True, km)
    fw = A.forward(q, k, v, scale, True, km)
    torch.testing.assert_close(fw["o"], o.detach(), rtol=1e-12, atol=1e-12)
    for n, t in (("dq", qq), ("dk", kk), ("dv", vv)):
        torch.testing.assert_close(bw[n], t.grad, rtol=1e-10, atol=1e-12)


def test_rope_inverse_matches_the_rotation():
    from egoscaler_amd import ops
    cos, sin = ops.rope_tables(40, 64, 10000.0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 2, 40, 64, generator=g).double()
    half = 32
    c, s = cos.double(), sin.double()
    fwd = torch.cat([x[..., :half] * c - x[..., half:] * s, x[..., half:] * c + x[..., :half] * s], -1)     # HF apply_rotary_pos_emb
    back, _ = A.rope_inverse(fwd, fwd.abs(), cos, sin)
    torch.testing.assert_close(back, x, rtol=0, atol=1e-6)                  # fp32 tables: cos^2 + sin^2 = 1 to ~1e-7
    rot, e = A.rope_inverse(x, x.abs(), cos, sin)                            # the bound carried through the rotation covers the value
    assert bool((rot.abs() <= e + 1e-12).all())


def _rejects(got, ref, e):
    return not A.within(got, ref, e)


def test_metric_rejects_late_rows_scaled(case692):
    c = case692
    o = _bf(c["fw"]["o"]).clone()
    o[:, :, 600:] *= 0.8
    assert _rejects(o, c["fw"]["o"], c["fw"]["e_o"])


def test_metric_rejects_half_the_diagonal_tile(case692):
    """Rows >= 600: the probabilities of their own 32-key diagonal tile halved, LSE left correct."""
    c = case692
    q, k, v, scale = c["q"], c["k"], c["v"], c["scale"]
    S = q.shape[2]
    keep = A.visible(1, S, True, None)[0]
    p, _, _, _ = A._probs(q[0], k[0], keep, scale)
    qi = torch.arange(S)[:, None]
    ki = torch.arange(S)[None, :]
    diag = (ki // 32 == qi // 32) & (qi >= 600)
    o = _bf((p * torch.where(diag, 0.5, 1.0)) @ v[0])[None]
    assert _rejects(o, c["fw"]["o"], c["fw"]["e_o"])


def test_metric_rejects_a_v_tile_read_from_its_neighbour(case692):
    c = case692
    v2 = c["v"].clone()
    v2[:, :, 320:352] = c["v"][:, :, 352:384]
    o = _bf(A.forward(c["q"], c["k"], v2, c["scale"], True)["o"])
    assert _rejects(o, c["fw"]["o"], c["fw"]["e_o"])


@pytest.mark.parametrize("name", ["dv", "dk"])
def test_metric_rejects_the_last_32_keys_zeroed(case692, name):
    """The gap the metric closes: the global-scale check of test_fused_attention_backward (3e-2 of max |ref|) accepts a dV with its last 32
    keys zeroed; dK likewise."""
    bw = case692["bw"]
    got = _bf(bw[name]).clone()
    got[:, :, -32:] = 0
    assert _rejects(got, bw[name], bw["e_" + name])
    assert A.global_ok(got, bw[name], 3e-2)


def test_old_criterion_misses_dv_of_the_last_64_keys(case692):
    bw = case692["bw"]
    got = _bf(bw["dv"]).clone()
    got[:, :, -64:] = 0
    assert A.global_ok(got, bw["dv"], 3e-2)
    assert _rejects(got, bw["dv"], bw["e_dv"])


def test_metric_rejects_a_dropped_dq_row(case692):
    bw = case692["bw"]
    for row in (1, 345, 691):
        got = _bf(bw["dq"]).clone()
        got[:, :, row] = 0
        assert _rejects(got, bw["dq"], bw["e_dq"]), row


def test_lse_bound_sees_one_dropped_key(case692):
    c = case692
    km = torch.ones(1, 692, dtype=torch.uint8)
    km[0, 100] = 0
    fw = A.forward(c["q"], c["k"], c["v"], c["scale"], True, km)
    assert A.lse_ratio(fw["lse"], c["fw"]["lse"], c["fw"]["smax"]) > 10 * A.LSE_TOL


def test_metric_treats_rows_without_keys_exactly():
    e = torch.tensor([[0.0, 0.0], [1.0, 2.0]])
    ref = torch.zeros(2, 2)
    assert A.within(torch.zeros(2, 2), ref, e)
    assert not A.within(torch.tensor([[1e-2, 0.0], [0.0, 0.0]]), ref, e)
    assert not A.within(torch.tensor([[float("nan"), 0.0], [0.0, 0.0]]), ref, e)
    inf = float("inf")
    assert A.lse_ratio(torch.tensor([inf, 1.0]), torch.tensor([inf, 1.0]), torch.ones(2)) == 0.0
    assert A.lse_ratio(torch.tensor([0.0, 1.0]), torch.tensor([inf, 1.0]), torch.ones(2)) == inf
