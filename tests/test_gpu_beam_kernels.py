"""GPU: the beam-search kernels on their own.
  * egomi_attn_decode_rows (row-table attention) bit-equal to egomi_attn_decode on the physically gathered cache: bf16 / fp32,
    head_dim 32 / 64 / 128, T_len not a multiple of 16, masked prompt keys, every operand at the end of its own allocation.
  * egomi_beam_rows + egomi_beam_update against a few-line torch restatement of HF's beam-search helpers on random logits with ties
    (ties resolve to the lower flat index)."""
import numpy as np
import pytest
import torch

from egoscaler_amd import decode

pytestmark = pytest.mark.gpu
SEG = 2 << 20


def at_end(src, keep):
    """A copy of `src` whose last byte is the last byte of a fresh device allocation (tests/test_gpu_bounds.py's convention)."""
    n, es = src.numel(), src.element_size()
    nbytes = max(16 << 20, -(-n * es // SEG) * SEG)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    buf = torch.empty(nbytes // es, dtype=src.dtype, device="cuda")
    keep.append(buf)
    t = buf[buf.numel() - n:].view(src.shape)
    t.copy_(src)
    return t


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_attn_decode_rows_equals_gathered_cache(dtype, hd):
    g = torch.Generator().manual_seed(hd)
    Bi, nb, H, Smax, S0, T_len = 3, 4, 4, 80, 37, 53
    R, d = Bi * nb, H * hd
    kc0 = torch.randn(R, H, Smax, hd, generator=g).to(dtype).cuda()
    vc0 = torch.randn(R, H, Smax, hd, generator=g).to(dtype).cuda()
    qkv0 = torch.randn(R, 3 * d, generator=g).to(dtype).cuda()
    km0 = torch.ones(R, Smax, dtype=torch.uint8, device="cuda")
    km0[nb:2 * nb, 1:4] = 0                                           # item 1's prompt has masked keys
    tab = torch.empty(R, Smax, dtype=torch.int32)
    tab[:, :S0] = (torch.arange(R) // nb)[:, None]
    tab[:, S0:] = torch.randint(0, R, (R, Smax - S0), generator=g, dtype=torch.int32)
    tab0 = tab.cuda()
    t_idx = torch.arange(Smax).cuda()
    kg = kc0[tab0.long(), :, t_idx[None, :]].permute(0, 2, 1, 3).contiguous()     # [R, H, Smax, hd] gathered
    vg = vc0[tab0.long(), :, t_idx[None, :]].permute(0, 2, 1, 3).contiguous()
    ref = torch.full((R, d), 3.0, dtype=dtype, device="cuda")
    decode.attn_decode(qkv0, 3 * d, kg, vg, km0, ref, R, H, hd, Smax, T_len, hd ** -0.5)
    keep = []
    kc, vc, qkv, km, tb = (at_end(t, keep) for t in (kc0, vc0, qkv0, km0, tab0))
    out = at_end(torch.full((R, d), 3.0, dtype=dtype, device="cuda"), keep)
    decode.attn_decode_rows(qkv, 3 * d, kc, vc, tb, R, km, out, R, nb, H, hd, Smax, T_len, hd ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def _hf_step(lp, run_s, nb, K, V, cur_len, S0, max_len, eos, lpen, es, fin_s, fin_f, heur):
    """One step of HF's _beam_search on [B, nb, V] processed log-probs (greedy), ties -> lower index (stable sort)."""
    B = lp.shape[0]
    acc = (lp + run_s[:, :, None]).reshape(B, nb * V)
    order = torch.sort(acc, dim=1, descending=True, stable=True)
    tk_s, tk_i = order[0][:, :K], order[1][:, :K]
    tok = tk_i % V
    hit = (tok == eos) | (cur_len + 1 >= max_len)
    rs = tk_s + hit.float() * -1e9
    nxt = torch.sort(rs, dim=1, descending=True, stable=True)[1][:, :nb]
    run_new = torch.gather(rs, 1, nxt)
    f = tk_s / float((cur_len + 1 - S0) ** lpen)
    f = f + (fin_f.all(1, keepdim=True) & (es == 1)).float() * -1e9
    f = f + (~heur).float() * -1e9
    did = hit & (torch.arange(K) < nb)[None]
    f = f + (~did).float() * -1e9
    ms = torch.cat([fin_s, f], 1)
    mi = torch.sort(ms, dim=1, descending=True, stable=True)[1][:, :nb]
    return tk_i, nxt, run_new, torch.gather(ms, 1, mi), mi


def test_beam_rows_and_update_match_torch_restatement():
    g = torch.Generator().manual_seed(0)
    Bi, nb, V, S0, Smax = 3, 4, 1000, 5, 16
    R, K, eos = Bi * nb, 2 * nb, 7
    lg = (torch.randn(R, V, generator=g) * 3).round()                 # integer logits: many exact ties
    lg[:, eos] += 2.0
    run_s = torch.tensor([[0.0, -0.5, -1.0, -1.5]] * Bi)
    seq = torch.zeros(R, Smax, dtype=torch.int64)
    seq[:, :S0] = torch.randint(0, V, (R, S0), generator=g)
    dev = "cuda"
    sc = torch.empty(R, V, device=dev)
    ck, cs, ct = torch.empty(R, K, device=dev), torch.empty(R, K, device=dev), torch.empty(R, K, dtype=torch.int32, device=dev)
    ctl = torch.zeros(8, dtype=torch.int32, device=dev)
    ctl[0] = 1
    rsd = run_s.reshape(-1).cuda()
    seqd = seq.cuda()
    decode.beam_rows(lg.cuda(), 1, R, nb, sc, seqd, S0, repetition_penalty=1.0, temperature=1.0, top_k=0, top_p=1.0, min_keep=2, do_sample=False,
                     rng=None, draw=0, run_score=rsd, cand_key=ck, cand_score=cs, cand_tok=ct, ctl=ctl)
    lp = torch.log_softmax(lg, -1)
    assert float((sc.cpu() - lp).abs().max()) < 1e-5
    # every row's K best by (accumulated score desc, token asc)
    acc = sc.cpu() + run_s.reshape(-1)[:, None]
    want_tok = torch.sort(acc, dim=1, descending=True, stable=True)[1][:, :K]
    assert torch.equal(ct.cpu().long(), want_tok)
    fin_s, fin_f = torch.full((Bi, nb), -1e9), torch.zeros(Bi, nb, dtype=torch.bool)
    heur = torch.ones(Bi, 1, dtype=torch.bool)
    fin_seq, bidx, fin_bidx = seqd.clone(), torch.full((R, Smax), -1, dtype=torch.int32, device=dev), torch.full((R, Smax), -1, dtype=torch.int32, device=dev)
    kv = torch.zeros(R, Smax, dtype=torch.int32, device=dev)
    kv[:, :S0] = (torch.arange(R, device=dev, dtype=torch.int32) // nb)[:, None]
    fsd, ffd, hd_, tok = torch.full((R,), -1e9, device=dev), torch.zeros(R, dtype=torch.int32, device=dev), torch.ones(Bi, dtype=torch.int32, device=dev), \
        torch.zeros(R, dtype=torch.int64, device=dev)
    decode.beam_update(Bi, nb, V, ck, cs, ct, S0, S0, Smax, eos, 1.0, False, seqd, fin_seq, bidx, fin_bidx, kv, rsd, fsd, ffd, hd_, tok, ctl)
    tk_i, nxt, run_new, fin_new, mi = _hf_step(sc.cpu().view(Bi, nb, V), run_s, nb, K, V, S0, S0, Smax, eos, 1.0, 0, fin_s, fin_f, heur)
    assert torch.equal(rsd.cpu().view(Bi, nb), run_new)
    assert torch.equal(fsd.cpu().view(Bi, nb), fin_new)
    par = torch.gather(tk_i, 1, nxt) // V                              # parent beam and token of every new running beam
    ntok = torch.gather(tk_i, 1, nxt) % V
    assert torch.equal(tok.cpu().view(Bi, nb), ntok)
    rows = (par + torch.arange(Bi)[:, None] * nb).reshape(-1)
    assert torch.equal(seqd.cpu()[:, :S0], seq[rows, :S0]) and torch.equal(seqd.cpu()[:, S0], ntok.reshape(-1))
    assert torch.equal(bidx.cpu()[:, 0].long(), rows) and torch.equal(kv.cpu()[:, S0], torch.arange(R, dtype=torch.int32))
    assert int(ctl[1]) == 1 and int(ctl[0]) == 1


def _hf_warp(lp, temperature, top_k, top_p, min_keep):
    """HF's own warpers on processed log-probs, built as _get_logits_processor builds them for beam sampling."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = lp.clone()
    ids = torch.zeros(lp.shape[0], 1, dtype=torch.long)
    if temperature != 1.0:
        s = TemperatureLogitsWarper(temperature)(ids, s)
    if top_k:
        s = TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=min_keep)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=min_keep)(ids, s)
    return s


@pytest.mark.parametrize("draw", [0, 5])
@pytest.mark.parametrize("warp", [(0.7, 50, 0.95), (1.0, 1, 1.0), (1.0, 0, 0.01)])
def test_beam_rows_sampling_is_gumbel_top_k(draw, warp):
    """do_sample=1: the processed rows equal HF's warpers with min_tokens_to_keep = 2 (top_k=1 and a tiny top_p keep TWO tokens), and
    every row's candidates are exactly the ordered top K of scores + run_score + gumbel_noise(seed; logical row, token, draw counter)."""
    from oracle import sampling as OS
    temperature, top_k, top_p = warp
    g = torch.Generator().manual_seed(11 + draw)
    Bi, nb, V = 2, 4, 3000
    R, K, seed, base = Bi * nb, 2 * nb, 987654321, 3
    lg = torch.randn(R, V, generator=g) * 2.5
    run_s = -torch.rand(R, generator=g) * 3
    sc = torch.empty(R, V, device="cuda")
    ck, cs, ct = torch.empty(R, K, device="cuda"), torch.empty(R, K, device="cuda"), torch.empty(R, K, dtype=torch.int32, device="cuda")
    rng = torch.tensor([seed, base], dtype=torch.int64, device="cuda")
    decode.beam_rows(lg.cuda(), 1, R, nb, sc, None, 0, repetition_penalty=1.0, temperature=temperature, top_k=top_k, top_p=top_p, min_keep=2,
                     do_sample=True, rng=rng, draw=draw, run_score=run_s.cuda(), cand_key=ck, cand_score=cs, cand_tok=ct, ctl=None)
    got = sc.cpu()
    want = _hf_warp(torch.log_softmax(lg, -1), temperature, top_k, top_p, 2)
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(got))
    if top_k == 1 or top_p < 0.05:
        assert int(fin.sum(1).min()) == 2 and int(fin.sum(1).max()) == 2          # min_tokens_to_keep = 2 decides the support
    assert float((got[fin] - want[fin]).abs().max()) < 1e-5 * float(want[fin].abs().max())
    noise = torch.from_numpy(OS.gumbel_noise(R, V, seed, base + draw))
    key = (got + run_s[:, None]) + noise
    flat = torch.arange(R)[:, None] % nb * V + torch.arange(V)[None, :]
    for r in range(R):
        order = sorted(range(V), key=lambda c: (-float(key[r, c]), int(flat[r, c])))[:K]
        assert ct[r].cpu().tolist() == order, r
        assert torch.allclose(ck[r].cpu(), key[r, order], rtol=0, atol=1e-5)
        assert torch.equal(cs[r].cpu(), got[r, order] + run_s[r])
