"""float64 oracle and per-element error metric for the attention kernels (csrc/attention.hip, the decode attention of
attn_decode.hip).  A plain module, not a test file: tests/test_attn_oracle_host.py checks the metric on the CPU,
tests/test_gpu_attention_oracle.py runs every kernel form against it.

Reference.  Everything is computed in float64 on the CPU from the values the kernel receives (bf16 q|k|v, dout, the bf16-rounded O and the
fp32 LSE handed to the backward; the dequantised fp8 cache of the decode kernels).  A query row that sees no key at all (left padding under
causal masking, a sample whose keys are all masked) follows the kernels' convention (attention.hip: `inv = l > 0 ? 1/l : 0`, LSE = +inf):
O = 0, LSE = +inf, and it contributes nothing to any gradient.

Metric.  Every element is bounded by the magnitude of the terms it is made of, not by the tensor's maximum:
    O[q,j]   E = sum_k P_qk |V_kj|
    dV[k,j]  E = sum_q P_qk |dO_qj|
    dQ[q,j]  E = scale sum_k P_qk (|dP_qk| + |delta_q|) |K_kj|
    dK[k,j]  E = scale sum_q P_qk (|dP_qk| + |delta_q|) |Q_qj|
    delta[q] E = sum_j |dO_qj| |O_qj|
(with the inverse-RoPE epilogue, E is carried through the rotation with |cos| and |sin|).  A tensor passes when
    |got - ref| <= TAU * E + PHI * max(E)
holds for every element; PHI is a floor for elements whose exact value and terms vanish (causal dQ of row 0).  LSE has an absolute bound
per row: |got - ref| <= LSE_TOL * (1 + max_k |s_qk|), s the scaled scores of the row.

Bounds, from MI355X measurements of tests/test_gpu_attention_oracle.py (worst value over the whole module: every case, every form, both
head dims, the decode kernels included).  TAU and LSE_TOL are about 3x the worst measured:
    (err - PHI max E) / E   measured 5.1e-3 (O, forward form 3, peaked scores; dQ 4.7e-3, dV 3.0e-3, dK 2.2e-3, decode 2.2e-3)   TAU = 1.5e-2
    LSE                     measured 3.5e-7 (per row, relative to 1 + max|s|; S = 4096)                                       LSE_TOL = 1e-6
    floor                   PHI = 1e-3; with PHI = 1e-4 the worst measured ratio is 9.9e-3 (dQ with RoPE, peaked scores), still under TAU
A CPU emulation of the kernels' rounding (bf16 P and dS, fp32 sums, bf16 output) gives 2.2e-3 on the 692-key causal case.
The simulated defects of test_attn_oracle_host.py (a late row scaled by 0.8, half the diagonal tile's P, a V tile read from its
neighbour, the dV / dK of the last 32 keys zeroed, a dQ row dropped) give err / E between 0.05 and 0.8."""
import torch

TAU = 1.5e-2
PHI = 1e-3
LSE_TOL = 1e-6

_CHUNK = 1 << 25          # elements of one [heads, S, S] block of P: bounds the oracle's memory at the bench shape


def split_qkv(qkv, B, S, H, hd):
    """qkv [B*S, >= 3*H*hd] (q|k|v column blocks) -> q, k, v float64 [B, H, S, hd]."""
    d = H * hd
    x = qkv[:, :3 * d].double().reshape(B, S, 3, H, hd)
    return tuple(x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))


def rows_to_bhsd(x, B, S, H, hd):
    return x[:, :H * hd].double().reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()


def bhsd_to_rows(x):
    B, H, S, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * hd)


def visible(B, S, causal, key_mask):
    """[B, 1, S, S] bool: query q sees key k."""
    keep = torch.ones(S, S, dtype=torch.bool)
    if causal:
        keep = torch.tril(keep)
    keep = keep[None, None].expand(B, 1, S, S)
    if key_mask is not None:
        keep = keep & key_mask.bool().cpu()[:, None, None, :]
    return keep


def _heads(H, S):
    n = max(1, _CHUNK // max(1, S * S))
    return [(h0, min(H, h0 + n)) for h0 in range(0, H, n)]


def _probs(q, k, keep, scale):
    """P [.., S, S] float64, LSE [.., S] (+inf for rows that see nothing), max |s| per row."""
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(s, -1)
    dead = ~keep.any(-1).expand_as(lse)
    p = torch.exp(s - torch.where(dead, torch.zeros_like(lse), lse)[..., None])
    p = p.masked_fill(~keep, 0.0)
    smax = s.masked_fill(~keep, 0.0).abs().amax(-1)
    return p, torch.where(dead, torch.full_like(lse, float("inf")), lse), smax, dead


def forward(q, k, v, scale, causal, key_mask=None):
    """q, k, v float64 [B, H, S, hd] -> dict: o, e_o [B, H, S, hd]; lse, smax [B, H, S]; dead [B, S] (rows that see no key)."""
    B, H, S, hd = q.shape
    keep = visible(B, S, causal, key_mask)
    o, e_o = torch.empty_like(q), torch.empty_like(q)
    lse, smax = torch.empty(B, H, S, dtype=torch.float64), torch.empty(B, H, S, dtype=torch.float64)
    dead = ~keep[:, 0].any(-1)
    for b in range(B):
        for h0, h1 in _heads(H, S):
            p, l_, m_, _ = _probs(q[b, h0:h1], k[b, h0:h1], keep[b], scale)
            o[b, h0:h1] = p @ v[b, h0:h1]
            e_o[b, h0:h1] = p @ v[b, h0:h1].abs()
            lse[b, h0:h1], smax[b, h0:h1] = l_, m_
    return dict(o=o, e_o=e_o, lse=lse, smax=smax, dead=dead)


def backward(q, k, v, o, dout, scale, causal, key_mask=None):
    """Explicit float64 backward from the O the kernel is handed (bf16-rounded): dq, dk, dv, their bounds e_dq, e_dk, e_dv, delta and e_delta.
    P is recomputed from q, k (not from a rounded LSE)."""
    B, H, S, hd = q.shape
    keep = visible(B, S, causal, key_mask)
    delta = (dout * o).sum(-1)
    e_delta = (dout.abs() * o.abs()).sum(-1)
    r = {n: torch.empty_like(q) for n in ("dq", "dk", "dv", "e_dq", "e_dk", "e_dv")}
    for b in range(B):
        for h0, h1 in _heads(H, S):
            sl = (b, slice(h0, h1))
            p, _, _, _ = _probs(q[sl], k[sl], keep[b], scale)
            do = dout[sl]
            dp = do @ v[sl].transpose(-1, -2)
            dl = delta[sl][..., None]
            ds = p * (dp - dl)
            es = p * (dp.abs() + dl.abs())
            r["dv"][sl] = p.transpose(-1, -2) @ do
            r["e_dv"][sl] = p.transpose(-1, -2) @ do.abs()
            r["dq"][sl] = scale * (ds @ k[sl])
            r["e_dq"][sl] = scale * (es @ k[sl].abs())
            r["dk"][sl] = scale * (ds.transpose(-1, -2) @ q[sl])
            r["e_dk"][sl] = scale * (es.transpose(-1, -2) @ q[sl].abs())
    r["delta"], r["e_delta"] = delta, e_delta
    return r


def rope_inverse(x, e, cos, sin):
    """The backward's RoPE epilogue in float64: x [B, H, S, hd] (a gradient w.r.t. the rotated q or k) rotated back with the half-split
    pairs (i, i + hd/2) of HF's rotate_half; the bound e rotated with |cos|, |sin|.  cos, sin fp32 [>= S, hd/2]."""
    S, half = x.shape[2], x.shape[3] // 2
    c, s = cos[:S].double(), sin[:S].double()
    a, b = x[..., :half], x[..., half:]
    ea, eb = e[..., :half], e[..., half:]
    xr = torch.cat([a * c + b * s, b * c - a * s], -1)
    er = torch.cat([ea * c.abs() + eb * s.abs(), eb * c.abs() + ea * s.abs()], -1)
    return xr, er


def decode(q, kc, vc, scale, T_len, key_mask=None, kv_row=None):
    """Single-query attention against a cache: q float64 [B, H, hd], kc / vc float64 [B_phys, H, Smax, hd]; key t of logical row b is read
    from physical row kv_row[b, t] (default b).  -> o, e_o [B, H, hd]; a row that sees no key gives O = 0."""
    B, H, hd = q.shape
    t = torch.arange(T_len)
    rows = torch.arange(B)[:, None].expand(B, T_len) if kv_row is None else kv_row[:, :T_len].long().cpu()
    K = kc[rows, :, t[None, :]]                       # [B, T, H, hd]
    V = vc[rows, :, t[None, :]]
    s = torch.einsum("bhd,bthd->bht", q, K) * scale
    keep = torch.ones(B, T_len, dtype=torch.bool) if key_mask is None else key_mask[:, :T_len].bool().cpu()
    s = s.masked_fill(~keep[:, None, :], float("-inf"))
    dead = ~keep.any(-1)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - torch.where(dead[:, None], torch.zeros_like(lse), lse)[..., None]).masked_fill(~keep[:, None, :], 0.0)
    return torch.einsum("bht,bthd->bhd", p, V), torch.einsum("bht,bthd->bhd", p, V.abs())


def ratio(got, ref, e, phi=PHI):
    """Worst (|got - ref| - phi * max(e)) / e over the tensor: <= TAU passes.  Elements with e == 0 must be exact (+inf otherwise)."""
    got, ref, e = got.double().cpu(), ref.double().cpu(), e.double().cpu()
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    slack = (err - phi * float(e.max()) if e.numel() else err).clamp_min(0.0)
    r = torch.where(e > 0, slack / e.clamp_min(1e-300), torch.where(slack > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    return float(r.max()) if r.numel() else 0.0


def within(got, ref, e, tau=TAU, phi=PHI):
    return ratio(got, ref, e, phi) <= tau


def lse_ratio(got, ref, smax):
    """Worst |got - ref| / (1 + max|s|) over the rows that see a key; rows that see none must be +inf exactly (inf otherwise)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    live = torch.isfinite(ref)
    if not bool((got[~live] == float("inf")).all()):
        return float("inf")
    if not bool(live.any()):
        return 0.0
    g = got[live]
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return float(((g - ref[live]).abs() / (1.0 + smax.double().cpu()[live])).max())


def global_ok(got, ref, tol):
    """The suite's older criterion: max |got - ref| <= tol * max |ref|."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max()) <= tol * (float(ref.abs().max()) + 1e-12)
