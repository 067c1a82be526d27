"""GPU: beam search on the split KV cache, generate(num_beams=N, kv_cache_layout="split"): one prompt cache row per clip, one suffix row
per beam, egomi_attn_decode_shared_rows through the beam row table in every step (decode.Decoder(split_cache=True)).
  * tiny fp32 model: every case of tests/golden/beam_search.npz under the criteria of tests/test_gpu_beam.py (sequences and beam_indices
    exact, sequences_scores within 1e-4, scores within 1e-3 relative with HF's iteration count); beam sampling against the dense layout
    under the same seed; graph replay equals eager bit for bit; a left-padded prompt; the cache's tensors and size; the rejected
    combinations; LoRA adapters and fp8 decode weights reach the split steps.
  * 7B width (bf16, 2 layers, hd 128, 8 clips x 4 beams, S0 = 540): a dense and a split Decoder step eagerly on the same forced tokens and
    the same forced random parents for 16 steps, inside the bounds of tests/test_gpu_best_of_k.py (FRO_TOL, MAX_TOL).
    Measured on an MI355X: see MEASURED_7B below."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import synth
from egoscaler_amd.config import dims_tiny

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-3                                   # tests/test_gpu_beam.py (scores)
FRO_TOL, MAX_TOL = 2.5e-2, 4e-2              # tests/test_gpu_best_of_k.py (two bf16 paths that sum in another order)
SPLIT = dict(kv_cache_layout="split")
MEASURED_7B = "fro 6.9e-3, max 8.3e-3 (relative Frobenius / relative max over all 32 rows x vocabulary, worst of the 16 steps)"


def _errs(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30)), float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _rel_finite(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(got))
    return float((got[fin] - want[fin]).abs().max() / want[fin].abs().max())


def make_model(dims, dtype=torch.float32, seed=0, **extra):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None, **extra)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, seed)
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}, strict=not extra)
    return m.eval()


@pytest.fixture(scope="module")
def setup(golden_dir):
    g = np.load(os.path.join(golden_dir, "beam_search.npz"), allow_pickle=False)
    dims = dims_tiny()
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(2)]).cuda()
    return g, dims, pts, make_model(dims)


def _gen(m, g, pts, leftpad=False, **kw):
    ids, mask = torch.from_numpy(g["prompt_ids"]).clone(), torch.from_numpy(g["prompt_mask"]).bool().clone()
    if leftpad:
        mask[1, :2] = False
        ids[1, :2] = m.dims.tok.pad
    return m.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), point_clouds=pts, max_length=int(g["t_new"]),
                      fps_start=g["fps_start"], **kw)


def _case_kw(g, c):
    nb, nrs, lp, es, rep, eos, lpad = g[f"{c}/args"].tolist()
    return dict(num_beams=int(nb), num_return_sequences=int(nrs), length_penalty=lp, early_stopping={0: False, 1: True, 2: "never"}[int(es)],
                repetition_penalty=rep, eos_token_id=int(eos), do_sample=False), bool(lpad)


def _last_decoder(m):
    """The decoder the model made last (a call that reuses a cached decoder does not move it: see _fresh)."""
    return list(m._decoders.values())[-1]


def _fresh(m):
    """Drop the model's cached decoders, so that the next generate() makes its own and _last_decoder finds it."""
    m.__dict__.pop("_decoders", None)


def test_split_beam_search_matches_hf(setup):
    g, dims, pts, m = setup
    assert len(g["cases"]) > 0
    for c in g["cases"]:
        kw, lpad = _case_kw(g, c)
        _fresh(m)
        o = _gen(m, g, pts, leftpad=lpad, **kw, **SPLIT)
        dec = _last_decoder(m)
        assert dec.kc is None and dec.split and dec.nb == kw["num_beams"], c       # the split decoder is what ran
        assert np.array_equal(o.sequences.cpu().numpy(), g[f"{c}/sequences"]), c
        assert np.array_equal(o.beam_indices.cpu().numpy(), g[f"{c}/beam_indices"]), c
        assert float(np.abs(o.sequences_scores.cpu().numpy() - g[f"{c}/sequences_scores"]).max()) < 1e-4, c
        want = g[f"{c}/scores"]
        got = torch.stack(o.scores, 0).cpu().numpy()
        assert got.shape == want.shape, (c, got.shape, want.shape)
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)), c
        assert float(np.abs(got[fin] - want[fin]).max() / np.abs(want[fin]).max()) < REL, c


def test_split_beam_sampling_follows_the_dense_layout(setup):
    g, dims, pts, m = setup
    nb, T, k, p, rep = g["sample/args"].tolist()
    kw = dict(num_beams=int(nb), do_sample=True, temperature=T, top_k=int(k), top_p=p, repetition_penalty=rep, eos_token_id=None, seed=1234)
    _fresh(m)
    dense = _gen(m, g, pts, **kw)
    split = _gen(m, g, pts, **kw, **SPLIT)
    assert _last_decoder(m).kc is None
    assert split.sequences.shape == dense.sequences.shape and split.beam_indices.shape == dense.beam_indices.shape
    same = float((split.sequences == dense.sequences).float().mean())
    r0 = _rel_finite(split.scores[0], dense.scores[0])
    print(f"split beam sampling: {same:.3f} of the tokens equal the dense layout's, step-0 scores rel {r0:.2e}")
    assert same > 0.9
    assert r0 < REL


def test_split_graph_equals_eager_and_replay(setup):
    g, dims, pts, m = setup
    kw, _ = _case_kw(g, "eos")
    for extra in (dict(), dict(do_sample=True, temperature=0.7, seed=3)):
        k = {**kw, **extra, **SPLIT}
        a = _gen(m, g, pts, **k)
        b = _gen(m, g, pts, use_graph=False, **k)
        c = _gen(m, g, pts, **k)                       # the cached graph replayed
        for x in (b, c):
            assert torch.equal(a.sequences, x.sequences) and torch.equal(a.sequences_scores, x.sequences_scores)
            assert torch.equal(a.beam_indices, x.beam_indices) and len(a.scores) == len(x.scores)
            assert all(torch.equal(p, q) for p, q in zip(a.scores, x.scores))


def test_split_left_padded_prompt(setup):
    g, dims, pts, m = setup
    kw, _ = _case_kw(g, "nb4")
    dense = _gen(m, g, pts, leftpad=True, **kw)
    split = _gen(m, g, pts, leftpad=True, **kw, **SPLIT)
    unpadded = _gen(m, g, pts, **kw, **SPLIT)
    assert torch.equal(split.sequences, dense.sequences) and torch.equal(split.beam_indices, dense.beam_indices)
    assert float((split.sequences_scores - dense.sequences_scores).abs().max()) < 1e-4
    assert len(split.scores) == len(dense.scores)
    assert max(_rel_finite(a, b) for a, b in zip(split.scores, dense.scores)) < REL
    assert not torch.equal(split.scores[1], unpadded.scores[1])       # the padding mask is what the split steps saw


def test_split_cache_tensors_and_size(setup):
    g, dims, pts, m = setup
    kw, _ = _case_kw(g, "nb4")
    nb, T = kw["num_beams"], int(g["t_new"])
    B, S0 = g["prompt_ids"].shape
    _fresh(m)
    _gen(m, g, pts, **kw, **SPLIT)
    dec = _last_decoder(m)
    lm = dims.lm
    L, H, hd = lm.num_hidden_layers, lm.num_attention_heads, lm.head_dim
    assert dec.kc is None and dec.vc is None
    assert dec.kp.shape == dec.vp.shape == (L, B, H, S0, hd)
    assert dec.ksfx.shape == dec.vsfx.shape == (L, B * nb, H, T, hd)
    assert sum(t.numel() for t in (dec.kp, dec.vp, dec.ksfx, dec.vsfx)) == 2 * L * H * hd * (B * S0 + B * nb * T)
    assert dec.fused["qkv"] == 0
    _gen(m, g, pts, **kw)                                             # the dense decoder is another cache entry, and what it was
    dd = _last_decoder(m)
    assert dd is not dec and dd.kc.shape == (L, B * nb, H, S0 + T, hd) and not dd.split
    _gen(m, g, pts, **kw, kv_cache_layout="dense")                    # the default by its name: the same entry
    assert _last_decoder(m) is dd and len(m._decoders) == 2


def test_split_rejected_combinations(setup):
    g, dims, pts, m = setup
    kw = dict(do_sample=False, eos_token_id=None)
    with pytest.raises(ValueError, match="share_prompt"):
        _gen(m, g, pts, **kw, **SPLIT)
    with pytest.raises(ValueError, match="share_prompt"):
        _gen(m, g, pts, **kw, num_beams=1, num_return_sequences=2, **SPLIT)
    with pytest.raises(NotImplementedError):
        _gen(m, g, pts, **kw, num_beams=2, kv_cache_dtype="fp8", **SPLIT)
    with pytest.raises(NotImplementedError):
        _gen(m, g, [p for p in pts], **kw, num_beams=2, **SPLIT)
    with pytest.raises(ValueError, match="kv_cache_layout"):
        _gen(m, g, pts, **kw, num_beams=2, kv_cache_layout="paged")
    with pytest.raises(NotImplementedError, match="kv_cache_layout"):
        _gen(m, g, pts, **kw, num_beams=2, share_prompt=True)
    from egoscaler_amd.decode import Decoder
    S0, T = g["prompt_ids"].shape[1], int(g["t_new"])
    with pytest.raises(ValueError):
        Decoder(m.engine, 8, S0 + T, split_cache=True, max_new_tokens=T)                 # no beams
    with pytest.raises(ValueError):
        Decoder(m.engine, 8, S0 + T, num_beams=4, split_cache=True)                      # no suffix length
    with pytest.raises(ValueError):
        Decoder(m.engine, 6, S0 + T, num_beams=4, split_cache=True, max_new_tokens=T)
    with pytest.raises(NotImplementedError):
        Decoder(m.engine, 8, S0 + T, num_beams=4, split_cache=True, max_new_tokens=T, kv_dtype="fp8")


def test_lora_adapters_reach_the_split_steps(setup):
    from egoscaler_amd import lora
    g, dims, pts, plain = setup
    m = make_model(dims, lora_r=8, lora_alpha=16.0, lora_target_modules=",".join(lora.TARGETS))
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B.weight"):
                p.copy_(0.05 * torch.randn(p.shape, generator=gen))
            elif n.endswith("lora_A.weight"):
                p.mul_(4.0)
    m.load_state_dict(m.state_dict())
    kw, _ = _case_kw(g, "nb4")
    kw = dict(kw, eos_token_id=None)
    dense = _gen(m, g, pts, **kw)
    split = _gen(m, g, pts, **kw, **SPLIT)
    assert _last_decoder(m).kc is None and _last_decoder(m).wo is not None
    without = _gen(plain, g, pts, **kw, **SPLIT)
    assert torch.equal(split.sequences, dense.sequences) and torch.equal(split.beam_indices, dense.beam_indices)
    assert float((split.sequences_scores - dense.sequences_scores).abs().max()) < 1e-4
    assert max(_rel_finite(a, b) for a, b in zip(split.scores, dense.scores)) < REL
    assert len(without.scores) == len(split.scores) and _errs(split.scores[1], without.scores[1])[1] > REL


def test_fp8_decode_weights_reach_the_split_steps(setup):
    """bf16 tiny model, decode_weight_dtype='fp8': step 0 is the prefill (the same code in both layouts, so both start step 1 from the
    same beams); step 1's scores of the split layout sit inside the bf16 tolerances of the dense fp8 run, and differ from the split run on
    the bf16 weights."""
    g, dims, pts, _ = setup
    m = make_model(dims, torch.bfloat16)
    kw, _ = _case_kw(g, "nb4")
    kw = dict(kw, eos_token_id=None, decode_weight_dtype="fp8")
    dense = _gen(m, g, pts, **kw)
    split = _gen(m, g, pts, **kw, **SPLIT)
    dec = _last_decoder(m)
    assert dec.kc is None and dec.w8 is not None
    bf = _gen(m, g, pts, **{**kw, "decode_weight_dtype": None}, **SPLIT)
    assert torch.equal(split.scores[0], dense.scores[0])
    fro, mx = _errs(split.scores[1], dense.scores[1])
    print(f"split beams, fp8 decode weights: step-1 scores against the dense layout fro {fro:.2e} max {mx:.2e}")
    assert fro < FRO_TOL and mx < MAX_TOL, (fro, mx)
    assert not torch.equal(bf.scores[1], split.scores[1])


def _tool():
    spec = importlib.util.spec_from_file_location("bench_beam", os.path.join(ROOT, "tools", "bench_beam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@torch.no_grad()
def test_forced_beam_steps_at_7b_width():
    """7B width, 2 layers, bf16, hd 128, 8 clips x 4 beams, S0 = 540 (the MFMA prompt phase and the sliced suffix of
    egomi_attn_decode_shared_rows against egomi_attn_decode_rows on the dense cache): both decoders step eagerly on the same forced tokens
    and the same forced random parents (kv_row gathered by parent, then kv_row[r, cur_len] = r, as egomi_beam_update does) for 16 steps.
    Measured on an MI355X (worst over the 16 steps): see MEASURED_7B; bounds FRO_TOL 2.5e-2, MAX_TOL 4e-2."""
    from egoscaler_amd.decode import Decoder
    m, dims = _tool().model_7b(layers=2)
    B, nb, steps = 8, 4, 16
    R = B * nb
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    assert Lp == 540
    dd = Decoder(m.engine, R, Lp + steps, num_beams=nb)
    ds = Decoder(m.engine, R, Lp + steps, num_beams=nb, split_cache=True, max_new_tokens=steps)
    dd.prefill(ids, mask, pcs, st, steps, nb=nb)
    ds.prefill(ids, mask, pcs, st, steps, nb=nb)
    lm = dims.lm
    assert ds.kc is None and ds.kp.shape == (2, B, lm.num_attention_heads, Lp, lm.head_dim)
    assert ds.ksfx.shape == (2, R, lm.num_attention_heads, steps, lm.head_dim)
    assert ds.fused["qkv"] == 0 and ds.fused["o"] == dd.fused["o"] and ds.fused["down"] == dd.fused["down"]
    assert torch.equal(ds.lg[:B], dd.lg[:B])                          # the prefill is the same code
    own = torch.arange(R, dtype=torch.int32)
    kv_row = torch.zeros(R, Lp + steps, dtype=torch.int32)
    kv_row[:, :Lp] = (own // nb)[:, None]                             # every beam reads its item's prompt row (Decoder.beam)
    g = torch.Generator().manual_seed(0)
    worst = [0.0, 0.0]
    for t in range(steps):
        parent = (own // nb) * nb + torch.randint(0, nb, (R,), generator=g, dtype=torch.int32)
        kv_row = kv_row[parent.long()]
        kv_row[:, Lp + t] = own
        tok = torch.randint(0, 4000, (R, 1), generator=g).cuda()
        for d in (dd, ds):
            d.kv_row.copy_(kv_row)
            d.tok.copy_(tok)
            d.step(Lp + t)
        fro, mx = _errs(ds.lg, dd.lg)
        print(f"split beams 7B width step {t}: split vs dense logits fro {fro:.2e} max {mx:.2e}")
        assert fro < FRO_TOL and mx < MAX_TOL, (t, fro, mx)
        worst = [max(worst[0], fro), max(worst[1], mx)]
    lg = ds.lg.float().view(B, nb, -1)
    assert float((lg[:, 0] - lg[:, 1]).abs().max()) > 0               # the beams of a clip do see their own paths
    print(f"split beams 7B width (2 layers, 8 x 4 beams, S0 {Lp}, {steps} steps): split vs dense logits fro {worst[0]:.2e} max {worst[1]:.2e}")
