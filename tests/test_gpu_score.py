"""GPU: model.score() -- teacher-forced log-probs of GIVEN trajectories on a shared prompt (decode.Decoder.score: step 0 from the prefill
logits, ONE suffix pass with egomi_attn_suffix_shared for the rest, egomi_token_logprob per column), and the driver's --rescore.
  * tiny fp32 model.  Bound (a), the bound of tests/test_gpu_generate_logprobs.py: |got - ref| <= 2 * REL * max|logits| against the float64
    log_softmax of model.forward() on prompt + candidate (REL = 1e-3: the chosen logit and the log-sum-exp each move by at most the
    logits' error).  Held on generate()'s own samples (and against generate()'s own log-probs, lengths and rank), on random candidates
    that differ per candidate and per clip, at K = 1 and T = 1, under a row budget of one clip per pass, and with LoRA adapters.
  * the eos rule bit for bit; generate() undisturbed by score(); rejected inputs; the driver.
  * tiny bf16 model: score() of an int4 run's samples is the bf16 model's log-prob (bound: (a) with the project's bf16 logit bound MAX_TOL
    = 4e-2 in REL's place), not the int4 run's own.
  * 7B width (bf16, 2 layers, hd 128, 2 clips x K = 4, S0 = 540, T = 40): the suffix pass's logits against the shared decoder stepping on
    the same forced tokens, FRO_TOL / MAX_TOL.  Measured on an MI355X: see MEASURED_7B below."""
import json
import os
import types

import pytest
import torch

from tests.test_gpu_best_of_k import FRO_TOL, MAX_TOL, PLAIN, REL, SEED, _errs, _kw, _tiny_model, _tool
from tests.test_gpu_generate_logprobs import _forward_logprobs

pytestmark = pytest.mark.gpu
K, T = 4, 8
MEASURED_7B = "fro 5.1e-3, max 6.4e-3 (relative Frobenius / relative max over 8 rows x 39 positions x vocabulary)"


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _skw(toks, masks, Lp, pts):
    kw = _kw(toks, masks, Lp, pts, 0)
    del kw["max_length"]
    return kw


def _reference(m, toks, masks, Lp, pts, cand):
    """float64 teacher forcing on prompt + candidate: -> (log-probs [B*K, T], max|logits|)."""
    B, k, t = cand.shape
    seq = torch.cat([toks[:, :Lp].cuda().repeat_interleave(k, 0), cand.reshape(B * k, t).cuda()], 1)
    return _forward_logprobs(m, types.SimpleNamespace(sequences=seq), masks, Lp, pts, k, t)


def _draw(g, dims, shape, lo=0):
    """Token ids uniform over [lo, V) without the three point tokens: model.forward(), the reference, splices a cloud at a point-start
    token wherever it stands, while generate()'s steps and score() embed a suffix token as it is."""
    tok = dims.tok
    assert tok.point_start == tok.point_patch + 1 and tok.point_end == tok.point_patch + 2 and lo <= tok.point_patch
    c = torch.randint(lo, dims.lm.vocab_size - 3, shape, generator=g)
    return torch.where(c >= tok.point_patch, c + 3, c)


def _step_sum(lp):
    acc = torch.zeros(lp.shape[0], dtype=torch.float32, device=lp.device)
    for t in range(lp.shape[1]):
        acc = acc + lp[:, t]
    return acc


def test_score_of_generated_samples_matches_teacher_forcing_and_generate(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    gen = m.generate(**_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED, output_logprobs=True)
    cand = gen.sequences[:, Lp:].reshape(2, K, T)
    sc = m.score(**_skw(toks, masks, Lp, pts), candidates=cand, eos_token_id=None)
    assert sc.token_logprobs.shape == (2 * K, T) and sc.token_logprobs.dtype == torch.float32
    assert sc.sequences_logprobs.shape == (2 * K,) and sc.sequences_logprobs.dtype == torch.float32
    assert sc.sequences_lengths.shape == (2 * K,) and sc.sequences_lengths.dtype == torch.int32
    assert sc.sample_scores.shape == (2, K) and sc.sample_scores.dtype == torch.float32
    assert sc.rank.shape == (2, K) and sc.rank.dtype == torch.int32
    ref, mx = _reference(m, toks, masks, Lp, pts, cand)
    bound = 2 * REL * mx
    e_ref = float((sc.token_logprobs.double() - ref).abs().max())
    e_gen = float((sc.token_logprobs - gen.token_logprobs).abs().max())
    print(f"score tiny fp32: |score - float64| {e_ref:.3e}, |score - generate| {e_gen:.3e}, bound {bound:.3e} (max|logits| {mx:.3f})")
    assert e_ref <= bound and e_gen <= bound
    assert torch.equal(sc.sequences_lengths, gen.sequences_lengths)
    assert torch.equal(_step_sum(sc.token_logprobs), sc.sequences_logprobs)
    top = gen.sample_scores.sort(1, descending=True).values
    clear = (top[:, 0] - top[:, 1]) > 2 * bound
    assert torch.equal(sc.rank[clear, 0], gen.rank[clear, 0])


def test_random_candidates_each_read_their_own_suffix_and_prompt(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    g = torch.Generator().manual_seed(21)
    cand = torch.randint(0, dims.lm.vocab_size, (2, K, 9), generator=g)
    assert len({tuple(c.tolist()) for c in cand.reshape(-1, 9)}) == 2 * K
    sc = m.score(**_skw(toks, masks, Lp, pts), candidates=cand.cuda(), eos_token_id=None)
    ref, mx = _reference(m, toks, masks, Lp, pts, cand)
    err = float((sc.token_logprobs.double() - ref).abs().max())
    print(f"score tiny fp32, random candidates: |score - float64| {err:.3e}, bound {2 * REL * mx:.3e}")
    assert err <= 2 * REL * mx
    assert bool((sc.sequences_lengths == 9).all())


def test_eos_rule(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    Tc, eos = 9, 5
    g = torch.Generator().manual_seed(22)
    cand = _draw(g, dims, (2, K, Tc), lo=6)                            # no eos anywhere ...
    cand[0, 0, 0] = eos                                                # ... then at 0, in the middle (and again later), last, nowhere
    cand[0, 1, 4] = eos
    cand[0, 1, 6] = eos
    cand[0, 2, Tc - 1] = eos
    cand[1, 1, 3:] = eos                                               # the shape of a finished row with pad == eos
    want = torch.tensor([1, 5, Tc, Tc, Tc, 4, Tc, Tc], dtype=torch.int32)
    kw = _skw(toks, masks, Lp, pts)
    sc = m.score(**kw, candidates=cand.cuda(), eos_token_id=eos)
    assert torch.equal(sc.sequences_lengths.cpu(), want)
    after = torch.arange(Tc)[None, :] >= want[:, None]
    assert bool((sc.token_logprobs.cpu()[after] == 0).all()) and bool((sc.token_logprobs.cpu()[~after] < 0).all())
    assert torch.equal(_step_sum(sc.token_logprobs), sc.sequences_logprobs)
    other = cand.clone().reshape(2 * K, Tc)
    other[after] = _draw(g, dims, (int(after.sum()),))                 # whatever follows an eos is ignored
    sc2 = m.score(**kw, candidates=other.reshape(2, K, Tc).cuda(), eos_token_id=eos)
    for f in ("token_logprobs", "sequences_logprobs", "sequences_lengths", "sample_scores", "rank"):
        assert torch.equal(getattr(sc, f), getattr(sc2, f)), f
    ref, mx = _reference(m, toks, masks, Lp, pts, cand)
    assert float(((sc.token_logprobs.double() - ref).abs() * (~after).cuda()).max()) <= 2 * REL * mx
    free = m.score(**kw, candidates=cand.cuda(), eos_token_id=None)    # None counts all
    assert bool((free.sequences_lengths == Tc).all()) and bool((free.token_logprobs < 0).all())
    assert float((free.token_logprobs.double() - ref).abs().max()) <= 2 * REL * mx


def test_one_candidate_and_one_token(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    g = torch.Generator().manual_seed(23)
    kw = _skw(toks, masks, Lp, pts)
    for k, t in ((1, 9), (K, 1), (1, 1)):
        cand = _draw(g, dims, (2, k, t))
        sc = m.score(**kw, candidates=cand.cuda(), eos_token_id=None)
        ref, mx = _reference(m, toks, masks, Lp, pts, cand)
        assert sc.token_logprobs.shape == (2 * k, t) and sc.rank.shape == (2, k)
        assert float((sc.token_logprobs.double() - ref).abs().max()) <= 2 * REL * mx, (k, t)
        if k == 1:
            assert bool((sc.rank == 0).all())
    from egoscaler_amd.decode import DenseCache, Decoder
    assert isinstance(Decoder(m.engine, 2, Lp + 4, samples_per_prompt=1, max_new_tokens=4).cache, DenseCache)     # still the dense decoder


def test_row_budget_of_one_clip_per_pass(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    g = torch.Generator().manual_seed(24)
    cand = _draw(g, dims, (2, K, 9)).cuda()
    kw = _skw(toks, masks, Lp, pts)
    one = m.score(**kw, candidates=cand, eos_token_id=None)
    two = m.score(**kw, candidates=cand, eos_token_id=None, row_budget=K * 8)
    ref, mx = _reference(m, toks, masks, Lp, pts, cand.cpu())
    assert float((two.token_logprobs - one.token_logprobs).abs().max()) <= 2 * REL * mx
    assert float((two.token_logprobs.double() - ref).abs().max()) <= 2 * REL * mx
    assert torch.equal(one.sequences_lengths, two.sequences_lengths)


def test_lora_adapters_on_all_seven_targets():
    from egoscaler_amd import lora
    m, dims, toks, masks, Lp, pts = _tiny_model(lora_r=8, lora_alpha=16.0, lora_target_modules=",".join(lora.TARGETS))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B.weight"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    m.load_state_dict(m.state_dict())
    cand = _draw(g, dims, (2, K, 9))
    sc = m.score(**_skw(toks, masks, Lp, pts), candidates=cand.cuda(), eos_token_id=None)
    ref, mx = _reference(m, toks, masks, Lp, pts, cand)
    err = float((sc.token_logprobs.double() - ref).abs().max())
    print(f"score tiny fp32 + LoRA: |score - float64| {err:.3e}, bound {2 * REL * mx:.3e}")
    assert err <= 2 * REL * mx


def test_bf16_score_of_an_int4_run_is_the_bf16_models():
    """No generate() call forces given tokens, so the reference is the float64 log_softmax of the bf16 model.forward().  Bound: (a) with
    MAX_TOL in REL's place -- MAX_TOL = 4e-2 is the project's bound on the relative max error of bf16 logits, and the chosen logit and the
    log-sum-exp each move by at most the logits' error."""
    m, dims, toks, masks, Lp, pts = _tiny_model(torch.bfloat16)
    gen = m.generate(**_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED, output_logprobs=True,
                     decode_weight_dtype="int4")
    cand = gen.sequences[:, Lp:].reshape(2, K, T)
    sc = m.score(**_skw(toks, masks, Lp, pts), candidates=cand, eos_token_id=None)
    ref, mx = _reference(m, toks, masks, Lp, pts, cand)
    bound = 2 * MAX_TOL * mx
    err = float((sc.token_logprobs.double() - ref).abs().max())
    off = float((gen.token_logprobs.double() - ref).abs().max())
    print(f"score tiny bf16 on an int4 run's samples: |score - float64| {err:.3e}, |int4 run - float64| {off:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert not torch.equal(sc.token_logprobs[:, 1:], gen.token_logprobs[:, 1:])     # the int4 steps' log-probs are another model's
    assert float((sc.token_logprobs[:, 0] - gen.token_logprobs[:, 0]).abs().max()) <= bound       # step 0: both from the bf16 prefill


def test_generate_is_undisturbed_by_score(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED, output_logprobs=True)
    a = m.generate(**kw)
    held = dict(m._decoders)
    m.score(**_skw(toks, masks, Lp, pts), candidates=a.sequences[:, Lp:].reshape(2, K, T), eos_token_id=None)
    assert list(m._decoders) == list(held) and all(m._decoders[k] is v for k, v in held.items())
    b = m.generate(**kw)
    assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    assert torch.equal(a.token_logprobs, b.token_logprobs) and torch.equal(a.sequences_logprobs, b.sequences_logprobs)
    assert torch.equal(a.rank, b.rank)


def test_rejected_inputs(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = _skw(toks, masks, Lp, pts)
    ok = torch.zeros(2, K, T, dtype=torch.int64, device="cuda")
    for bad in (torch.zeros(2, 33, T, dtype=torch.int64, device="cuda"), torch.zeros(2, K, 0, dtype=torch.int64, device="cuda"),
                ok[0], ok.int(), torch.zeros(3, K, T, dtype=torch.int64, device="cuda"),
                torch.zeros(2, 1, dims.lm.max_position_embeddings - Lp + 1, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            m.score(**kw, candidates=bad)
    with pytest.raises(NotImplementedError):
        m.score(**{**kw, "point_clouds": [p for p in pts.cuda()]}, candidates=ok)


def test_driver_rescore(tmp_path, capsys, monkeypatch):
    from egoscaler_amd import driver
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    seen = []
    score = TrajPointLLMForCausalLM.score

    def spy(self, *a, **k):
        out = score(self, *a, **k)
        seen.append(out.rank[:, 0].tolist())
        return out
    monkeypatch.setattr(TrajPointLLMForCausalLM, "score", spy)
    torch.manual_seed(3)
    driver.main(["eval", "--tiny", "--num_samples", "4", "--select", "logprob", "--rescore", "--dtype", "fp32", "--bs", "2", "--n_val", "4",
                 "--num_steps", "5", "--max_traj_token", "48", "--out_dir", str(tmp_path)])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    dump = json.load(open(os.path.join(tmp_path, "test_gen_trajs.json")))
    assert len(seen) == 2 and {"ADE_sel", "FDE_sel", "n_sel"} <= set(rec) and rec["select"] == "logprob"
    sel = dump.pop("selected")
    assert len(dump) == 4 and set(sel) == set(dump)
    assert sorted(sel.values()) == sorted(j for batch in seen for j in batch)      # the picks are score()'s


@torch.no_grad()
def test_suffix_pass_logits_at_7b_width():
    """7B width, 2 layers, bf16, hd 128 (MFMA form), 2 clips x K = 4, S0 = 540, T = 40: the logits of ONE suffix pass against the shared
    decoder stepping 39 times on the same forced tokens (every row its own)."""
    from egoscaler_amd import synth
    from egoscaler_amd.decode import Decoder
    m, dims = _tool().model_7b(layers=2)
    B, k, t = 2, 4, 40
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    ids, mask = toks[:, :Lp].cuda(), masks[:, :Lp].cuda()
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    assert Lp == 540
    cand = torch.randint(0, 4000, (B * k, t), generator=torch.Generator().manual_seed(0)).cuda()
    ds = Decoder(m.engine, B * k, Lp + t, samples_per_prompt=k, max_new_tokens=t)
    dq = Decoder(m.engine, B * k, Lp + t, samples_per_prompt=k, max_new_tokens=t, score_cache=True)
    ds.prefill(ids, mask, pcs, st, t)
    dq.prefill(ids, mask, pcs, st, t)
    got =dq.score(cand, None, keep_logits=True)
    assert got.shape == (B * k, t - 1, dims.lm.vocab_size)
    ref = torch.empty_like(got)
    for s in range(t - 1):
        ds.tok.copy_(cand[:, s:s + 1])
        ds.step(Lp + s)
        ref[:, s] = ds.lg
    fro, mx = _errs(got, ref)
    print(f"score 7B width (2 layers, {B} x {k} rows, S0 {Lp}, T {t}): suffix pass vs stepped logits fro {fro:.2e} max {mx:.2e}")
    assert fro <= FRO_TOL and mx <= MAX_TOL, (fro, mx)
    lg = got.float().view(B, k, t - 1, -1)
    assert float((lg[:, 0] - lg[:, 1]).abs().max()) > 0               # the candidates of a clip do see their own suffix
