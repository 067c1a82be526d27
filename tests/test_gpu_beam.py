"""GPU: generate(num_beams > 1) — beam search and beam sampling on the device — against HF's own _beam_search
(tests/golden/beam_search.npz, recorded by tools/gen_beam_golden.py on the tiny model in fp32).

sequences and beam_indices exact, sequences_scores within 1e-4 absolute, scores within 1e-3 relative with HF's number of iterations.
Beam sampling: step-0 scores against HF's, and the step-0 choice against a Gumbel-top-K recomputed from oracle.sampling.gumbel_noise."""
import os
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import synth
from egoscaler_amd.config import dims_tiny

pytestmark = pytest.mark.gpu


def make_model(dims, seed=0):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.float32)
    m.load_state_dict(synth.synth_state_dict(dims, seed), strict=True)
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


def test_beam_search_matches_hf(setup):
    g, dims, pts, m = setup
    for c in g["cases"]:
        kw, lpad = _case_kw(g, c)
        o = _gen(m, g, pts, leftpad=lpad, **kw)
        assert np.array_equal(o.sequences.cpu().numpy(), g[f"{c}/sequences"]), c
        assert np.array_equal(o.beam_indices.cpu().numpy(), g[f"{c}/beam_indices"]), c
        assert float(np.abs(o.sequences_scores.cpu().numpy() - g[f"{c}/sequences_scores"]).max()) < 1e-4, c
        want = g[f"{c}/scores"]
        got = torch.stack(o.scores, 0).cpu().numpy()
        assert got.shape == want.shape, (c, got.shape, want.shape)
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)), c
        assert float(np.abs(got[fin] - want[fin]).max() / np.abs(want[fin]).max()) < 1e-3, c


def test_num_beams_one_is_todays_path(setup, golden_dir):
    g, dims, pts, m = setup
    # greedy with num_beams=1 still reproduces the reference's recorded greedy ids (tests/golden/tiny_model.npz, made before beam search existed)
    ref = np.load(os.path.join(golden_dir, "tiny_model.npz"), allow_pickle=False)
    ids, mask = torch.from_numpy(g["prompt_ids"]), torch.from_numpy(g["prompt_mask"]).bool()
    o = m.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), point_clouds=pts, max_length=10, do_sample=False, num_beams=1,
                   fps_start=g["fps_start"])
    assert np.array_equal(o.sequences.cpu().numpy(), ref["gen_sequences"])
    for kw in (dict(do_sample=False), dict(do_sample=True, seed=7)):
        a = _gen(m, g, pts, **kw)
        b = _gen(m, g, pts, num_beams=1, length_penalty=2.0, early_stopping=True, **kw)
        assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
        assert not hasattr(b, "sequences_scores")


def test_num_return_sequences_above_num_beams_raises(setup):
    g, dims, pts, m = setup
    with pytest.raises(ValueError, match="num_return_sequences"):
        _gen(m, g, pts, num_beams=2, num_return_sequences=3, do_sample=False)


def test_graph_equals_eager_and_replay(setup):
    g, dims, pts, m = setup
    kw, _ = _case_kw(g, "eos")
    for extra in (dict(), dict(do_sample=True, temperature=0.7, seed=3)):
        k = {**kw, **extra}
        a = _gen(m, g, pts, **k)
        b = _gen(m, g, pts, use_graph=False, **k)
        c = _gen(m, g, pts, **k)                       # the cached graph replayed
        for x in (b, c):
            assert torch.equal(a.sequences, x.sequences) and torch.equal(a.sequences_scores, x.sequences_scores)
            assert torch.equal(a.beam_indices, x.beam_indices) and len(a.scores) == len(x.scores)
            assert all(torch.equal(p, q) for p, q in zip(a.scores, x.scores))


def test_beam_sampling_step0(setup):
    from oracle import sampling as OS
    g, dims, pts, m = setup
    nb, T, k, p, rep = g["sample/args"].tolist()
    nb, k = int(nb), int(k)
    seed = 1234
    o = _gen(m, g, pts, num_beams=nb, do_sample=True, temperature=T, top_k=k, top_p=p, repetition_penalty=rep, eos_token_id=dims.tok.eos,
             seed=seed)
    s0 = o.scores[0].cpu()
    want = torch.from_numpy(g["sample/scores0"])
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(s0))
    assert float((s0[fin] - want[fin]).abs().max() / want[fin].abs().max()) < 1e-3
    # step-0 choice = Gumbel-top-K of the accumulated scores ([0, -1e9, ...] + scores) with the device's noise, draw counter 0
    R, V = s0.shape
    B, K = R // nb, 2 * nb
    run = torch.full((B, nb), -1e9)
    run[:, 0] = 0
    acc = s0.view(B, nb, V) + run[:, :, None]
    key = (acc + torch.from_numpy(OS.gumbel_noise(R, V, seed, 0)).view(B, nb, V)).view(B, nb * V)
    top = torch.topk(key, K, dim=1)[1]
    tok = top % V
    bi = o.beam_indices.cpu()
    S0 = g["prompt_ids"].shape[1]
    for b in range(B):
        # the top returned hypothesis' first token was one of the K draws, from a token inside the warped support
        t0 = int(o.sequences[b, S0])
        assert t0 in tok[b].tolist()
        assert bool(torch.isfinite(s0[int(bi[b, 0]), t0]))


def test_decoder_cache_follows_load_state_dict(setup, monkeypatch):
    g, dims, pts, _ = setup
    kw_beam, _ = _case_kw(g, "nb4")
    for kw in (dict(do_sample=False), kw_beam):
        m = make_model(dims, seed=0)
        _gen(m, g, pts, **kw)
        m.load_state_dict(synth.synth_state_dict(dims, 1), strict=True)
        a = _gen(m, g, pts, **kw)
        monkeypatch.setenv("EGOMI_DECODER_CACHE", "0")
        ref = make_model(dims, seed=1)
        b = _gen(ref, g, pts, **kw)
        monkeypatch.delenv("EGOMI_DECODER_CACHE")
        assert torch.equal(a.sequences, b.sequences)
        assert all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
