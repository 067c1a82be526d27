"""GPU: beam search in the production dtype (bf16) at LLaMA-7B width, the chunked-prefill beam path, and `driver eval --num_beams`.

At 7B width in bf16 the decisions cannot be pinned to HF (two candidates are often closer than bf16 noise), so the properties are:
two runs bit-equal, graph == eager, permuting the batch permutes the result, and every sequences_scores equals the sum of its chosen
per-step scores (followed through beam_indices) divided by len ** length_penalty.  L = 2 layers, B = 8 clips, 4 beams, the 540-token
prompt of tools/bench_beam.py; then one full 32-layer B = 8 x 4 run that must complete."""
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


def _bench():
    spec = importlib.util.spec_from_file_location("bench_beam", os.path.join(ROOT, "tools", "bench_beam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _inputs(dims, B):
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=16, num_steps=20, max_traj_token=160)
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    return toks[:, :Lp].cuda(), masks[:, :Lp].cuda(), pcs, np.arange(B) * 7


def _gen(m, ids, mask, pcs, st, T, **kw):
    return m.generate(input_ids=ids, attention_mask=mask, point_clouds=pcs, fps_start=st, max_length=T, num_beams=4, num_return_sequences=2,
                      eos_token_id=None, **kw)


def _same(a, b):
    return (torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores) and torch.equal(a.beam_indices, b.beam_indices)
            and len(a.scores) == len(b.scores) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores)))


@pytest.fixture(scope="module")
def model_l2():
    m, dims = _bench().model_7b(layers=2)
    yield m, dims
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("do_sample", [False, True])
def test_7b_width_bf16_beam_properties(model_l2, do_sample):
    m, dims = model_l2
    B, T, lp = 8, 12, 1.5
    ids, mask, pcs, st = _inputs(dims, B)
    assert ids.shape[1] == 540
    kw = dict(do_sample=do_sample, seed=5, length_penalty=lp, temperature=0.8)
    a = _gen(m, ids, mask, pcs, st, T, **kw)
    b = _gen(m, ids, mask, pcs, st, T, **kw)
    e = _gen(m, ids, mask, pcs, st, T, use_graph=False, **kw)
    assert _same(a, b) and _same(a, e)
    assert a.sequences.shape == (2 * B, 540 + T) and a.beam_indices.dtype == torch.int64 and len(a.scores) == T
    # sequences_scores = sum of the chosen per-step scores / len ** length_penalty
    sc = torch.stack(a.scores, 0).cpu()
    bi, seq = a.beam_indices.cpu(), a.sequences.cpu()
    for h in range(2 * B):
        n = int((bi[h] >= 0).sum())
        tot = torch.zeros((), dtype=torch.float32)
        for t in range(n):
            tot = tot + sc[t, int(bi[h, t]), int(seq[h, 540 + t])]
        want = float(tot) / n ** lp
        assert abs(float(a.sequences_scores[h]) - want) <= 1e-5 * max(1.0, abs(want)), (h, float(a.sequences_scores[h]), want)
    if not do_sample:
        # permuting the clips permutes the hypotheses (greedy beam search: no per-row random stream to follow the permutation).  Ids and
        # beam indices must follow exactly; the scores only within bf16 noise: the bf16 prompt pass does not give a clip bit-identical
        # logits at another batch position (a property of the engine's prefill, not of the per-item beam kernels)
        perm = torch.tensor([3, 0, 7, 5, 1, 6, 2, 4])
        p = _gen(m, ids[perm.cuda()], mask[perm.cuda()], pcs[perm.cuda()], st[perm.numpy()], T, **kw)
        rows = (perm[:, None] * 2 + torch.arange(2)[None]).reshape(-1).cuda()
        shift = ((torch.arange(B) - perm) * 4).repeat_interleave(2)[:, None].cuda()
        assert torch.equal(p.sequences, a.sequences[rows])
        assert torch.equal(p.beam_indices, a.beam_indices[rows] + shift)
        assert float((p.sequences_scores - a.sequences_scores[rows]).abs().max()) < 5e-3


def test_chunked_prefill_beam_equals_per_clip_runs():
    """B > 16 prompts go through prefill_chunked(nb=...): each item's result equals a run of that item in a small batch."""
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dims = dims_tiny()
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.float32)
    m.load_state_dict(synth.synth_state_dict(dims, 0), strict=True)
    m.eval()
    B = 18
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=8, num_steps=4, max_traj_token=40)
    pcs = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    st = np.arange(B) * 3
    kw = dict(max_length=6, num_beams=3, num_return_sequences=3, do_sample=False, eos_token_id=None)
    big = m.generate(input_ids=toks[:, :Lp].cuda(), attention_mask=masks[:, :Lp].cuda(), point_clouds=pcs, fps_start=st, **kw)
    for b0 in (0, 16):
        small = m.generate(input_ids=toks[b0:b0 + 2, :Lp].cuda(), attention_mask=masks[b0:b0 + 2, :Lp].cuda(), point_clouds=pcs[b0:b0 + 2],
                           fps_start=st[b0:b0 + 2], **kw)
        r = slice(3 * b0, 3 * b0 + 6)
        assert torch.equal(big.sequences[r], small.sequences)
        assert float((big.sequences_scores[r] - small.sequences_scores).abs().max()) < 1e-4
        assert torch.equal(big.beam_indices[r] - 3 * b0, small.beam_indices)


def test_driver_eval_num_beams(tmp_path):
    """`driver eval --num_beams N`: beam search per batch, one (the best) trajectory per image id in the dump."""
    from egoscaler_amd.driver import SyntheticTrajData, evaluate
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    import json
    dims = dims_tiny(vocab=320, num_bins=64)
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=64, model_name=None, max_traj_token=48,
                                 num_steps=5, bs=4, checkpoint_dir=str(tmp_path), val_sample=False, num_beams=3)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.float32)
    m.load_state_dict(synth.synth_state_dict(dims, 0))
    seen = []
    gen = m.generate

    def spy(*a, **k):
        out = gen(*a, **k)
        seen.append((k.get("num_beams", 1), out.sequences.shape[0], k["input_ids"].shape[0], hasattr(out, "sequences_scores")))
        return out
    m.generate = spy
    data = SyntheticTrajData(dims, 6, frames=2, size=32, text_len=8, num_steps=5, seed=977)
    metrics = evaluate(args, m, data, split="test")
    assert seen and all(x == (3, x[2], x[2], True) for x in seen)                  # beams asked for, one hypothesis back per clip
    assert sum(x[2] for x in seen) == len(data)
    dump = json.load(open(os.path.join(tmp_path, "test_gen_trajs.json")))
    assert len(dump) == metrics["n"] <= len(data)


def test_full_32_layer_beam_completes():
    """One full-size run: 7B, 32 layers, 8 clips x 4 beams, 540-token prompts, 24 new tokens, under the hipGraph."""
    m, dims = _bench().model_7b()
    ids, mask, pcs, st = _inputs(dims, 8)
    o = _gen(m, ids, mask, pcs, st, 24, do_sample=False)
    assert o.sequences.shape == (16, 540 + 24) and len(o.scores) == 24
    assert bool(torch.isfinite(o.sequences_scores).all()) and int(o.beam_indices.min()) >= 0
