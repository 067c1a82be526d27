"""GPU: generate(kv_cache_dtype="fp8") — the e4m3fn KV cache (csrc/kv8.hip) under every generation mode.  The captured loop equals the eager
one bit for bit, step 0 (prefill logits, which never read the cache) equals the bf16 cache's, the decoder's cache is 8-bit, a bf16 and an
fp8 decoder of one geometry never stand in for each other, the teacher-forced logit error at 7B width is small but not zero, a full-size
graph replays deterministically and per row, and `driver eval --kv_cache_dtype fp8` runs."""
import importlib.util
import os
import types

import pytest
import torch

from egoscaler_amd import synth
from egoscaler_amd.config import dims_tiny

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {"greedy": dict(do_sample=False), "sample": dict(do_sample=True, seed=11, top_k=20, top_p=0.9, temperature=0.8),
         "beam": dict(num_beams=4, num_return_sequences=2, do_sample=False)}


def _model(dims, dtype):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, 0)
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()})
    return m.eval()


def _tool():
    spec = importlib.util.spec_from_file_location("bench_decode_kv8", os.path.join(ROOT, "tools", "bench_decode_kv8.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kw(dims, B=2, T=6):
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)]).cuda()
    pm = masks[:, :Lp].clone()
    pm[0, 2:4] = False
    return dict(input_ids=toks[:, :Lp].cuda(), attention_mask=pm.cuda(), point_clouds=pts, max_length=T, fps_start=[0, 17][:B], eos_token_id=None)


def _same(a, b):
    ok = torch.equal(a.sequences, b.sequences) and len(a.scores) == len(b.scores) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    if hasattr(a, "sequences_scores"):
        ok = ok and torch.equal(a.sequences_scores, b.sequences_scores) and torch.equal(a.beam_indices, b.beam_indices)
    return ok


def _decoder(m, kv):
    decs = [d for d in m._decoders.values() if d.kv_dtype == kv]
    assert len(decs) == 1
    return decs[0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_fp8_graph_equals_eager_step0_equals_bf16(dtype, mode):
    dims = dims_tiny()
    m = _model(dims, dtype)
    kw = {**_kw(dims), **MODES[mode]}
    g8 = m.generate(**kw, kv_cache_dtype="fp8")
    e8 = m.generate(**kw, kv_cache_dtype="fp8", use_graph=False)
    assert _same(g8, e8)
    ref = m.generate(**kw, kv_cache_dtype="auto")
    assert torch.equal(g8.scores[0], ref.scores[0])                        # prefill logits: the cache is not read
    assert not all(torch.equal(x, y) for x, y in zip(g8.scores[1:], ref.scores[1:]))    # later steps do read it
    assert all(bool(torch.isfinite(s[s != float("-inf")]).all()) for s in g8.scores)
    d8, d16 = _decoder(m, "fp8"), _decoder(m, None)
    assert d8.kc.dtype == d8.vc.dtype == torch.uint8 and d8.ks.dtype == d8.vs.dtype == torch.float32
    assert d16.kc.dtype == dtype and d16.ks is None
    assert d8.kc.shape == d16.kc.shape and d8.ks.shape == d16.kc.shape[:-1]
    assert d8.kc.numel() * d8.kc.element_size() * d16.kc.element_size() == d16.kc.numel() * d16.kc.element_size()   # half the bytes of bf16


def test_bf16_fp8_bf16_with_one_geometry_keeps_the_bf16_results():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    for mode in ("greedy", "beam"):
        kw = {**_kw(dims), **MODES[mode]}
        a = m.generate(**kw)
        f = m.generate(**kw, kv_cache_dtype="fp8")
        b = m.generate(**kw, kv_cache_dtype=None)
        assert _same(a, b)
        assert not _same(a, f)
        assert {d.kv_dtype for d in m._decoders.values()} == {None, "fp8"}


def test_unknown_kv_cache_dtype_raises():
    dims = dims_tiny()
    m = _model(dims, torch.float32)
    kw = _kw(dims)
    for bad in ("int8", "e5m2", "bf16", torch.float8_e4m3fn):
        with pytest.raises(ValueError):
            m.generate(**kw, kv_cache_dtype=bad)
        with pytest.raises(ValueError):
            m.generate(**kw, kv_cache_dtype=bad, num_beams=2)


def test_teacher_forced_logit_error_at_7b_width():
    """7B width, 2 layers (bf16, fused single-token step: qkv_finish_fp8): both decoders step on the bf16 run's tokens for 16 steps."""
    tool = _tool()
    m, dims = tool.model_7b(layers=2)
    err = tool.teacher_forced_error(m, dims, B=8, steps=16)
    print(f"kv8 teacher-forced relative logit error (7B width, 2 layers, bs 8, 16 steps): {err:.5f}")
    assert 0 < err <= 0.1


def test_full_size_fp8_graph_replays_deterministically_and_per_row():
    """bs 256, 32 layers, fp8 cache: the captured loop replays bit for bit, and permuting the rows of the decoder's state after prefill (cache
    codes and scales, prefill logits, sequences, key mask) permutes the generated ids exactly.  The state is permuted rather than prefilled
    anew in another order because the prompt pass itself does not give row-order-independent bits (the bf16 cache's prefill logits differ
    too); the token loop on the fp8 cache is what is pinned here."""
    from egoscaler_amd.decode import Decoder
    tool = _tool()
    m, dims = tool.model_7b()
    B, T = 256, 16
    ids, pcs, st = tool.inputs(dims, B, distinct=16)
    g = torch.Generator().manual_seed(0)
    ids[:, -1] = torch.randint(0, 4000, (B,), generator=g).cuda()          # every row its own prompt
    S0 = ids.shape[1]
    dec = Decoder(m.engine, B, S0 + T, kv_dtype="fp8")
    dec.prefill_chunked(ids, None, pcs, st, T, chunk=16)
    names = ("kc", "vc", "ks", "vs")
    state = {n: getattr(dec, n).clone() for n in names}
    lg0, seq0, mask0 = dec.lg.clone(), dec.seq_buf.clone(), dec.mask_buf.clone()
    dec.greedy(T, use_graph=True, keep_scores=False)
    torch.cuda.synchronize()
    seq1 = dec.seq.clone()
    dec.lg.copy_(lg0)
    dec.graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dec.seq, seq1)
    perm = torch.randperm(B, generator=g).cuda()
    for n in names:
        getattr(dec, n).copy_(state[n][:, perm])
    dec.lg.copy_(lg0[perm])
    dec.seq_buf.copy_(seq0[perm])
    dec.mask_buf.copy_(mask0[perm])
    dec.graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dec.seq, seq1[perm])
    assert int((seq1[:, S0:] != seq1[:1, S0:]).any(1).sum()) > 0           # the rows do differ


def test_driver_eval_tiny_kv_cache_dtype_fp8(tmp_path, monkeypatch):
    from egoscaler_amd import driver
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    seen = []
    gen = TrajPointLLMForCausalLM.generate

    def spy(self, *a, **k):
        seen.append(k.get("kv_cache_dtype"))
        return gen(self, *a, **k)
    monkeypatch.setattr(TrajPointLLMForCausalLM, "generate", spy)
    driver.main(["eval", "--tiny", "--kv_cache_dtype", "fp8", "--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5",
                 "--max_traj_token", "48", "--val_greedy", "--out_dir", str(tmp_path)])
    assert seen and all(x == "fp8" for x in seen)
    assert driver.parse_args(["eval", "--tiny"]).kv_cache_dtype == "auto"
