"""GPU: generate(decode_weight_dtype="fp8") — the decode steps' four projections on e4m3fn codes (csrc/w8.hip) under every generation mode
and either KV dtype.  The captured loop equals the eager one bit for bit, step 0 (prefill, bf16 weights) equals the bf16 run's, the decode
steps multiply bf16(code * s) and not the model's weights, the fp8 copies are shared by the cached decoders and follow every change of the
weights, the bad configurations raise, the driver flag runs, and the teacher-forced logit error at 7B width is small but not zero."""
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

MODES = {"greedy": dict(do_sample=False), "sample": dict(do_sample=True, seed=11, top_k=20, top_p=0.9, temperature=0.8),
         "beam": dict(num_beams=4, num_return_sequences=2, do_sample=False)}
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _model(dims, dtype, sd=None, unfreeze=False):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=unfreeze, num_bins=dims.tok.num_bins, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, 0) if sd is None else sd
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()})
    return m.eval()


def _outliers(sd, dims, seed=3):
    """Every projection row gets one entry of +-448 * 2^e, e chosen so that it is about 8x the row's rms: it becomes the row's amax, so
    s_n = 2^e exactly and bf16(code * s) is exact, and the rest of the row loses visible precision to e4m3fn."""
    g = torch.Generator().manual_seed(seed)
    sd = dict(sd)
    for l in range(dims.lm.num_hidden_layers):
        for p in PROJ:
            k = f"model.layers.{l}.{p}.weight"
            w = sd[k].float().clone()
            rms = w.pow(2).mean(1).sqrt()
            e = torch.round(torch.log2(8 * rms / 448.0))
            col = torch.randint(0, w.shape[1], (w.shape[0],), generator=g)
            sign = torch.where(torch.rand(w.shape[0], generator=g) < 0.5, -1.0, 1.0)
            w[torch.arange(w.shape[0]), col] = sign * 448.0 * torch.exp2(e)
            assert bool((w.abs().amax(1) == 448.0 * torch.exp2(e)).all())
            sd[k] = w
    return sd


def w8_quantize(w):
    """decode.w8_quantize on the host (IEEE division; torch's device division of amax / 448 is not correctly rounded), back on the device."""
    from egoscaler_amd.decode import w8_quantize as q
    c, s = q(w.detach().cpu())
    return c.to(w.device), s.to(w.device)


def _tool():
    spec = importlib.util.spec_from_file_location("bench_decode_w8", os.path.join(ROOT, "tools", "bench_decode_w8.py"))
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


@pytest.mark.parametrize("kv", ["auto", "fp8"])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_fp8_weights_graph_equals_eager_step0_equals_bf16(mode, kv):
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    kw = {**_kw(dims), **MODES[mode], "kv_cache_dtype": kv}
    g8 = m.generate(**kw, decode_weight_dtype="fp8")
    e8 = m.generate(**kw, decode_weight_dtype="fp8", use_graph=False)
    assert _same(g8, e8)
    ref = m.generate(**kw, decode_weight_dtype="auto")
    assert torch.equal(g8.scores[0], ref.scores[0])                        # prefill logits: bf16 weights
    assert not all(torch.equal(x, y) for x, y in zip(g8.scores[1:], ref.scores[1:]))    # later steps read the fp8 weights
    assert all(bool(torch.isfinite(s[s != float("-inf")]).all()) for s in g8.scores)


@torch.no_grad()
def test_decode_steps_multiply_the_dequantized_weights():
    """Discriminating check: one prefill on the (outlier-carrying) bf16 weights, then teacher-forced single-token steps from copies of that
    cache state with fp8 weights, with a bf16 decoder whose four projections are bf16(code * s), and with the unmodified bf16 decoder."""
    from egoscaler_amd.decode import Decoder, argmax_rows
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16, _outliers(synth.synth_state_dict(dims, 0), dims))
    eng = m.engine
    kw = _kw(dims, B=2, T=8)
    ids = kw["input_ids"]
    B, S0, T = ids.shape[0], ids.shape[1], 6
    d16 = Decoder(eng, B, S0 + T + 1)
    d8 = Decoder(eng, B, S0 + T + 1, weight_dtype="fp8")
    dq = Decoder(eng, B, S0 + T + 1)
    deq = lambda t: (lambda c, s: (c.view(torch.float8_e4m3fn).float() * s[:, None]).to(torch.bfloat16))(*w8_quantize(t))
    L = dims.lm.num_hidden_layers
    wq = dict(eng.w)
    for l in range(L):
        for p in ("self_attn.o_proj", "mlp.down_proj"):
            wq[f"model.layers.{l}.{p}.weight"] = deq(eng.w[f"model.layers.{l}.{p}.weight"])
    dq.wqkv = [deq(t) for t in dq.wqkv]
    dq.wgu = [deq(t) for t in dq.wgu]
    dq.eng = types.SimpleNamespace(w=wq, dims=eng.dims, cos=eng.cos, sin=eng.sin, gu_il=eng.gu_il)
    for l in range(L):                                                    # the fp8 decoder's codes are those of the same stacks
        assert torch.equal(d8.w8[l]["qkv"][0], w8_quantize(d16.wqkv[l])[0]) and torch.equal(d8.w8[l]["gu"][0], w8_quantize(d16.wgu[l])[0])
    d16.prefill(ids, kw["attention_mask"], kw["point_clouds"], kw["fps_start"], T + 1)
    for d in (d8, dq):
        for n in ("kc", "vc", "lg", "seq_buf", "mask_buf"):
            getattr(d, n).copy_(getattr(d16, n))
        d.mask, d.pos = d.mask_buf, d16.pos
    e_q = e_16 = 0.0
    for t in range(T):
        argmax_rows(d16.lg, d16.tok.view(-1))
        for d in (d8, dq):
            d.tok.copy_(d16.tok)
        for d in (d16, d8, dq):
            d.step(S0 + t)
        l8, lq, l16 = d8.lg.float(), dq.lg.float(), d16.lg.float()
        e_q = max(e_q, float((l8 - lq).norm() / lq.norm()))
        e_16 = max(e_16, float((l8 - l16).norm() / l16.norm()))
    print(f"fp8 vs bf16(code*s): {e_q:.2e}   fp8 vs bf16 weights: {e_16:.2e}")
    tol = 2e-3
    assert e_q <= tol
    assert e_16 >= 10 * tol


def test_bf16_fp8_bf16_and_the_decoder_cache():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    for mode in ("greedy", "beam"):
        kw = {**_kw(dims), **MODES[mode]}
        a = m.generate(**kw)
        f = m.generate(**kw, decode_weight_dtype="fp8")
        b = m.generate(**kw, decode_weight_dtype=None)
        assert _same(a, b)
        assert not _same(a, f)
        w8 = [d for d in m._decoders.values() if d.w8 is not None]
        assert len(w8) == 1 and len(m._decoders) == 2
        q = w8[0].w8
        assert all(c.dtype == torch.uint8 and s.dtype == torch.float32 for lay in q for c, s in lay.values())
        assert m.engine.w8 is not None and m.engine.w8[1] is q              # held on the engine, keyed by its prepare epoch
        assert m.engine.w8[0] == m.engine.prepare_epoch
    kw = {**_kw(dims, T=4), **MODES["greedy"]}
    f1 = m.generate(**kw, decode_weight_dtype="fp8")                       # another geometry: a second fp8 decoder, the same copy
    assert _same(f1, m.generate(**kw, decode_weight_dtype="fp8"))
    assert all(d.w8 is m.engine.w8[1] for d in m._decoders.values() if d.w8 is not None)


def test_fp8_weights_follow_load_state_dict_and_apply():
    dims = dims_tiny()
    sd0, sd1 = synth.synth_state_dict(dims, 0), synth.synth_state_dict(dims, 1)
    kw = {**_kw(dims), **MODES["greedy"]}
    m = _model(dims, torch.bfloat16, sd0)
    a0 = m.generate(**kw, decode_weight_dtype="fp8")
    m.load_state_dict({k: (v.to(torch.bfloat16) if v.dtype.is_floating_point else v) for k, v in sd1.items()})
    assert m.engine.w8 is None                                            # unprepared: the copies are dropped
    a1 = m.generate(**kw, decode_weight_dtype="fp8")
    fresh = _model(dims, torch.bfloat16, sd1)
    assert _same(a1, fresh.generate(**kw, decode_weight_dtype="fp8"))
    assert not _same(a0, a1)
    # an in-place change of a projection is picked up by .to() / _apply (the engine is rebuilt), not left in a stale fp8 copy
    with torch.no_grad():
        for l in range(dims.lm.num_hidden_layers):
            dict(m.named_parameters())[f"model.layers.{l}.self_attn.o_proj.weight"].mul_(-1.5)
    m.to("cuda")
    a2 = m.generate(**kw, decode_weight_dtype="fp8")
    sd2 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert _same(a2, _model(dims, torch.bfloat16, sd2).generate(**kw, decode_weight_dtype="fp8"))
    assert not _same(a1, a2)


def test_trainable_llm_requantizes_after_an_optimizer_step(monkeypatch):
    from egoscaler_amd import decode
    from egoscaler_amd.optim import EgoAdamW
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16, unfreeze=True)
    seen = []
    orig = decode.Decoder._fp8_weights

    def spy(self):
        q = orig(self)
        seen.append(q)
        return q
    monkeypatch.setattr(decode.Decoder, "_fp8_weights", spy)
    kw = {**_kw(dims), **MODES["greedy"]}
    a = m.generate(**kw, decode_weight_dtype="fp8")
    opt = EgoAdamW(m, lr=1e-2, weight_decay=0.0)
    m.train()
    toks, masks, Lp = synth.synth_batch(dims, 2, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(2)]).cuda()
    m.loss_and_backward(toks.cuda(), masks.cuda(), pts, Lp, dims.tok.pad, fps_start=np.array([0, 17]))
    opt.step()
    m.eval()
    b = m.generate(**kw, decode_weight_dtype="fp8")
    assert len(seen) == 2 and m.engine.w8 is None                         # quantized afresh on each call, never cached
    assert not _same(a, b)
    params = dict(m.named_parameters())
    for l in range(dims.lm.num_hidden_layers):
        c, s = w8_quantize(params[f"model.layers.{l}.mlp.down_proj.weight"].detach())
        assert torch.equal(seen[-1][l]["down"][0], c) and torch.equal(seen[-1][l]["down"][1], s)
        c, s = w8_quantize(params[f"model.layers.{l}.self_attn.o_proj.weight"].detach())
        assert torch.equal(seen[-1][l]["o"][0], c)
        assert not torch.equal(seen[0][l]["o"][0], c)


def test_bad_configurations_raise():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    kw = _kw(dims)
    for bad in ("int8", "e5m2", "bf16", torch.float8_e4m3fn):
        with pytest.raises(ValueError):
            m.generate(**kw, decode_weight_dtype=bad)
        with pytest.raises(ValueError):
            m.generate(**kw, decode_weight_dtype=bad, num_beams=2)
    m32 = _model(dims, torch.float32)
    with pytest.raises(ValueError, match="bf16"):
        m32.generate(**kw, decode_weight_dtype="fp8")
    big = {**kw, "input_ids": kw["input_ids"][:1].repeat(130, 1), "attention_mask": None, "point_clouds": kw["point_clouds"][:1].repeat(130, 1, 1),
           "fps_start": [0] * 130}
    with pytest.raises(ValueError, match="512"):
        m.generate(**big, decode_weight_dtype="fp8", num_beams=4)          # 520 decoder rows


def test_driver_eval_tiny_decode_weight_dtype_fp8(tmp_path, monkeypatch):
    from egoscaler_amd import driver
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    seen = []
    gen = TrajPointLLMForCausalLM.generate

    def spy(self, *a, **k):
        seen.append(k.get("decode_weight_dtype"))
        return gen(self, *a, **k)
    monkeypatch.setattr(TrajPointLLMForCausalLM, "generate", spy)
    driver.main(["eval", "--tiny", "--decode_weight_dtype", "fp8", "--dtype", "bf16", "--bs", "2", "--n_val", "4", "--num_steps", "5",
                 "--max_traj_token", "48", "--val_greedy", "--out_dir", str(tmp_path)])
    assert seen and all(x == "fp8" for x in seen)
    assert os.path.exists(os.path.join(tmp_path, "test_gen_trajs.json"))
    assert driver.parse_args(["eval", "--tiny"]).decode_weight_dtype == "auto"


@pytest.mark.parametrize("B", [8, 32])
def test_teacher_forced_logit_error_at_7b_width(B):
    """7B width, 2 layers, seeded weights: both decoders step on the bf16 run's tokens for 16 steps; B = 8 (validation) and 32 rows (the
    8 x 4 beams of evaluation)."""
    tool = _tool()
    m, dims = tool.model_7b(layers=2)
    err = tool.teacher_forced_error(m, dims, B=B, steps=16, distinct=8)
    print(f"w8 teacher-forced relative logit error (7B width, 2 layers, {B} rows, 16 steps): {err:.5f}")
    assert 0 < err <= 0.1
