"""GPU: generate(decode_weight_dtype="int4") — the decode steps' four projections on group-scaled 4-bit codes (csrc/w4.hip) under every
generation mode and either KV dtype.  The captured loop equals the eager one bit for bit, step 0 (prefill, bf16 weights) equals the bf16
run's, the decode steps multiply bf16(code * s) and not the model's weights, the shared-prompt and split-cache steps read the codes, the
int4 copies follow every change of the weights (LoRA merge, load_state_dict, optimizer steps) and leave the other formats alone, the bad
configurations raise, the driver flag runs, and the teacher-forced logit error at 7B width lies between fp8's and a measured bound."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import lora, synth
from egoscaler_amd.config import dims_tiny
from tests.test_gpu_w8_generate import MODES, PROJ, _kw, _model, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def w4_quantize(w):
    """decode.w4_quantize on the host (IEEE division), back on the device."""
    from egoscaler_amd.decode import w4_quantize as q
    c, s = q(w.detach().cpu())
    return c.to(w.device), s.to(w.device)


def _tool():
    spec = importlib.util.spec_from_file_location("bench_decode_w4", os.path.join(ROOT, "tools", "bench_decode_w4.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _int4_decoders(m):
    return [d for d in m._decoders.values() if d.w4 is not None]


def _group_outliers(sd, dims, seed=3):
    """Every 128-column group of every projection row gets one entry of +-7 * 2^e, e chosen so that it is about 8x the row's rms: it is
    the group's amax, so s = 2^e exactly and bf16(code * s) is exact, and the rest of the group is coded in steps of about one rms."""
    g = torch.Generator().manual_seed(seed)
    sd = dict(sd)
    for l in range(dims.lm.num_hidden_layers):
        for p in PROJ:
            k = f"model.layers.{l}.{p}.weight"
            w = sd[k].float().clone()
            N, K = w.shape
            top = 7.0 * torch.exp2(torch.round(torch.log2(8 * w.pow(2).mean(1).sqrt() / 7.0)))
            for k0 in range(0, K, 128):
                k1 = min(K, k0 + 128)
                col = torch.randint(k0, k1, (N,), generator=g)
                sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
                w[torch.arange(N), col] = sign * top
                assert bool((w[:, k0:k1].abs().amax(1) == top).all())
            sd[k] = w
    return sd


@pytest.mark.parametrize("kv", ["auto", "fp8"])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_int4_weights_graph_equals_eager_step0_equals_bf16(mode, kv):
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    kw = {**_kw(dims), **MODES[mode], "kv_cache_dtype": kv}
    g4 = m.generate(**kw, decode_weight_dtype="int4")
    e4 = m.generate(**kw, decode_weight_dtype="int4", use_graph=False)
    assert _same(g4, e4)
    ref = m.generate(**kw, decode_weight_dtype="auto")
    assert torch.equal(g4.scores[0], ref.scores[0])                        # prefill logits: bf16 weights
    assert not any(torch.equal(x, y) for x, y in zip(g4.scores[1:], ref.scores[1:]))    # every later step reads the int4 weights
    assert all(bool(torch.isfinite(s[s != float("-inf")]).all()) for s in g4.scores)


@torch.no_grad()
def test_decode_steps_multiply_the_dequantized_weights():
    """Discriminating check: one prefill on the (outlier-carrying) bf16 weights, then teacher-forced single-token steps from copies of that
    cache state with int4 weights, with a bf16 decoder whose four projections are bf16(code * s) (exact: s is a power of two), and with the
    unmodified bf16 decoder.  2e-3 is the project's bound for two bf16 decoders on equal weights (tests/test_gpu_w8_generate.py)."""
    from egoscaler_amd.decode import Decoder, argmax_rows, w4_dequantize
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16, _group_outliers(synth.synth_state_dict(dims, 0), dims))
    eng = m.engine
    kw = _kw(dims, B=2, T=8)
    ids = kw["input_ids"]
    B, S0, T = ids.shape[0], ids.shape[1], 6
    d16 = Decoder(eng, B, S0 + T + 1)
    d4 = Decoder(eng, B, S0 + T + 1, weight_dtype="int4")
    dq = Decoder(eng, B, S0 + T + 1)
    assert d4.w8 is None and d4.wq is d4.w4 and eng.w4[1] is d4.w4 and eng.w8 is None

    def deq(t):
        packed, s = w4_quantize(t)
        assert bool((torch.exp2(torch.round(torch.log2(s))) == s).all())  # every scale a power of two
        d = w4_dequantize(packed, s, t.shape[1])
        assert torch.equal(d.to(torch.bfloat16).float(), d)
        return d.to(torch.bfloat16)
    L = dims.lm.num_hidden_layers
    wq = dict(eng.w)
    for l in range(L):
        for p in ("self_attn.o_proj", "mlp.down_proj"):
            wq[f"model.layers.{l}.{p}.weight"] = deq(eng.w[f"model.layers.{l}.{p}.weight"])
    dq.wqkv = [deq(t) for t in dq.wqkv]
    dq.wgu = [deq(t) for t in dq.wgu]
    dq.eng = types.SimpleNamespace(w=wq, dims=eng.dims, cos=eng.cos, sin=eng.sin, gu_il=eng.gu_il)
    for l in range(L):                                                    # the int4 decoder's codes and scales are those of the same stacks
        for name, stack in (("qkv", d16.wqkv[l]), ("gu", d16.wgu[l]), ("o", d16._w(l, "o")), ("down", d16._w(l, "down"))):
            packed, s = w4_quantize(stack)
            assert torch.equal(d4.w4[l][name][0], packed) and torch.equal(d4.w4[l][name][1], s), (l, name)
    d16.prefill(ids, kw["attention_mask"], kw["point_clouds"], kw["fps_start"], T + 1)
    for d in (d4, dq):
        for n in ("kc", "vc", "lg", "seq_buf", "mask_buf"):
            getattr(d, n).copy_(getattr(d16, n))
        d.mask, d.pos = d.mask_buf, d16.pos
    e_q = e_16 = 0.0
    for t in range(T):
        argmax_rows(d16.lg, d16.tok.view(-1))
        for d in (d4, dq):
            d.tok.copy_(d16.tok)
        for d in (d16, d4, dq):
            d.step(S0 + t)
        l4, lq, l16 = d4.lg.float(), dq.lg.float(), d16.lg.float()
        e_q = max(e_q, float((l4 - lq).norm() / lq.norm()))
        e_16 = max(e_16, float((l4 - l16).norm() / l16.norm()))
    print(f"int4 vs bf16(code*s): {e_q:.2e}   int4 vs bf16 weights: {e_16:.2e}")
    tol = 2e-3
    assert e_q <= tol
    assert e_16 >= 10 * tol


def test_int4_weights_run_in_the_shared_and_the_split_steps():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    from egoscaler_amd.decode import SplitCache
    for extra in (dict(do_sample=True, seed=11, top_k=20, top_p=0.9, num_return_sequences=3, share_prompt=True),
                  dict(do_sample=False, num_beams=2, kv_cache_layout="split")):
        kw = {**_kw(dims), **extra}
        q = m.generate(**kw, decode_weight_dtype="int4")
        dec = _int4_decoders(m)
        assert len(dec) == 1 and isinstance(dec[0].cache, SplitCache) and dec[0].fused["qkv"] == 0
        assert _same(q, m.generate(**kw, decode_weight_dtype="int4", use_graph=False))
        bf = m.generate(**kw)
        assert torch.equal(q.scores[0], bf.scores[0]) and not torch.equal(q.scores[1], bf.scores[1])
        m.__dict__.pop("_decoders", None)


def test_lora_merge_reaches_the_codes():
    from tests.test_gpu_lora import _model as _lora_model
    dims = dims_tiny()
    m = _lora_model(dims, torch.bfloat16).eval()
    kw = {**_kw(dims), **MODES["greedy"]}
    a = m.generate(**kw, decode_weight_dtype="int4")
    assert torch.equal(a.scores[0], m.generate(**kw).scores[0])
    d4, = _int4_decoders(m)
    eng = m.engine
    for l in range(dims.lm.num_hidden_layers):
        merged, base = eng.lora_merged(l, "o_proj"), eng.w[lora.base_name(l, "o_proj")]
        assert torch.equal(d4.w4[l]["o"][0], w4_quantize(merged)[0]) and not torch.equal(d4.w4[l]["o"][0], w4_quantize(base)[0])
        assert torch.equal(d4.w4[l]["qkv"][0], w4_quantize(d4.wqkv[l])[0]) and torch.equal(d4.w4[l]["gu"][1], w4_quantize(d4.wgu[l])[1])
        assert not torch.equal(d4.w4[l]["qkv"][0], w4_quantize(eng.wqkv[l] if l in eng.wqkv else torch.cat(
            [eng.w[lora.base_name(l, t)] for t in ("q_proj", "k_proj", "v_proj")], 0))[0])
    with torch.no_grad():                                                 # new adapter values: the held copies are dropped with them
        for n, p in m.named_parameters():
            if n.endswith("lora_B.weight"):
                p.mul_(-1.0)
    m.load_state_dict(m.state_dict())
    assert m.engine.w4 is None
    assert not _same(a, m.generate(**kw, decode_weight_dtype="int4"))


def test_int4_weights_follow_load_state_dict():
    dims = dims_tiny()
    sd0, sd1 = synth.synth_state_dict(dims, 0), synth.synth_state_dict(dims, 1)
    kw = {**_kw(dims), **MODES["greedy"]}
    m = _model(dims, torch.bfloat16, sd0)
    a0 = m.generate(**kw, decode_weight_dtype="int4")
    assert m.engine.w4 is not None and m.engine.w4[0] == m.engine.prepare_epoch
    m.load_state_dict({k: (v.to(torch.bfloat16) if v.dtype.is_floating_point else v) for k, v in sd1.items()})
    assert m.engine.w4 is None                                            # unprepared: the copies are dropped
    a1 = m.generate(**kw, decode_weight_dtype="int4")
    assert _same(a1, _model(dims, torch.bfloat16, sd1).generate(**kw, decode_weight_dtype="int4"))
    assert not _same(a0, a1)


def test_trainable_llm_requantizes_after_an_optimizer_step(monkeypatch):
    from egoscaler_amd import decode
    from egoscaler_amd.optim import EgoAdamW
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16, unfreeze=True)
    seen = []
    orig = decode.Decoder._int4_weights

    def spy(self):
        q = orig(self)
        seen.append(q)
        return q
    monkeypatch.setattr(decode.Decoder, "_int4_weights", spy)
    kw = {**_kw(dims), **MODES["greedy"]}
    a = m.generate(**kw, decode_weight_dtype="int4")
    opt = EgoAdamW(m, lr=1e-2, weight_decay=0.0)
    m.train()
    toks, masks, Lp = synth.synth_batch(dims, 2, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(2)]).cuda()
    m.loss_and_backward(toks.cuda(), masks.cuda(), pts, Lp, dims.tok.pad, fps_start=np.array([0, 17]))
    opt.step()
    m.eval()
    b = m.generate(**kw, decode_weight_dtype="int4")
    assert len(seen) == 2 and m.engine.w4 is None                         # quantized afresh on each call, never cached
    assert not _same(a, b)
    params = dict(m.named_parameters())
    for l in range(dims.lm.num_hidden_layers):
        c, s = w4_quantize(params[f"model.layers.{l}.mlp.down_proj.weight"].detach())
        assert torch.equal(seen[-1][l]["down"][0], c) and torch.equal(seen[-1][l]["down"][1], s)
        c, s = w4_quantize(params[f"model.layers.{l}.self_attn.o_proj.weight"].detach())
        assert torch.equal(seen[-1][l]["o"][0], c)
        assert not torch.equal(seen[0][l]["o"][0], c)


def test_bf16_int4_fp8_bf16_on_one_geometry():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16)
    for mode in ("greedy", "beam"):
        kw = {**_kw(dims), **MODES[mode]}
        a = m.generate(**kw)
        q4 = m.generate(**kw, decode_weight_dtype="int4")
        q8 = m.generate(**kw, decode_weight_dtype="fp8")
        b = m.generate(**kw, decode_weight_dtype=None)
        assert _same(a, b) and not _same(a, q4) and not _same(a, q8) and not _same(q4, q8)
        assert _same(q4, m.generate(**kw, decode_weight_dtype="int4"))
        assert m.engine.w4 is not None and m.engine.w8 is not None        # both copies held on the engine, each under its own name
        assert all(p.dtype == torch.uint8 and s.dtype == torch.float32 and s.shape[1] == p.shape[0] and p.shape[1] * 2 in (128, 352)
                   for lay in m.engine.w4[1] for p, s in lay.values())
        assert all(d.w8 is None for d in _int4_decoders(m))


def test_bad_configurations_raise():
    dims = dims_tiny()
    kw = _kw(dims)
    m32 = _model(dims, torch.float32)
    with pytest.raises(ValueError, match="bf16"):
        m32.generate(**kw, decode_weight_dtype="int4")
    m = _model(dims, torch.bfloat16)
    big = {**kw, "input_ids": kw["input_ids"][:1].repeat(130, 1), "attention_mask": None, "point_clouds": kw["point_clouds"][:1].repeat(130, 1, 1),
           "fps_start": [0] * 130}
    with pytest.raises(ValueError, match="512"):
        m.generate(**big, decode_weight_dtype="int4", num_beams=4)         # 520 decoder rows
    with pytest.raises(ValueError):
        m.generate(**kw, decode_weight_dtype="int3")


def test_driver_eval_tiny_decode_weight_dtype_int4(tmp_path, monkeypatch):
    from egoscaler_amd import driver
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    seen = []
    gen = TrajPointLLMForCausalLM.generate

    def spy(self, *a, **k):
        seen.append(k.get("decode_weight_dtype"))
        return gen(self, *a, **k)
    monkeypatch.setattr(TrajPointLLMForCausalLM, "generate", spy)
    driver.main(["eval", "--tiny", "--decode_weight_dtype", "int4", "--dtype", "bf16", "--bs", "2", "--n_val", "4", "--num_steps", "5",
                 "--max_traj_token", "48", "--val_greedy", "--out_dir", str(tmp_path)])
    assert seen and all(x == "int4" for x in seen)
    assert os.path.exists(os.path.join(tmp_path, "test_gen_trajs.json"))


INT4_BOUND = 0.40      # 1.5 x the 0.2637 measured on the MI355X, rounded up to two digits (profiles/w4_decode.txt)


def test_teacher_forced_logit_error_at_7b_width():
    """7B width, 2 layers, seeded weights, B = 8: both decoders step on the bf16 run's tokens for 16 steps.  Measured on the MI355X: int4
    0.2637, fp8 0.0627 (the weight-error ratio 11.7 % / 2.6 % of Gaussian weights predicts 0.063 * 4.5 = 0.28); bound 0.40 = 1.5 x the
    measurement, rounded up to two digits.  The seeded weights have no outlier channels: accuracy on a real checkpoint is not measured."""
    tool = _tool()
    m, dims = tool.model_7b(layers=2)
    err = tool.teacher_forced_error(m, dims, B=8, steps=16, distinct=8, weight_dtype="int4")
    err8 = tool.teacher_forced_error(m, dims, B=8, steps=16, distinct=8, weight_dtype="fp8")
    print(f"teacher-forced relative logit error (7B width, 2 layers, 8 rows, 16 steps): int4 {err:.5f}  fp8 {err8:.5f}")
    assert err8 < err <= INT4_BOUND
