"""GPU: LoRA adapters end to end.  The oracle runs the reference model on the merged weights W + s B A with A and B as autograd leaves, so
torch gives the exact adapter gradients without touching oracle/.  Covers fp32 parity (logits, loss, dA, dB, the frozen-mode gradients),
AdamW steps, fresh adapters, bit-reproducible steps, generate() in every mode against merged models, merge_lora, save/load_lora and the
driver."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import lora, synth
from egoscaler_amd.config import dims_tiny

pytestmark = pytest.mark.gpu
ALL7 = ",".join(lora.TARGETS)


def _model(dims, dtype, r=8, alpha=16.0, targets=ALL7, sd=None, nonzero_B=True, seed=0):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None,
                                 lora_r=r, lora_alpha=alpha, lora_target_modules=targets)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, 0) if sd is None else sd
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}, strict=False)
    if nonzero_B:
        g = torch.Generator().manual_seed(seed + 5)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("lora_B.weight"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
                elif n.endswith("lora_A.weight"):
                    p.mul_(4.0)                                  # A ~ U(+-4/sqrt(in)): a LoRA term comparable to the base product
        m.load_state_dict(m.state_dict())                        # (marks the engine's derived copies stale, as a checkpoint load does)
    return m


def _batch(dims, B=2):
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)])
    return toks, masks, pts, Lp, np.array([0, 17, 5, 9][:B])


def _merged_sd(model):
    """The reference's state dict with every adapter folded in on the host in fp32 (no adapter keys)."""
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    cfg = model.lora_cfg
    out = {k: v for k, v in sd.items() if not lora.is_adapter(k)}
    for l in range(model.dims.lm.num_hidden_layers):
        for t in cfg.targets:
            a, b = lora.adapter_names(l, t)
            out[lora.base_name(l, t)] = out[lora.base_name(l, t)] + cfg.scale * sd[b] @ sd[a]
    return out


def _oracle(model, toks, masks, pts, start, Lp, trainable):
    """Oracle loss with the model's trainable tensors and the adapters as leaves; -> (loss, logits, {name: grad})."""
    from oracle import pointllm as OPL, llama as OL
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k in sd if k in trainable}
    cfg = model.lora_cfg
    use = {k: v for k, v in sd.items() if not lora.is_adapter(k)}
    for l in range(model.dims.lm.num_hidden_layers):
        for t in cfg.targets:
            a, b = lora.adapter_names(l, t)
            use[lora.base_name(l, t)] = sd[lora.base_name(l, t)] + cfg.scale * sd[b] @ sd[a]
    logits = OPL.forward(use, model.dims, toks, masks, pts, start)
    loss = OL.traj_loss(logits, toks, Lp, model.dims.tok.pad)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in leaves.items()}


def _rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max()) / (float(b.float().abs().max()) + 1e-12)


@pytest.mark.parametrize("targets", [ALL7, "q_proj,v_proj", "k_proj,up_proj"])
def test_tiny_fp32_parity_with_oracle(targets):
    dims = dims_tiny()
    m = _model(dims, torch.float32, targets=targets).train()
    toks, masks, pts, Lp, start = _batch(dims)
    loss = m.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
    params = dict(m.named_parameters())
    trainable = [n for n, p in params.items() if p.requires_grad]
    assert sum(lora.is_adapter(n) for n in trainable) == 2 * dims.lm.num_hidden_layers * len(targets.split(","))
    assert not any(n.startswith("model.layers.") and not lora.is_adapter(n) for n in trainable)     # base layers frozen
    lo, logits_o, grads = _oracle(m, toks, masks, pts, start, Lp, set(trainable))
    assert abs(float(loss) - float(lo)) < 1e-4 * abs(float(lo))
    with torch.no_grad():
        logits = m(input_ids=toks.cuda(), attention_mask=masks.cuda(), point_clouds=pts.cuda(), fps_start=start).logits
    assert _rel(logits, logits_o) < 1e-4
    for n in trainable:
        assert grads[n] is not None, n
        assert _rel(params[n].main_grad, grads[n]) < 2e-3, (n, _rel(params[n].main_grad, grads[n]))


def test_adamw_steps_match_torch():
    from egoscaler_amd.optim import EgoAdamW
    dims = dims_tiny()
    m = _model(dims, torch.float32).train()
    toks, masks, pts, Lp, start = _batch(dims)
    params = dict(m.named_parameters())
    trainable = [n for n, p in params.items() if p.requires_grad]
    opt = EgoAdamW(m, lr=1e-3, weight_decay=0.01)
    ref = copy.deepcopy({k: v.detach().float().cpu() for k, v in m.state_dict().items()})
    leaves = {k: ref[k].clone().requires_grad_(True) for k in trainable}
    topt = torch.optim.AdamW(list(leaves.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    from oracle import pointllm as OPL, llama as OL
    s = m.lora_cfg.scale
    for _ in range(3):
        m.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
        opt.step()
        use = {k: (leaves[k] if k in leaves else v) for k, v in ref.items() if not lora.is_adapter(k)}
        for l in range(dims.lm.num_hidden_layers):
            for t in m.lora_cfg.targets:
                a, b = lora.adapter_names(l, t)
                use[lora.base_name(l, t)] = ref[lora.base_name(l, t)] + s * leaves[b] @ leaves[a]
        topt.zero_grad()
        OL.traj_loss(OPL.forward(use, dims, toks, masks, pts, start), toks, Lp, dims.tok.pad).backward()
        topt.step()
    for n in trainable:
        assert _rel(params[n].detach(), leaves[n].detach()) < 1e-3, n


def test_fresh_adapters_change_nothing():
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dims = dims_tiny()
    toks, masks, pts, Lp, start = _batch(dims)
    m = _model(dims, torch.bfloat16, nonzero_B=False).train()
    for n, p in m.named_parameters():
        if n.endswith("lora_A.weight"):
            b = 1 / np.sqrt(p.shape[1])
            assert float(p.float().abs().max()) <= b * 1.01 and float(p.float().abs().max()) > 0.5 * b
        if n.endswith("lora_B.weight"):
            assert float(p.abs().max()) == 0
    base = TrajPointLLMForCausalLM(types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins,
                                                         model_name=None), dims, None, device="cuda", dtype=torch.bfloat16)
    base.load_state_dict({k: v.to(torch.bfloat16) if v.dtype.is_floating_point else v for k, v in synth.synth_state_dict(dims, 0).items()})
    base.train()
    l1 = m.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
    l0 = base.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
    assert abs(float(l1) - float(l0)) < 1e-2 * abs(float(l0))


def test_bf16_repeated_step_bit_equal():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16).train()
    toks, masks, pts, Lp, start = _batch(dims)
    out = []
    for _ in range(2):
        m.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
        out.append({n: p.main_grad.clone() for n, p in m.named_parameters() if lora.is_adapter(n)})
    assert all(torch.equal(out[0][n], out[1][n]) for n in out[0])
    assert all(float(v.abs().max()) > 0 for v in out[0].values())
    lo, _, grads = _oracle(m, toks, masks, pts, start, Lp, set(out[0]))
    worst = max(_rel(out[0][n], grads[n]) for n in out[0])
    assert worst < 0.08, worst


def _gen(m, ids, mask, pts, start, **kw):
    kw.setdefault("max_length", 6)
    kw.setdefault("eos_token_id", None)
    return m.generate(input_ids=ids, attention_mask=mask, point_clouds=pts, fps_start=start, **kw)


def _prompt(dims, B=2):
    toks, masks, pts, Lp, start = _batch(dims, B)
    return toks[:, :Lp].cuda(), masks[:, :Lp].cuda(), pts.cuda(), start


def test_generate_greedy_matches_oracle_and_forward():
    from oracle import pointllm as OPL
    dims = dims_tiny()
    m = _model(dims, torch.float32).eval()
    ids, mask, pts, start = _prompt(dims)
    out = _gen(m, ids, mask, pts, start, do_sample=False, output_scores=True)
    ref = OPL.greedy_generate(_merged_sd(m), dims, ids.cpu(), mask.cpu(), pts.cpu(), start, 6)
    ref = ref if isinstance(ref, torch.Tensor) else ref[0]
    assert torch.equal(out.sequences.cpu(), ref.cpu()[:, :out.sequences.shape[1]])
    with torch.no_grad():
        lg = m(input_ids=ids, attention_mask=mask, point_clouds=pts, fps_start=start).logits[:, -1]
    assert _rel(out.scores[0], lg) < 1e-5                                  # step 0: the prefill runs the unmerged adapters
    eager = _gen(m, ids, mask, pts, start, do_sample=False, use_graph=False)
    assert torch.equal(eager.sequences, out.sequences)
    assert all(torch.equal(a, b) for a, b in zip(eager.scores, out.scores))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_after_step_sees_new_adapters(dtype):
    from egoscaler_amd.optim import EgoAdamW
    dims = dims_tiny()
    m = _model(dims, dtype)
    ids, mask, pts, start = _prompt(dims)
    toks, masks, pts_t, Lp, st = _batch(dims)
    opt = EgoAdamW(m, lr=5e-2)
    first = _gen(m.eval(), ids, mask, pts, start, do_sample=False)
    m.train()
    m.loss_and_backward(toks.cuda(), masks.cuda(), pts_t.cuda(), Lp, dims.tok.pad, fps_start=st)
    opt.step(overlap=True)
    second = _gen(m.eval(), ids, mask, pts, start, do_sample=False)
    fresh = _model(dims, dtype, sd={k: v.float().cpu() for k, v in m.state_dict().items()}, nonzero_B=False)
    fresh.load_state_dict(m.state_dict())
    ref = _gen(fresh.eval(), ids, mask, pts, start, do_sample=False)
    assert torch.equal(second.sequences, ref.sequences)
    assert all(torch.equal(a, b) for a, b in zip(second.scores, ref.scores))
    assert not all(torch.equal(a, b) for a, b in zip(first.scores, second.scores))


def test_modes_run_with_adapters():
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16).eval()
    ids, mask, pts, start = _prompt(dims)
    base = _gen(m, ids, mask, pts, start, do_sample=False)
    for kw in (dict(do_sample=True, seed=3, top_k=20, top_p=0.9), dict(do_sample=False, num_return_sequences=2),
               dict(num_beams=3, num_return_sequences=2, do_sample=False), dict(do_sample=False, kv_cache_dtype="fp8"),
               dict(do_sample=False, decode_weight_dtype="fp8"), dict(num_beams=2, do_sample=False, decode_weight_dtype="fp8", kv_cache_dtype="fp8")):
        o = _gen(m, ids, mask, pts, start, **kw)
        assert o.sequences.shape[1] == ids.shape[1] + 6
    o = _gen(m, ids, mask, pts, start, do_sample=False, decode_weight_dtype="fp8")
    assert torch.equal(o.scores[0], base.scores[0])                       # step 0 is the prefill: bf16 weights, unmerged adapters


def test_merge_lora_and_peft_files(tmp_path):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dims = dims_tiny()
    m = _model(dims, torch.bfloat16).eval()
    ids, mask, pts, start = _prompt(dims)
    with torch.no_grad():
        lg = m(input_ids=ids, attention_mask=mask, point_clouds=pts, fps_start=start).logits.float()
    m.save_lora(str(tmp_path / "ad"))
    cfg = json.load(open(tmp_path / "ad" / "adapter_config.json"))
    assert cfg["r"] == 8 and cfg["target_modules"] == list(lora.TARGETS)
    ad = {k: v.clone() for k, v in m.lora_state_dict().items()}
    m2 = _model(dims, torch.bfloat16, nonzero_B=False)
    m2.load_lora(str(tmp_path / "ad"))
    assert all(torch.equal(v, m2.lora_state_dict()[k]) for k, v in ad.items())
    m.merge_lora()
    base_keys = set(TrajPointLLMForCausalLM(types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False,
                                                                  num_bins=dims.tok.num_bins, model_name=None), dims, None,
                                            device="cuda", dtype=torch.bfloat16).state_dict())
    assert set(m.state_dict()) == base_keys
    with torch.no_grad():
        lg2 = m(input_ids=ids, attention_mask=mask, point_clouds=pts, fps_start=start).logits.float()
    assert _rel(lg2, lg) < 3e-2
    o = _gen(m, ids, mask, pts, start, do_sample=False)
    assert o.sequences.shape[1] == ids.shape[1] + 6
    with pytest.raises(ValueError):
        m.save_lora(str(tmp_path / "x"))


def test_strict_load_and_errors():
    dims = dims_tiny()
    m = _model(dims, torch.float32)
    sd = {k: v for k, v in m.state_dict().items() if not lora.is_adapter(k)}
    with pytest.raises(RuntimeError, match="lora_A"):
        m.load_state_dict(sd)
    keep = m.lora_state_dict()["model.layers.0.self_attn.q_proj.lora_B.weight"].clone()
    m.load_state_dict(sd, strict=False)
    assert torch.equal(m.lora_state_dict()["model.layers.0.self_attn.q_proj.lora_B.weight"], keep)
    with pytest.raises(ValueError, match="unfreeze_language_model"):
        from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
        TrajPointLLMForCausalLM(types.SimpleNamespace(unfreeze_language_model=True, lora_r=8), dims, None, device="cuda")


def test_driver_train_resume_eval(tmp_path):
    from egoscaler_amd import driver
    out = str(tmp_path / "run")
    common = ["--tiny", "--bs", "4", "--n_train", "8", "--n_val", "4", "--out_dir", out, "--lora_r", "8",
              "--lora_target_modules", "q_proj,v_proj,down_proj"]
    driver.main(["train", *common, "--epochs", "2"])
    ck = torch.load(os.path.join(out, "latest_model.pt"), map_location="cpu", weights_only=True)
    keys = [k for k in ck["model_state_dict"] if lora.is_adapter(k)]
    assert len(keys) == 2 * 2 * 3
    assert float(ck["model_state_dict"]["model.layers.0.mlp.down_proj.lora_B.weight"].float().abs().max()) > 0     # the adapters trained
    driver.main(["train", *common, "--epochs", "3", "--resume"])
    driver.main(["eval", *common, "--split", "val", "--checkpoint_dir", out])
    with pytest.raises(ValueError, match="LoRA adapters"):
        driver.main(["eval", *common[:-4], "--split", "val", "--checkpoint_dir", out])
