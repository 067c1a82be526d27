"""GPU: EgoAdamW(max_grad_norm=...) over whole optimizer steps at tiny dimensions — a threshold that never bites changes no bit in any of
the four training modes, one that bites matches torch's clip_grad_norm_ + AdamW on the engine's own gradients, and the step stays
order-independent (overlap, repeated runs) and clips accumulated micro-batches once."""
import types

import numpy as np
import pytest
import torch

from tests import grad_clip_ref as R

pytestmark = pytest.mark.gpu

LR = 1e-3
MODES = {"frozen": dict(dtype=torch.bfloat16), "unfreeze_lm": dict(dtype=torch.bfloat16, lm=True), "unfreeze_pc": dict(dtype=torch.float32, pc=True),
         "lora": dict(dtype=torch.bfloat16, lora=True)}


def _dims():
    from egoscaler_amd.config import dims_tiny
    d = dims_tiny()
    d.lm.hidden_size, d.lm.num_attention_heads, d.lm.intermediate_size = 256, 2, 512
    return d


def _build(mode):
    from egoscaler_amd import synth
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    cfg, dims = MODES[mode], _dims()
    dtype = cfg["dtype"]
    args = types.SimpleNamespace(unfreeze_pc_encoder=bool(cfg.get("pc")), unfreeze_language_model=bool(cfg.get("lm")), num_bins=dims.tok.num_bins,
                                 model_name=None)
    if cfg.get("lora"):
        args.lora_r, args.lora_alpha, args.lora_target_modules = 8, 16.0, "q_proj,v_proj"
    torch.manual_seed(0)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, 0)
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}, strict=not cfg.get("lora"))
    if cfg.get("lora"):
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("lora_B.weight"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
        m.load_state_dict(m.state_dict())
    m.train()
    return m, dims


def _batch(dims, n):
    from egoscaler_amd import synth
    toks, masks, Lp = synth.synth_batch(dims, n, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(n)])
    return toks.cuda(), masks.cuda(), pts.cuda(), Lp, [0, 17, 3, 9][:n]


def _grads(m, opt):
    eng = m.engine
    return {n: eng.reduced_grad.get(n, eng.main_grad.get(n)).detach().clone() for n in opt.state
            if eng.reduced_grad.get(n, eng.main_grad.get(n)) is not None}


def _state(m, opt):
    m.engine.wait_param_updates()
    torch.cuda.synchronize()
    out = {}
    for n, st in opt.state.items():
        for k in ("master", "m", "v"):
            out[f"{n}/{k}"] = st[k].detach().cpu().clone()
        out[f"{n}/p"] = st["p"].detach().cpu().clone()
    return out


def _run(mode, max_grad_norm, steps=2, overlap=False, micro=1, samples=2):
    """`steps` optimizer steps of `micro` micro-batches on one fixed batch.  -> (state, [gradients per step], [last_grad_norm per step], opt)."""
    from egoscaler_amd.optim import EgoAdamW
    m, dims = _build(mode)
    opt = EgoAdamW(m, lr=LR) if max_grad_norm is None else EgoAdamW(m, lr=LR, max_grad_norm=max_grad_norm)
    toks, masks, pts, Lp, start = _batch(dims, samples)
    per = samples // micro
    grads, norms = [], []
    torch.manual_seed(1)
    for _ in range(steps):
        for a in range(micro):
            m.accumulate_grads = a > 0
            sl = slice(a * per, (a + 1) * per)
            m.loss_and_backward(toks[sl], masks[sl], pts[sl], Lp, dims.tok.pad, fps_start=start[sl])
        m.accumulate_grads = False
        grads.append(_grads(m, opt))
        opt.step(grad_scale=1.0 / micro, overlap=overlap)
        if max_grad_norm is not None:
            norms.append(float(opt.last_grad_norm))
    return _state(m, opt), grads, norms, opt


def _initial_masters(names):
    """The fp32 masters of a fresh unfreeze_lm model, for the torch-CPU arm."""
    from egoscaler_amd.optim import EgoAdamW
    m, _ = _build("unfreeze_lm")
    return {n: st["master"].detach().cpu().clone() for n, st in EgoAdamW(m, lr=LR).state.items() if n in names}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", list(MODES))
def test_threshold_that_never_bites_changes_no_bit(mode):
    base, _, _, _ = _run(mode, None)
    got, grads, norms, opt = _run(mode, 1e30)
    assert len(base) >= 4
    _same_bits(base, got)
    for g, n in zip(grads, norms):
        ref = R.global_norm(list(g.values()), 1.0)
        assert ref > 0 and abs(n - ref) <= 2.0 ** -23 * ref, (n, ref)
    st = opt.grad_stats()
    assert (st["steps"], st["clipped_steps"], st["nonfinite_steps"]) == (2, 0, 0) and st["grad_norm_max"] == max(norms)
    assert opt.grad_stats()["steps"] == 0                                                  # the read reset the window
    per = opt.per_tensor_grad_norms()
    assert sorted(per) == sorted(grads[-1])
    for n, g in grads[-1].items():
        ref = R.global_norm([g], 1.0)
        assert abs(per[n] - ref) <= 1e-12 * ref + 1e-300, n
    assert sorted(opt.state_dict()) == ["state", "t"]


@pytest.fixture(scope="module")
def biting():
    """max_grad_norm = a tenth of the first step's norm, measured on a run WITHOUT the option by the float64 reference."""
    _, grads, _, _ = _run("unfreeze_lm", None, steps=1)
    first = R.global_norm(list(grads[0].values()), 1.0)
    mx = first / 10
    return mx, first, _run("unfreeze_lm", mx)


def test_clipping_that_bites_matches_torch(biting):
    mx, first, (state, grads, norms, opt) = biting
    init = _initial_masters(grads[0])
    ref, ref_norms = R.torch_clip_adamw(init, grads, 1.0, mx, LR)
    assert abs(norms[0] - first) <= 2.0 ** -23 * first
    for got, r in zip(norms, ref_norms):
        assert abs(got - r) <= 1e-5 * r
    for n, r in ref.items():
        got = state[f"{n}/master"].float().reshape(r.shape)
        err, scale = float((got - r).abs().max()), float(r.abs().max()) + 1e-12
        assert err <= 1e-5 * scale, (n, err, scale)                                        # close(..., 1e-5) of test_adamw_matches_torch
    st = opt.grad_stats()
    assert (st["steps"], st["clipped_steps"], st["nonfinite_steps"]) == (2, 2, 0)
    base, _, _, _ = _run("unfreeze_lm", None)
    assert any(not torch.equal(base[k], state[k]) for k in state)                          # it did bite


def test_overlap_and_repeat_are_bit_equal(biting):
    mx, _, (state, _, norms, _) = biting
    again, _, norms2, _ = _run("unfreeze_lm", mx)
    _same_bits(state, again)
    assert norms == norms2
    over, _, norms3, _ = _run("unfreeze_lm", mx, overlap=True)
    _same_bits(state, over)
    assert norms == norms3


def test_arm_returns_false_with_clipping():
    from egoscaler_amd.optim import EgoAdamW
    m, _ = _build("unfreeze_lm")
    assert EgoAdamW(m, lr=LR).arm() is True
    m.engine.layer_final_hook = None
    opt = EgoAdamW(m, lr=LR, max_grad_norm=1.0)
    assert opt.arm() is False and m.engine.layer_final_hook is None
    with pytest.raises(ValueError):
        EgoAdamW(m, lr=LR, max_grad_norm=0.0)


def test_micro_batches_are_clipped_once_on_the_accumulated_gradient():
    _, grads, _, _ = _run("unfreeze_lm", None, steps=1, micro=2, samples=4)
    first = R.global_norm(list(grads[0].values()), 0.5)
    state, grads2, norms, opt = _run("unfreeze_lm", first / 10, steps=1, micro=2, samples=4)
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads2[0][n]), n
    assert abs(norms[0] - first) <= 2.0 ** -23 * first
    st = opt.grad_stats()
    assert (st["steps"], st["clipped_steps"], st["nonfinite_steps"]) == (1, 1, 0)
    init = _initial_masters(grads[0])
    ref, _ = R.torch_clip_adamw(init, grads2, 0.5, first / 10, LR)
    for n, r in ref.items():
        got = state[f"{n}/master"].float().reshape(r.shape)
        assert float((got - r).abs().max()) <= 1e-5 * (float(r.abs().max()) + 1e-12), n
