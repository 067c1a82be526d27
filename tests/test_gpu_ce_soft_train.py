"""GPU: the bin-aware loss through the training step (loss_and_backward(bin_soft=...)) and the driver (--bin_sigma), tiny model.

fp32: the fused path against autograd -- model.forward() logits through the float64 soft cross-entropy of tests/ce_soft_ref.py, then
.backward() -- on the loss, last_nll and every trainable gradient.  Tolerance: the same test runs the same comparison for the hard loss
(bin_soft=None against F.cross_entropy on forward()), on code that exists without this feature; the soft comparison may show 4x the
relative Frobenius error found there, per tensor (the project's usual margin for another box's expf).  Both are printed.  For the two
scalars a hard error that happens to be near zero would ask the impossible, so they get the kernel's own per-row bound on top:
|got - ref| <= 4 e_hard |ref| + BOUND (1 + |ref|) (tests/ce_soft_ref.py: every row's loss meets BOUND (1 + |row|), and so does their mean)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from egoscaler_amd import synth, traj
from egoscaler_amd.config import dims_tiny
from tests import ce_soft_ref as C

pytestmark = pytest.mark.gpu
VOCAB = 326                                                              # even, no multiple of 64: the bf16 logits buffer has 58 pad columns


def _dims():
    d = dims_tiny(vocab=VOCAB, num_bins=64)
    d.lm.hidden_size, d.lm.num_attention_heads, d.lm.intermediate_size = 256, 2, 512
    return d


def _model(dims, dtype, unfreeze=True, lora_targets=None):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=unfreeze, num_bins=dims.tok.num_bins, model_name=None)
    if lora_targets:
        args.lora_r, args.lora_alpha, args.lora_target_modules = 8, 16.0, lora_targets
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    sd = synth.synth_state_dict(dims, 0)
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}, strict=not lora_targets)
    if lora_targets:
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("lora_B.weight"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
        m.load_state_dict(m.state_dict())
    m.train()
    return m


_BATCH = {}


def _batch(dims, B=4):
    if B not in _BATCH:
        toks, masks, Lp = synth.synth_batch(dims, B, text_len=8, num_steps=4, max_traj_token=40)
        pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)])
        _BATCH[B] = (toks.cuda(), masks.cuda(), pts.cuda(), Lp, [0, 17, 3, 9][:B])
    return _BATCH[B]


def _grads(m):
    return {n: p.grad.detach().double().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _fused(m, dims, batch, main=False, **kw):
    """main=True: the engine's fp32 main_grad buffers (where the bf16 step leaves its gradients) instead of p.grad."""
    toks, mk, pts, Lp, start = batch
    _clear(m)
    loss = m.loss_and_backward(toks, mk, pts, Lp, dims.tok.pad, fps_start=start, **kw)
    if main:
        return float(loss), {n: p.main_grad.clone() for n, p in m.named_parameters() if getattr(p, "main_grad", None) is not None}
    return float(loss), _grads(m)


def _autograd(m, dims, batch, spec):
    toks, mk, pts, Lp, start = batch
    _clear(m)
    out = m(input_ids=toks, attention_mask=mk, point_clouds=pts, fps_start=start, return_dict=True)
    logits = out.logits[:, Lp - 1:-1, :]
    logits, tgt = logits.reshape(-1, logits.shape[-1]), toks[:, Lp:].flatten()
    if spec is None:
        loss = hard = F.cross_entropy(logits.double(), tgt, ignore_index=dims.tok.pad)
    else:
        loss, hard = C.torch_soft_ce(logits, tgt, dims.tok.pad, spec)
    loss.backward()
    return float(loss.detach()), float(hard.detach()), _grads(m)


def _fro(a, b):
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())


@pytest.mark.parametrize("how", ["unfrozen", "lora"])
def test_fp32_fused_soft_step_against_autograd(how):
    dims = _dims()
    batch = _batch(dims)
    m = _model(dims, torch.float32, unfreeze=how == "unfrozen", lora_targets="q_proj,v_proj" if how == "lora" else None)
    spec = traj.soft_target_spec(dims.tok, 1.0)
    tg = batch[0][:, batch[3]:]
    assert int(((tg >= spec.p0) & (tg < spec.p0 + spec.nb)).sum()) > 20 and int((tg == dims.tok.tsep).sum()) > 0      # bins and specials among the targets
    lh, gh = _fused(m, dims, batch)
    rh, _, ah = _autograd(m, dims, batch, None)
    ls, gs = _fused(m, dims, batch, bin_soft=spec)
    nll = float(m.last_nll)
    rs, rhard, as_ = _autograd(m, dims, batch, spec)
    assert gh.keys() == ah.keys() == gs.keys() == as_.keys() and len(gs) >= 4
    e_loss = abs(lh - rh) / abs(rh)
    tol = lambda ref: 4 * e_loss * abs(ref) + C.BOUND * (1 + abs(ref))
    print(f"ce_soft train {how}: hard loss {lh:.7f} vs autograd {rh:.7f} (rel {e_loss:.2e}); soft {ls:.7f} vs {rs:.7f} (rel {abs(ls - rs) / abs(rs):.2e}); "
          f"last_nll {nll:.7f} vs {rhard:.7f}")
    worst = 0.0
    for n in gs:
        eh, es = _fro(gh[n], ah[n]), _fro(gs[n], as_[n])
        worst = max(worst, es / eh if eh > 0 else float("inf") if es > 0 else 0.0)
        print(f"ce_soft train {how}: {n}: relative Frobenius error hard {eh:.3e} soft {es:.3e}")
    print(f"ce_soft train {how}: worst soft / hard error ratio {worst:.3f} (allowed 4)")
    assert abs(ls - rs) <= tol(rs), (ls, rs, e_loss)
    assert abs(nll - rhard) <= tol(rhard) and abs(nll - lh) <= 1e-5 * abs(lh), (nll, rhard, lh)      # the hard loss of the same logits
    assert abs(ls - lh) > 1e-3 * abs(lh)                                  # and the soft loss is another number
    for n in gs:
        assert _fro(gs[n], as_[n]) <= 4 * _fro(gh[n], ah[n]), n
    if how == "lora":
        assert any("lora_A" in n for n in gs) and not any(n.endswith("q_proj.weight") for n in gs)


def test_bf16_soft_step_tracks_fp32_and_keeps_the_pad_columns_zero():
    dims = _dims()
    batch = _batch(dims)
    spec = traj.soft_target_spec(dims.tok, 1.0)
    l32, _ = _fused(_model(dims, torch.float32), dims, batch, bin_soft=spec)
    m = _model(dims, torch.bfloat16)
    seen, logits = [], m.engine.logits

    def spy(*a, **kw):
        seen.append(logits(*a, **kw))
        return seen[-1]
    m.engine.logits = spy
    l16, g16 = _fused(m, dims, batch, main=True, bin_soft=spec)
    assert abs(l16 - l32) < 2e-2 * abs(l32), (l16, l32)                   # tests/test_gpu_train_modes.py's tolerance for l16 against l32
    assert len(g16) >= 4 and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in g16.values())
    assert np.isfinite(float(m.last_nll)) and m.last_nll.dtype == torch.float32 and m.last_nll.is_cuda and m.last_nll.dim() == 0
    (lg,) = seen
    buf = lg._base
    assert buf is not None and buf.shape[1] == 384 and lg.shape[1] == VOCAB
    assert not bool(buf[:, VOCAB:].any())                                 # still the zeros the lm_head data gradient reduces over
    assert float(lg.float().abs().max()) < 1.0                            # the buffer now holds gradients, not logits


def test_none_is_the_call_without_the_argument_and_nb1_is_the_hard_loss():
    dims = _dims()
    batch = _batch(dims)
    for dtype in (torch.float32, torch.bfloat16):
        m = _model(dims, dtype)
        la, ga = _fused(m, dims, batch, main=True)
        lb, gb = _fused(m, dims, batch, main=True, bin_soft=None)
        assert la == lb and ga.keys() == gb.keys() and len(ga) >= 4 and m.last_nll is None
        for n in ga:
            assert torch.equal(ga[n], gb[n]), (dtype, n)
        one = traj.SoftTargetSpec(dims.tok.p0 + 5, 1, 1.0, 3)
        lc, gc = _fused(m, dims, batch, main=True, bin_soft=one)
        assert lc == float(m.last_nll) and abs(lc - la) <= 1e-5 * abs(la), (lc, float(m.last_nll), la)


def test_two_accumulated_micro_batches_equal_one_batch():
    dims = _dims()
    toks, mk, pts, Lp, start = _batch(dims)
    spec = traj.soft_target_spec(dims.tok, 2.5, 4)
    m = _model(dims, torch.float32)
    call = lambda s: m.loss_and_backward(toks[s], mk[s], pts[s], Lp, dims.tok.pad, fps_start=start[s], bin_soft=spec)
    lw = float(call(slice(0, 4)))
    g1 = {n: g.clone() for n, g in m.engine.main_grad.items()}
    assert int((toks[:2, Lp:] != dims.tok.pad).sum()) == int((toks[2:, Lp:] != dims.tok.pad).sum())      # equal token counts: means add up
    la = float(call(slice(0, 2)))
    m.accumulate_grads = True
    lb = float(call(slice(2, 4)))
    m.accumulate_grads = False
    assert abs(0.5 * (la + lb) - lw) <= 1e-5 * abs(lw)
    for n in ("lm_head.weight", "model.point_proj.4.weight", "model.layers.0.self_attn.q_proj.weight"):
        a, ref = m.engine.main_grad[n] * 0.5, g1[n]
        assert float((a - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-8, n       # tests/test_gpu_driver.py's fp32 tolerance


def _setup(tmp, epochs=3, **kw):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dims = dims_tiny(vocab=320, num_bins=64)
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=True, num_bins=64, model_name=None,
                                 max_traj_token=48, num_steps=5, epochs=epochs, bs=4, lr_llm=3e-3, resume=False, out_dir=str(tmp),
                                 checkpoint_dir=str(tmp), val_batches=1, val_sample=False, grad_accum_steps=1, **kw)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.float32)
    m.load_state_dict(synth.synth_state_dict(dims, 0))
    return dims, args, m


def test_driver_trains_with_bin_sigma_and_without_it_keeps_the_record(tmp_path):
    from egoscaler_amd.driver import SyntheticTrajData, parse_args, train
    dev = torch.device("cuda")
    dims, args, model = _setup(tmp_path / "soft", bin_sigma=1.0, bin_radius=None)
    tr = SyntheticTrajData(dims, 16, frames=2, size=32, text_len=8, num_steps=5)
    steps = []
    hist = train(args, model, tr, None, dev, log=lambda s: None, step_log=steps.append)
    assert len(hist) == 3
    for h in hist:
        assert set(h) == {"epoch", "train_loss", "global_step", "learning_rate", "train_nll", "bin_sigma", "bin_radius"}
        assert h["bin_sigma"] == 1.0 and h["bin_radius"] == 3 and np.isfinite(h["train_loss"]) and h["train_loss"] != h["train_nll"]
    assert hist[-1]["train_nll"] < hist[0]["train_nll"] and hist[-1]["train_loss"] < hist[0]["train_loss"], hist
    assert len(steps) == 12 and all(set(s) == {"epoch", "step", "learning_rate", "loss", "nll"} and np.isfinite(s["nll"]) for s in steps)
    assert abs(np.mean([s["nll"] for s in steps[:4]]) - hist[0]["train_nll"]) <= 1e-5 * hist[0]["train_nll"]
    # the checkpoint round trip: a fresh model resumes at epoch 3 from where this one stopped
    ck = torch.load(os.path.join(tmp_path / "soft", "latest_model.pt"), map_location="cpu", weights_only=True)
    assert ck["epoch"] == 2 and ck["global_step"] == 12
    _, args2, model2 = _setup(tmp_path / "soft", epochs=4, bin_sigma=1.0, bin_radius=None)
    args2.resume = True
    hist2 = train(args2, model2, tr, None, dev, log=lambda s: None)
    assert [h["epoch"] for h in hist2] == [3] and hist2[0]["train_nll"] < hist[0]["train_nll"], (hist, hist2)
    # without the flag: the record and the step log have exactly the keys they had before the option existed
    for kw in ({}, {"bin_sigma": 0.0, "bin_radius": None}):
        _, args3, model3 = _setup(tmp_path / f"hard{len(kw)}", epochs=1, **kw)
        steps3 = []
        hist3 = train(args3, model3, tr, None, dev, log=lambda s: None, step_log=steps3.append)
        assert set(hist3[0]) == {"epoch", "train_loss", "global_step", "learning_rate"}
        assert all(set(s) == {"epoch", "step", "learning_rate", "loss"} for s in steps3) and model3.last_nll is None
    for bad in (["--bin_sigma", "-0.5"], ["--bin_sigma", "nan"], ["--bin_sigma", "inf"], ["--bin_sigma", "1", "--bin_radius", "0"],
                ["--bin_sigma", "1", "--bin_radius", "33"]):
        with pytest.raises(SystemExit):
            parse_args(["train", "--tiny"] + bad)
