"""GPU: the frozen top decoder layer on the rows the loss reads (Engine.forward_hidden(loss_from=...), engine.use_top_rows) against the
path that runs every row (use_top_rows = False: what the engine did before) and against the fp32 engine.

Bounds of the on / off comparison.  Both arms must meet the bounds of test_gpu_train_modes.py against fp32 (loss 2e-2 relative, every
trainable tensor max|g - g32| <= 0.2 max|g32| + 1e-6).  On top of that the on-arm's error against fp32 may exceed the off-arm's, per tensor
and in the same run, only by what two bf16 evaluation orders of equal quality warrant: err_on <= RATIO * err_off + FLOOR with RATIO = 2 and
FLOOR = 2^-8 * max|g32| (one bf16 ulp of the tensor's largest element) — two independent bf16 roundings of the same exact values are two
draws from one error distribution, and a factor 2 on a max-norm over a few thousand elements states "the same size of error".  RATIO and
FLOOR were fixed from this reasoning before the first run.  Measured on the first MI355X run (the test prints every tensor, -s):
err_on / err_off = 1.000 for every tensor of (a) and of both (d) cases, and the losses agree to the last digit (6.487861 on and off,
fp32 6.483644 in (a)): the arms agree bit for bit, so the margin over 1.0 is unused.  That is by construction, at the 7B shape too: the
compact products run whole 8-phase tiles whose rows keep the bits of the full products (tests/test_gpu_gemm_top_rows.py,
profiles/top_rows_ab.txt)."""
import types

import pytest
import torch

from egoscaler_amd import synth
from egoscaler_amd.config import dims_tiny

pytestmark = pytest.mark.gpu
RATIO, FLOOR = 2.0, 2.0 ** -8


def _dims(layers=None):
    d = dims_tiny()
    d.lm.hidden_size, d.lm.num_attention_heads, d.lm.intermediate_size = 256, 2, 512
    if layers is not None:
        d.lm.num_hidden_layers = layers
    return d


def _model(dims, dtype, unfreeze=False, lora_targets=None):
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


def _batch(dims, B=3):
    if B not in _BATCH:
        toks, masks, Lp = synth.synth_batch(dims, B, text_len=8, num_steps=4, max_traj_token=40)
        pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)])
        _BATCH[B] = (toks.cuda(), masks.cuda(), pts.cuda(), Lp, [0, 17, 3, 9][:B])
    return _BATCH[B]


def _step(m, batch, dims, Lp=None, masks=None):
    toks, mk, pts, Lp0, start = batch
    loss = m.loss_and_backward(toks, mk if masks is None else masks, pts, Lp0 if Lp is None else Lp, dims.tok.pad, fps_start=start)
    return float(loss), {n: p.main_grad.clone() for n, p in m.named_parameters() if getattr(p, "main_grad", None) is not None}


def _same(a, b):
    (la, ga), (lb, gb) = a, b
    assert la == lb, (la, lb)
    assert ga.keys() == gb.keys()
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def _against_fp32(dims, masks=None, tag=""):
    batch = _batch(dims)
    l32, g32 = _step(_model(dims, torch.float32), batch, dims, masks=masks)
    res = {}
    for on in (False, True):
        m = _model(dims, torch.bfloat16)
        m.engine.use_top_rows = on
        res[on] = _step(m, batch, dims, masks=masks)
        S, Lp = batch[0].shape[1], batch[3]
        assert m.engine.top_rows_taken == (S - Lp + 1 if on else 0)
    worst = 0.0
    for on in (False, True):
        l16, g16 = res[on]
        assert abs(l16 - l32) < 2e-2 * abs(l32), (on, l16, l32)
        assert g16.keys() == g32.keys()
        for n, g in g32.items():
            err = float((g16[n] - g).abs().max())
            assert err <= 0.2 * float(g.abs().max()) + 1e-6, (on, n, err, float(g.abs().max()))
    for n, g in g32.items():
        e_on, e_off = float((res[True][1][n] - g).abs().max()), float((res[False][1][n] - g).abs().max())
        worst = max(worst, e_on / max(e_off, 1e-30))
        print(f"top-rows{tag} {n}: err_on {e_on:.3e} err_off {e_off:.3e} ratio {e_on / max(e_off, 1e-30):.3f} max|g32| {float(g.abs().max()):.3e}")
        assert e_on <= RATIO * e_off + FLOOR * float(g.abs().max()), (n, e_on, e_off)
    print(f"top-rows{tag} loss on {res[True][0]:.6f} off {res[False][0]:.6f} fp32 {l32:.6f}; worst err_on / err_off {worst:.3f}")


def test_on_against_off_and_fp32():
    _against_fp32(_dims(), tag=" (a)")


def test_two_identical_steps_are_bit_identical():
    dims = _dims()
    m = _model(dims, torch.bfloat16)
    a = _step(m, _batch(dims), dims)
    assert m.engine.top_rows_taken > 0
    m.engine.zero_grad()
    _same(a, _step(m, _batch(dims), dims))


def test_a_window_that_moves_leaves_nothing_behind():
    """One engine, prompt_len = Lp, Lp + 7 (the window shrinks), Lp - 5 (it grows): each step equals a fresh engine's at that prompt_len,
    so the rows that left the window hold zeros again in the buffers that stay from step to step."""
    dims = _dims()
    batch = _batch(dims)
    Lp = batch[3]
    m = _model(dims, torch.bfloat16)
    for lp in (Lp, Lp + 7, Lp - 5):
        m.engine.zero_grad()
        got = _step(m, batch, dims, Lp=lp)
        assert m.engine.top_rows_taken == batch[0].shape[1] - lp + 1
        _same(got, _step(_model(dims, torch.bfloat16), batch, dims, Lp=lp))


def test_one_layer_model_against_off_and_fp32():
    _against_fp32(_dims(layers=1), tag=" (d, one layer)")


def test_left_padded_masks_against_off_and_fp32():
    dims = _dims()
    masks = _batch(dims)[1].clone()
    masks[1, :5] = False                                 # rows 0..4 of sample 1 see no key
    masks[2, :1] = False
    _against_fp32(dims, masks=masks, tag=" (d, left padding)")


@pytest.mark.parametrize("how", ["lora", "unfrozen"])
def test_trainable_top_layer_takes_the_full_path(how):
    dims = _dims()
    batch = _batch(dims)
    res = {}
    for on in (True, False):
        m = _model(dims, torch.bfloat16, unfreeze=how == "unfrozen", lora_targets="q_proj,v_proj" if how == "lora" else None)
        m.engine.use_top_rows = on
        res[on] = _step(m, batch, dims)
        assert m.engine.top_rows_taken == 0
    _same(res[True], res[False])
