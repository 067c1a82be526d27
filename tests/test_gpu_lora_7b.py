"""GPU: LoRA at LLaMA-7B width (d=4096, ffn=11008, H=32), the bench's batch geometry (B=8, S=692 -> M=5536), two decoder layers, bf16 —
against the CPU oracle in fp32 on the same bf16-rounded weights, with every adapted projection replaced by W + s B A and A, B autograd
leaves (oracle/ unchanged).  This is where the engine issues the bf16 MFMA lora_down, the interleaved-32 gate|up adapters next to the
8-phase products and the K-sliced dgrads.  Bounds are those of test_gpu_parity_7b.py.  Also: fresh adapters (B = 0) leave the loss where
the frozen model has it."""
import copy
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import lora, synth
from egoscaler_amd.config import dims_7b

pytestmark = pytest.mark.gpu

B, TEXT, STEPS, MAXT, LAYERS, R = 8, 16, 20, 160, 2, 16
FRO_TOL, MAX_TOL, LOSS_TOL = 2.5e-2, 4e-2, 5e-4
ALL7 = ",".join(lora.TARGETS)


def _dims():
    d = dims_7b()
    d.lm.num_hidden_layers = LAYERS
    return d


@pytest.fixture(scope="module")
def inputs():
    dims = _dims()
    toks, masks, Lp = synth.synth_batch(dims, B, text_len=TEXT, num_steps=STEPS, max_traj_token=MAXT)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)])
    start = np.arange(B) * 13 % dims.pb.npoints
    sd = synth.synth_state_dict(dims, 0)
    sd = {k: (v.to(torch.bfloat16) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    return dims, toks, masks, Lp, pts, start, sd


def _model(dims, sd, targets, fresh=False):
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None,
                                 lora_r=R if targets else 0, lora_alpha=32, lora_target_modules=targets)
    m = TrajPointLLMForCausalLM(args, copy.deepcopy(dims), None, device="cuda", dtype=torch.bfloat16)
    m.load_state_dict(sd, strict=not targets)
    if targets and not fresh:
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("lora_B.weight"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
        m.load_state_dict(m.state_dict())
    return m.train()


def _errs(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30)), float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize("targets", ["q_proj,v_proj", ALL7], ids=["qv", "all7"])
def test_bf16_7b_width_lora_step_matches_fp32_oracle(inputs, targets):
    from oracle import pointllm as OPL, llama as OL
    dims, toks, masks, Lp, pts, start, sd = inputs
    m = _model(dims, sd, targets)
    loss = m.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
    params = dict(m.named_parameters())
    watch = [n for n in params if lora.is_adapter(n)] + ["model.point_proj.4.weight", "model.embed_tokens.weight", "lm_head.weight"]
    got = {n: params[n].main_grad.detach().float().cpu() for n in watch}
    cfg = m.lora_cfg
    ref_sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    del m
    torch.cuda.empty_cache()
    leaves = {n: ref_sd[n].clone().requires_grad_(True) for n in watch}
    use = {k: leaves.get(k, v) for k, v in ref_sd.items() if not lora.is_adapter(k)}
    for l in range(LAYERS):
        for t in cfg.targets:
            a, b = lora.adapter_names(l, t)
            use[lora.base_name(l, t)] = ref_sd[lora.base_name(l, t)] + cfg.scale * leaves[b] @ leaves[a]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    lo = OL.traj_loss(OPL.forward(use, dims, toks, masks, pts, start), toks, Lp, dims.tok.pad)
    lo.backward()
    assert abs(float(loss) - float(lo)) < LOSS_TOL * abs(float(lo)), (float(loss), float(lo))
    for n in watch:
        fro, mx = _errs(got[n], leaves[n].grad)
        assert fro < FRO_TOL and mx < MAX_TOL, (n, fro, mx)


def test_fresh_adapters_at_7b_width_leave_the_loss(inputs):
    dims, toks, masks, Lp, pts, start, sd = inputs
    args = (toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad)
    m = _model(dims, sd, ALL7, fresh=True)
    assert all(float(p.abs().max()) == 0 for n, p in m.named_parameters() if n.endswith("lora_B.weight"))
    l1 = float(m.loss_and_backward(*args, fps_start=start))
    del m
    torch.cuda.empty_cache()
    l0 = float(_model(dims, sd, None).loss_and_backward(*args, fps_start=start))
    assert abs(l1 - l0) < 2e-3 * abs(l0), (l1, l0)        # only the summation order differs: no tail fusion / SwiGLU epilogue on adapted products
