"""GPU, two ranks on one MI355X over gloo (the test_gpu_dp.py pattern) with LoRA adapters on all seven projections of a frozen LLM: both
ranks start from the same adapters, the adapter gradients travel in their decoder layer's bucket (packed and resident exchanges), the
exchanged gradient equals the single-process gradient of the whole batch, and the replicas stay bit-identical after the step."""
import os
import socket
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import lora

pytestmark = pytest.mark.gpu
ALL7 = ",".join(lora.TARGETS)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dims():
    from egoscaler_amd.config import dims_tiny
    d = dims_tiny()
    d.lm.hidden_size, d.lm.num_attention_heads, d.lm.intermediate_size = 256, 2, 512
    return d


def _build(dims):
    from egoscaler_amd import synth
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None,
                                 lora_r=8, lora_alpha=16, lora_target_modules=ALL7)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.bfloat16)
    sd = synth.synth_state_dict(dims, 0)
    m.load_state_dict({k: (v.to(torch.bfloat16) if v.dtype.is_floating_point else v) for k, v in sd.items()}, strict=False)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B.weight"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    m.load_state_dict(m.state_dict())
    return m.train()


def _batch(dims, n):
    from egoscaler_amd import synth
    toks, masks, Lp = synth.synth_batch(dims, n, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(n)])
    return toks, masks, Lp, pts, [0, 17, 3, 9][:n]


NAMES = [lora.adapter_names(l, t)[i] for l in (0, 1) for t in ("q_proj", "v_proj", "gate_proj", "up_proj", "down_proj") for i in (0, 1)] + \
        ["lm_head.weight", "model.point_proj.0.weight"]


def _worker(rank, world, port, wire, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from egoscaler_amd.dp import GradSync, shard_range
        from egoscaler_amd.optim import EgoAdamW
        dims = _dims()
        m = _build(dims)
        a0 = {n: p.detach().float().cpu().numpy() for n, p in m.named_parameters() if n.endswith("lora_A.weight")}
        opt = EgoAdamW(m, lr=1e-3)
        sync = GradSync(wire_dtype=torch.bfloat16 if wire else None, wire_min_bytes=1 << 10, resident=(wire == "resident"))
        m.engine.grad_sync = sync
        toks, masks, Lp, pts, start = _batch(dims, 4)
        lo, hi = shard_range(4, rank, world)
        loss = m.loss_and_backward(toks[lo:hi].cuda(), masks[lo:hi].cuda(), pts[lo:hi].cuda(), Lp, dims.tok.pad, fps_start=start[lo:hi])
        sync.finish()
        grads = {n: (m.engine.reduced_grad.get(n, m.engine.main_grad[n]).float() * sync.grad_scale).cpu().numpy() for n in NAMES}
        opt.step(grad_scale=sync.grad_scale)
        w = {n: dict(m.named_parameters())[n].detach().float().cpu().numpy() for n in NAMES}
        q.put((rank, float(loss), grads, w, dict(sync.stats), a0))
    finally:
        dist.destroy_process_group()


def _two_ranks(wire):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, wire, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(300)
@pytest.mark.parametrize("wire", [False, "resident"])
def test_lora_two_ranks_match_single_process_full_batch(wire):
    res = _two_ranks(wire)
    for n, a in res[0][5].items():
        assert np.array_equal(a, res[1][5][n]), n                                           # identical adapters on every rank at the start
    dims = _dims()
    m = _build(dims)
    toks, masks, Lp, pts, start = _batch(dims, 4)
    loss = m.loss_and_backward(toks.cuda(), masks.cuda(), pts.cuda(), Lp, dims.tok.pad, fps_start=start)
    assert abs(0.5 * (res[0][1] + res[1][1]) - float(loss)) < 2e-2 * abs(float(loss))
    for n, g0 in res[0][2].items():
        ref = m.engine.main_grad[n].float().cpu().numpy()
        assert float(np.abs(ref).max()) > 0, n
        tol = (3e-2 if wire else 2e-2) * float(np.abs(ref).max()) + 1e-6
        assert float(np.abs(g0 - ref).max()) <= tol, n                                       # DP mean gradient == full-batch gradient
        assert np.array_equal(g0, res[1][2][n]), n                                          # both ranks hold the same reduced gradient
        assert np.array_equal(res[0][3][n], res[1][3][n]), n                                # ... and the same weights after the step
    st = res[0][4]
    assert st["buckets"] == 1 + dims.lm.num_hidden_layers + 1, st                          # lm_head, one per decoder layer (adapters), the rest
    if wire == "resident":
        assert st.get("resident_buckets") == dims.lm.num_hidden_layers, st                  # the adapters' layer buckets are wire buffers
