"""GPU, two ranks on one MI355X over gloo (the pattern of tests/test_gpu_dp.py): gradient-norm clipping under the resident bf16 exchange.
The norm is taken after the exchange on the rank-summed bf16 values both ranks hold, so both get the same coefficient with no collective
added: same last_grad_norm bits, bit-identical parameters, and the norm of the float64 reference on those values."""
import hashlib
import os

import pytest
import torch

from tests.test_gpu_dp import _batch, _build, _dims, _free_port

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from egoscaler_amd.dp import GradSync, shard_range
        from egoscaler_amd.optim import EgoAdamW
        from tests import grad_clip_ref as R
        dims = _dims()
        m = _build(dims, True)
        sync = GradSync(wire_dtype=torch.bfloat16, wire_min_bytes=1 << 16, resident=True)
        m.engine.grad_sync = sync
        toks, masks, Lp, pts, start = _batch(dims, 4)
        lo, hi = shard_range(4, rank, world)
        m.loss_and_backward(toks[lo:hi].cuda(), masks[lo:hi].cuda(), pts[lo:hi].cuda(), Lp, dims.tok.pad, fps_start=start[lo:hi])
        sync.finish()
        eng = m.engine
        names = [n for n, p in m.named_parameters() if p.requires_grad and eng.reduced_grad.get(n, eng.main_grad.get(n)) is not None]
        grads = [eng.reduced_grad.get(n, eng.main_grad.get(n)) for n in names]
        n_bf16 = sum(g.dtype == torch.bfloat16 for g in grads)
        ref = R.global_norm(grads, sync.grad_scale)                 # the reference on the rank-summed values this rank holds
        opt = EgoAdamW(m, lr=1e-3, max_grad_norm=ref / 10)          # a threshold that bites, from the reference
        armed = opt.arm(grad_scale=sync.grad_scale)
        opt.step(grad_scale=sync.grad_scale)
        norm = opt.last_grad_norm.cpu()
        st = opt.grad_stats()
        torch.cuda.synchronize()
        digest = {n: hashlib.sha256(p.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for n, p in m.named_parameters()}
        q.put((rank, norm.numpy().tobytes(), float(norm), ref, digest, st, n_bf16, armed, float(sync.grad_scale)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_clip_with_the_same_coefficient():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    a, b = res
    assert a[1] == b[1]                                              # the same last_grad_norm bits on both ranks
    assert a[4] == b[4] and len(a[4]) > 10                           # bit-identical parameters after the clipped step
    assert a[3] == b[3]                                              # (both ranks hold the same reduced values)
    for r in res:
        assert r[3] > 0 and abs(r[2] - r[3]) <= 2.0 ** -23 * r[3], (r[2], r[3])
        assert (r[5]["steps"], r[5]["clipped_steps"], r[5]["nonfinite_steps"]) == (1, 1, 0)
        assert r[6] >= _dims().lm.num_hidden_layers and r[7] is False and r[8] == 0.5
