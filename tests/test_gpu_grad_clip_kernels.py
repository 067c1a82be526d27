"""GPU: egomi_grad_sumsq, egomi_clip_scale and the device-scale AdamW entry points against tests/grad_clip_ref.py.

grad_sumsq bound, per segment and on the total: |got - ref| <= 1e-12 * ref.  All terms are non-negative, so any summation order of n float64
terms errs by at most (n - 1) * 2^-53 relative; a per-lane run of a few hundred terms plus a tree stays near 1e-14."""
import struct

import numpy as np
import pytest
import torch

from tests import grad_clip_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from egoscaler_amd import ops as O
    return O


def _vals(n, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dtype)


def _place(vals, off=0):
    """The values on the device, `off` elements into a buffer of their own: off = 1 puts an fp32 / bf16 segment off 16-B alignment."""
    buf = torch.empty(off + vals.numel(), dtype=vals.dtype, device="cuda")
    buf[off:] = vals.cuda()
    return buf[off:]


SEG = 2 << 20


def at_end(src, keep):
    """A copy of `src` whose last byte is the last byte of a fresh device allocation of its own (tests/test_gpu_bounds.py's convention): >= 16 MB
    and a multiple of 2 MB, requested from an EMPTY cache so that the allocator maps a segment of exactly that size."""
    n, es = src.numel(), src.element_size()
    nbytes = max(16 << 20, -(-n * es // SEG) * SEG)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    buf = torch.empty(nbytes // es, dtype=src.dtype, device="cuda")
    keep.append(buf)
    t = buf[buf.numel() - n:].view(src.shape)
    t.copy_(src)
    return t


def _bits(x):
    return struct.pack("<d", float(x))


def _run(ops, tensors):
    t = ops.GradTable(tensors)
    seg, tot = ops.grad_sumsq(t)
    return seg.cpu().tolist(), float(tot.cpu())


@pytest.fixture(scope="module")
def mixed(ops):
    """The mixed table (host values, device tensors), computed once."""
    ch = ops.grad_sumsq_chunk()
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, ch - 1, ch, ch + 1, 2 * ch + 7]
    host = []
    for i, n in enumerate(sizes):
        host.append(_vals(n, F32 if i % 2 == 0 else BF16, 100 + i))
        host.append(_vals(n, BF16 if i % 2 == 0 else F32, 200 + i))
    host.append(_vals((1 << 24) + 3, F32, 7))                       # stage 2 sums a few hundred partials
    host.append(_vals(5000, F32, 8, 1e18))                          # squares overflow in fp32
    host.append(_vals(5000, F32, 9, 1e-30))                         # squares vanish in fp32
    host.append(_vals(4097, BF16, 10, 1e18))
    host.append(_vals(4097, BF16, 11, 1e-30))
    dev = [_place(h) for h in host]
    ref = [R.seg_sumsq(h) for h in host]
    return host, dev, ref


def test_grad_sumsq_matches_float64_reference(ops, mixed):
    host, dev, ref = mixed
    seg, tot = _run(ops, dev)
    worst = 0.0
    for h, g, r in zip(host, seg, ref):
        assert r > 0 and np.isfinite(r)
        worst = max(worst, abs(g - r) / r)
        assert abs(g - r) <= 1e-12 * r, (h.numel(), h.dtype, g, r)
    rt = R.total_sumsq(ref)
    worst_t = abs(tot - rt) / rt
    print(f"grad_sumsq: worst |got - ref| / ref per segment {worst:.3e}, total {worst_t:.3e} (bound 1e-12; chunk {ops.grad_sumsq_chunk()})")
    assert abs(tot - rt) <= 1e-12 * rt
    f32_sq = (host[-4].float() ** 2).sum()
    assert torch.isinf(f32_sq) and float((host[-3].float() ** 2).sum()) == 0.0          # what an fp32 pass would have reported


def test_grad_sumsq_bits(ops, mixed):
    """A segment's bits: alone == in the middle of a table == 1 element off 16-B alignment; a second run; a permuted table."""
    host, dev, _ = mixed
    seg, tot = _run(ops, dev)
    seg2, tot2 = _run(ops, dev)
    assert [_bits(a) for a in seg] == [_bits(a) for a in seg2] and _bits(tot) == _bits(tot2)
    t = ops.GradTable(dev)
    for _ in range(2):                                               # the same table object, run again
        s3, t3 = ops.grad_sumsq(t)
        assert [_bits(a) for a in s3.cpu().tolist()] == [_bits(a) for a in seg] and _bits(float(t3.cpu())) == _bits(tot)
    ch = ops.grad_sumsq_chunk()
    for i, h in enumerate(host):
        if h.numel() > 2 * ch + 7:
            continue
        alone, _ = _run(ops, [dev[i]])
        assert _bits(alone[0]) == _bits(seg[i]), (i, h.numel(), h.dtype)
        shifted = _place(h, 1)
        assert shifted.data_ptr() % 16 != 0 and dev[i].data_ptr() % 16 == 0
        off, _ = _run(ops, [dev[0], shifted, dev[3]])
        assert _bits(off[1]) == _bits(seg[i]), (i, h.numel(), h.dtype)
    perm = torch.randperm(len(dev), generator=torch.Generator().manual_seed(3)).tolist()
    segp, _ = _run(ops, [dev[j] for j in perm])
    assert [_bits(a) for a in segp] == [_bits(seg[j]) for j in perm]


def test_grad_sumsq_segment_at_the_end_of_its_allocation(ops):
    """The segment ends at the last byte of a device allocation of its own, so a load past it leaves mapped memory.  The end of an allocation is
    16-B aligned, so a segment that ends there starts 16-B aligned exactly when its size is a multiple of the vector (4 fp32 / 8 bf16
    elements): those sizes take the 16-B loads up to the allocation's last 16 bytes, in one chunk, in a full chunk and in the short last
    chunk of several; every other size (one element more or fewer, among them the smallest) starts off alignment and takes the 4-B / 2-B
    loads, whose last, partly filled vector slot is the one that must not be read whole.  A 16-B body with a scalar tail cannot end at an
    allocation's end (an aligned start plus a tail ends off alignment); the mixed table covers that form.  The tables here also hold
    a second, ordinary segment before and after, so that the chunk's segment lookup is not the trivial one."""
    ch = ops.grad_sumsq_chunk()
    pad = _place(_vals(ch + 5, F32, 1))
    for dtype, V in ((F32, 4), (BF16, 8)):
        for n in (V, 1024 * V, ch, ch + V, 2 * ch + 2 * V):
            for m in (n, n - 1, n + 1):
                h = _vals(m, dtype, m)
                r = R.seg_sumsq(h)
                keep = []
                g = at_end(h, keep)
                assert g.data_ptr() + m * g.element_size() == keep[0].data_ptr() + keep[0].numel() * keep[0].element_size()
                assert (g.data_ptr() % 16 == 0) == (m == n)
                seg, _ = _run(ops, [pad, g, pad])
                assert abs(seg[1] - r) <= 1e-12 * r, (dtype, m)
                alone, tot = _run(ops, [g])
                assert _bits(alone[0]) == _bits(seg[1]) == _bits(tot), (dtype, m)
                del g, keep


def test_surplus_workgroups_change_no_bit(ops, mixed):
    """The grid: more chunks launched than the table needs (the header allows it; the surplus workgroups do nothing) gives the same bits."""
    from egoscaler_amd import _lib
    _, dev, _ = mixed
    tensors = dev[:9] + dev[-4:]
    seg, tot = _run(ops, tensors)
    t = ops.GradTable(tensors)
    for extra in (1, 300):
        n_chunks = t.n_chunks + extra
        ws_bytes = _lib.query("egomi_grad_sumsq_workspace_bytes", t.n_seg, n_chunks)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
        _lib.call("egomi_grad_sumsq", t.addr, t.numel, t.dtype, t.dtype0, t.n_seg, n_chunks, t.seg_sumsq, t.total, ws, ws_bytes, None)
        assert [_bits(a) for a in t.seg_sumsq.cpu().tolist()] == [_bits(a) for a in seg] and _bits(float(t.total.cpu())) == _bits(tot)


def _clip(ops, total, gs, mx, stats=None):
    out = torch.zeros(3, dtype=torch.float32, device="cuda")
    stats = torch.zeros(5, dtype=torch.float64, device="cuda") if stats is None else stats
    ops.clip_scale(torch.tensor([total], dtype=torch.float64, device="cuda"), gs, mx, out, stats)
    return out.cpu().numpy(), stats


def _ulps(a, b):
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def test_clip_scale(ops):
    gs = 1.0 / 3.0
    for mx in (1e3, float("inf")):                                   # below the threshold: the bits of grad_scale
        out, _ = _clip(ops, 37.5, gs, mx)
        ref = R.clip_scale(37.5, gs, mx)
        assert out[2].tobytes() == np.float32(gs).tobytes() and out[1] == 1.0 and _ulps(out[0], ref[0]) <= 1
    for total, mx in ((37.5, 1.0), (1e40, 0.3), (3e-9, 1e-7)):       # above it: within 1 fp32 ulp of the reference
        out, _ = _clip(ops, total, gs, mx)
        ref = R.clip_scale(total, gs, mx)
        assert ref[1] < 1.0
        for i in range(3):
            assert _ulps(out[i], ref[i]) <= 1, (total, mx, i, out[i], ref[i])
    out, _ = _clip(ops, float("inf"), gs, 1.0)
    assert np.isinf(out[0]) and out[1] == 0.0 and out[2] == 0.0
    out, _ = _clip(ops, float("nan"), gs, 1.0)
    assert np.isnan(out).all()


def test_clip_scale_stats(ops):
    calls = [(4.0, 1.0, 10.0), (400.0, 1.0, 10.0), (float("inf"), 1.0, 10.0), (float("nan"), 1.0, 10.0), (900.0, 0.5, 10.0), (1.0, 1.0, float("inf"))]
    stats = None
    for total, gs, mx in calls:
        _, stats = _clip(ops, total, gs, mx, stats)
    assert stats.cpu().tolist() == R.stats_after(calls) == [6.0, 2.0, 2.0, 38.0, 20.0]


def test_argument_errors(ops):
    from egoscaler_amd import _abi, _lib
    rc = lambda name, *a: getattr(_lib.lib(), name)(*_lib.marshal(name, a))
    t = ops.GradTable([torch.ones(5, device="cuda"), torch.ones(7, dtype=torch.bfloat16, device="cuda")])
    assert t.dtype is not None
    for dtype in (F32, BF16):                                        # one dtype throughout: no dtype table, the `dtype` argument is the one read
        u = ops.GradTable([torch.full((5,), 2.0, dtype=dtype, device="cuda"), torch.ones(9, dtype=dtype, device="cuda")])
        assert u.dtype is None and u.dtype0 == ops.dt(dtype)
        assert ops.grad_sumsq(u)[0].cpu().tolist() == [20.0, 9.0]
    good = [t.addr, t.numel, t.dtype, ops.F32, t.n_seg, t.n_chunks, t.seg_sumsq, t.total, t.ws, t.ws_bytes, None]

    def with_(i, v):
        a = list(good)
        a[i] = v
        return rc("egomi_grad_sumsq", *a)
    assert rc("egomi_grad_sumsq", *good) == 0
    assert t.seg_sumsq.cpu().tolist() == [5.0, 7.0]
    for i in (0, 1, 6, 7, 8):
        assert with_(i, None) == _abi.EGOMI_E_BADARG, i
    assert with_(4, 0) == _abi.EGOMI_E_SHAPE and with_(9, t.ws_bytes - 1) == _abi.EGOMI_E_SHAPE and with_(5, 0) == _abi.EGOMI_E_SHAPE
    assert with_(3, 2) == _abi.EGOMI_E_UNSUPPORTED
    out, stats, tot = torch.zeros(3, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"), torch.ones(1, dtype=torch.float64, device="cuda")
    assert rc("egomi_clip_scale", tot, 1.0, 1.0, out, stats, None) == 0
    for mx in (0.0, -1.0, float("nan")):
        assert rc("egomi_clip_scale", tot, 1.0, mx, out, stats, None) == _abi.EGOMI_E_BADARG
    assert rc("egomi_clip_scale", None, 1.0, 1.0, out, stats, None) == _abi.EGOMI_E_BADARG
    assert rc("egomi_clip_scale", tot, 1.0, 1.0, None, stats, None) == _abi.EGOMI_E_BADARG
    assert rc("egomi_clip_scale", tot, 1.0, 1.0, out, None, None) == _abi.EGOMI_E_BADARG
    torch.cuda.synchronize()
    assert float(stats[0]) == 1.0                                    # the refused calls launched nothing
    with pytest.raises(_lib.EgomiError):
        ops.GradTable([torch.ones(0, device="cuda")])                # element counts are device data: the Python side checks them
    with pytest.raises(_lib.EgomiError):
        ops.GradTable([torch.ones(4, dtype=torch.float16, device="cuda")])
    m = torch.zeros(4, device="cuda")
    assert rc("egomi_adamw_ds", m, None, m, m, m, 4, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, None, 0, None) == _abi.EGOMI_E_BADARG


def test_short_chunk_count_reports_nan_without_reading_out_of_bounds(ops):
    """n_chunks smaller than the table needs (a caller's mistake the call cannot see: the counts are device data): the segments past it and the
    total are NaN, the ones before it are right."""
    from egoscaler_amd import _lib
    ch = ops.grad_sumsq_chunk()
    h = [_vals(ch + 1, F32, 1), _vals(ch + 1, F32, 2)]
    t = ops.GradTable([_place(x) for x in h])
    assert t.n_chunks == 4
    _lib.call("egomi_grad_sumsq", t.addr, t.numel, t.dtype, t.dtype0, t.n_seg, 3, t.seg_sumsq, t.total, t.ws, t.ws_bytes, None)
    seg = t.seg_sumsq.cpu().tolist()
    r = R.seg_sumsq(h[0])
    assert abs(seg[0] - r) <= 1e-12 * r and np.isnan(seg[1]) and np.isnan(float(t.total.cpu()))


@pytest.mark.parametrize("gdtype", [F32, BF16])
@pytest.mark.parametrize("n,off", [(5003, 0), (1001, 1), (3, 0), (70000, 4)])
def test_adamw_ds_equals_host_scale(ops, n, off, gdtype):
    """The scale read from device memory: master, m, v and the bf16 copy bit-equal to ops.adamw(..., grad_scale=s), s the float read back."""
    def at(vals, dtype=F32):
        buf = torch.zeros(n + 8, dtype=dtype, device="cuda")
        buf[off:off + n] = vals.cuda().to(dtype)
        return buf[off:off + n]
    out = torch.zeros(3, dtype=torch.float32, device="cuda")
    ops.clip_scale(torch.tensor([123.456], dtype=torch.float64, device="cuda"), 0.5, 1.0, out, torch.zeros(5, dtype=torch.float64, device="cuda"))
    s = float(out[2])
    assert 0 < s < 0.5
    vals = [_vals(n, F32, k) for k in range(4)]
    outs = []
    for dev_scale in (False, True):
        master, m, v, g = at(vals[0]), at(vals[1]), at(vals[2].abs()), at(vals[3], gdtype)
        cp = at(torch.zeros(n), BF16)
        for step in (1, 2):
            if dev_scale:
                ops.adamw(master, cp, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, grad_scale_dev=out[2:3])
            else:
                ops.adamw(master, cp, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, s)
        outs.append([t.clone() for t in (master, m, v, cp)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0].cpu(), vals[0])
