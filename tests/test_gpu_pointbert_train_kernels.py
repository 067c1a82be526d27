"""GPU: every C-ABI entry point of csrc/pointbert_train.hip (the trainable point backbone's kernels, --unfreeze_pc_encoder) against a
float64 torch evaluation of the same op on the CPU, through the wrappers in egoscaler_amd/pointbert_train.py.  Shapes reach the
geometry `bench.py --mode pc` runs (R = 131072 BatchNorm rows, 512 partial rows per column reduction, 4104 LayerNorm rows) and
the edges around the kernels' block sizes and grid caps.  fp32: <= 1e-4 of the output scale; bf16 (inputs rounded first, the
reference works on the rounded values): <= 2e-2; indices, maxima and scatters exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
DTYPES = [torch.float32, torch.bfloat16]
DT_ID = {torch.float32: "f32", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def pt():
    assert torch.cuda.is_available()
    from egoscaler_amd import pointbert_train as T
    return T


def close(got, ref, tol, what="", scale=0.0):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item()
    scale = max(ref.abs().max().item(), scale) + 1e-12
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed, scale=1.0, dtype=torch.float32):
    """host tensor rounded to `dtype`: the reference takes exactly these values (in float64)"""
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(dtype)


def rc_of(fn, *args):
    from egoscaler_amd import _lib
    return getattr(_lib.lib(), fn)(*args)


# ------------------------------------------------------------------------------------------------ train-mode BatchNorm (+ ReLU)
def bn_reference(x, gamma, beta, rm, rv, dy, relu, eps=1e-5):
    """float64 nn.BatchNorm1d in train() mode (momentum 0.1) and its autograd: y, batch mean, rstd, running stats after, dx, dgamma, dbeta"""
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(x64, rm64, rv64, g64, b64, training=True, momentum=0.1, eps=eps)
    if relu:
        y = F.relu(y)
    y.backward(dy.double())
    xd = x.double()
    mean = xd.mean(0)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(0) + eps)
    return y.detach(), mean, rstd, rm64, rv64, x64.grad, g64.grad, b64.grad


def bn_inputs(R, C, dtype, seed, offsets=None):
    """x [R, C] with two boundary channels: channel 0 is +1 (R//4 rows), -1 (R//4 rows), 0 elsewhere — batch mean exactly 0, so with
    beta 0 the pre-ReLU value of the zero rows is exactly 0 (the `y > 0` mask at its boundary); channel 1 has gamma = beta = 0 (every
    pre-ReLU value 0).  offsets: {channel: offset in units of that channel's std}."""
    std = 0.5 + torch.rand(C, generator=gen(seed + 1))
    mu = torch.randn(C, generator=gen(seed + 2))
    x = torch.randn(R, C, generator=gen(seed)) * std + mu
    for c, k in (offsets or {}).items():
        x[:, c] += k * float(std[c])
    n = R // 4
    if n:
        x[:, 0] = 0.0
        x[:n, 0], x[n:2 * n, 0] = 1.0, -1.0
    x = x.to(dtype)
    gamma = (0.5 + torch.rand(C, generator=gen(seed + 3))).to(dtype)
    beta = (0.3 * torch.randn(C, generator=gen(seed + 4))).to(dtype)
    beta[0] = 0
    if C > 1:
        gamma[1] = beta[1] = 0
    rm = (0.2 * torch.randn(C, generator=gen(seed + 5))).to(dtype)
    rv = (0.5 + torch.rand(C, generator=gen(seed + 6))).to(dtype)
    dy = randn(R, C, seed=seed + 7, dtype=dtype)
    return x, gamma, beta, rm, rv, dy


def run_bn(pt, x, gamma, beta, rm, rv, dy, relu, y_for_bwd=None):
    """forward, then backward with the saved stats of that forward; the backward's ReLU mask reads `y_for_bwd` when given (the reference's
    y rounded to the dtype: fp32 rounding may move a pre-ReLU value within ~1e-7 of 0 to the other side, an O(1) change of dx there)"""
    R, C = x.shape
    xd = x.cuda()
    stats = torch.full((4 * C,), float("nan"), dtype=torch.float32, device="cuda")
    rmd, rvd = rm.cuda(), rv.cuda()
    y = pt.bn_train_fwd(xd, gamma.cuda(), beta.cuda(), 1e-5, relu, stats, rmd, rvd, momentum=0.1)
    dg = torch.full((C,), float("nan"), dtype=torch.float32, device="cuda")     # written by the call, not accumulated
    db = torch.full((C,), float("nan"), dtype=torch.float32, device="cuda")
    yb = y if y_for_bwd is None else y_for_bwd.to(x.dtype).cuda()
    dx = pt.bn_train_bwd(dy.cuda(), xd, yb, stats, gamma.cuda(), relu, dg, db)
    torch.cuda.synchronize()
    return y, stats, rmd, rvd, dx, dg, db


def check_bn(out, ref, dtype, C, gamma, dy):
    y, stats, rmd, rvd, dx, dg, db = out
    ry, rmean, rrstd, rrm, rrv, rdx, rdg, rdb = ref
    tol = TOL[dtype]
    # dx = gamma*rstd/R * (R*dy - dbeta - xh*dgamma) cancels to ~0 at R = 2 (two normalised values are always -1, +1): its scale is that of the terms
    dx_scale = float((gamma.double() * rrstd * dy.double()).abs().max())
    close(y, ry, tol, "y")
    close(stats[2 * C:3 * C], rmean, tol, "saved mean")
    close(stats[3 * C:], rrstd, tol, "saved rstd")
    close(rmd, rrm, tol, "running_mean")
    close(rvd, rrv, tol, "running_var (unbiased)")
    close(dx, rdx, tol, "dx", scale=dx_scale)
    close(dg, rdg, tol, "dgamma")
    close(db, rdb, tol, "dbeta")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("C", [1, 128, 257, 512])
@pytest.mark.parametrize("R", [2, 255, 256, 257, 4097, 131072])
def test_bn_train_fwd_bwd(pt, R, C, relu, dtype):
    x, gamma, beta, rm, rv, dy = bn_inputs(R, C, dtype, seed=R + 7 * C)
    ref = bn_reference(x, gamma, beta, rm, rv, dy, relu)
    out = run_bn(pt, x, gamma, beta, rm, rv, dy, relu, y_for_bwd=ref[0])
    check_bn(out, ref, dtype, C, gamma, dy)
    if R >= 4:
        zero_rows = x[:, 0] == 0                                                # pre-ReLU exactly 0 (masked, like torch's relu backward)
        assert int(zero_rows.sum()) >= R // 2 and not bool(out[0][:, 0].cpu()[zero_rows].any())
        close(out[5][:1], ref[6][:1], TOL[dtype], "dgamma of the boundary channel")
        close(out[6][:1], ref[7][:1], TOL[dtype], "dbeta of the boundary channel")


@pytest.mark.parametrize("offset", [10.0, 1e2, 1e3])
def test_bn_train_offset_channels(pt, offset):
    """Channels whose batch mean is `offset` x their spread (a conv output with a bias in front of the BatchNorm): in exact arithmetic the
    output ignores such a shift, so the kernel must meet the same fp32 bound as for centred channels.  The former sumsq/R - mean^2 form
    cancelled here (rstd 0.1 % off at 100 std, 15 % at 1000 std)."""
    R, C = 131072, 128
    offs = {c: (offset if c % 2 else -offset) for c in range(2, C, 3)}
    x, gamma, beta, rm, rv, dy = bn_inputs(R, C, torch.float32, seed=11, offsets=offs)
    for relu in (True, False):
        ref = bn_reference(x, gamma, beta, rm, rv, dy, relu)
        out = run_bn(pt, x, gamma, beta, rm, rv, dy, relu, y_for_bwd=ref[0])
        check_bn(out, ref, torch.float32, C, gamma, dy)
        cols = sorted(offs)
        close(out[1][3 * C:].cpu()[cols], ref[2][cols], 1e-4, "rstd of the offset channels alone")


def test_bn_train_refuses_short_partials(pt):
    from egoscaler_amd.ops import P, S
    from egoscaler_amd._lib import c_f, c_i, c_i64
    R, C = 1000, 8
    x = torch.zeros(R, C, device="cuda")
    g, st, part = torch.ones(C, device="cuda"), torch.zeros(4 * C, device="cuda"), torch.zeros(4 * 2 * C - 1, device="cuda")
    assert rc_of("egomi_bn_train_fwd", P(x), c_i64(R), c_i(C), P(g), P(g), c_f(1e-5), c_i(1), P(x), P(st), P(g), P(g), c_f(0.1), P(part),
                 c_i64(part.numel()), c_i(0), S()) == -1
    assert rc_of("egomi_bn_train_bwd", P(x), P(x), P(x), c_i64(R), c_i(C), P(st), P(g), c_i(1), P(g), P(g), P(x), P(part), c_i64(part.numel()),
                 c_i(0), S()) == -1


# ------------------------------------------------------------------------------------------------ LayerNorm backward
LN_MODES = [("pair", True), ("separate", False), ("swapped", True), ("dw_only", False), ("db_only", True), ("neither", False)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("cols", [96, 100, 384, 2048])
@pytest.mark.parametrize("rows", [1, 5, 66, 2052, 4104])
def test_layernorm_bwd(pt, rows, cols, dtype):
    """dx (+ dx_add) and the accumulated dw / db: back to back in one buffer (the one-pass branch), at separate addresses, db placed
    in front of dw, only one of them, neither.  rows > 2048 run the 512-block grid-stride loop."""
    eps = 1e-5
    s = rows * 31 + cols
    x = randn(rows, cols, seed=s, dtype=dtype) * 1.5 + 0.25
    x = x.to(dtype)
    w = (1.0 + 0.3 * torch.randn(cols, generator=gen(s + 1))).to(dtype)
    b = (0.2 * torch.randn(cols, generator=gen(s + 2))).to(dtype)
    dy = randn(rows, cols, seed=s + 3, dtype=dtype)
    add = randn(rows, cols, seed=s + 4, dtype=dtype, scale=0.5)
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.layer_norm(x64, (cols,), w64, b64, eps).backward(dy.double())
    pre_w = 0.5 * torch.randn(cols, generator=gen(s + 5))                       # dw / db accumulate into what is there
    pre_b = 0.5 * torch.randn(cols, generator=gen(s + 6))
    xd, wd, dyd, addd = x.cuda(), w.cuda(), dy.cuda(), add.cuda()
    tol = TOL[dtype]
    for mode, with_add in LN_MODES:
        buf = torch.full((2 * cols + 64,), float("nan"), device="cuda")
        if mode == "pair":
            dw, db = buf[:cols], buf[cols:2 * cols]
        elif mode == "swapped":
            db, dw = buf[:cols], buf[cols:2 * cols]
        elif mode == "separate":
            dw, db = buf[:cols], buf[cols + 64:2 * cols + 64]
        else:
            dw = buf[:cols] if mode == "dw_only" else None
            db = buf[:cols] if mode == "db_only" else None
        for t, pre in ((dw, pre_w), (db, pre_b)):
            if t is not None:
                t.copy_(pre)
        if mode == "pair":
            assert db.data_ptr() == dw.data_ptr() + 4 * cols
        dx = pt.layernorm_bwd(dyd, xd, wd, eps, dx_add=addd if with_add else None, dw=dw, db=db)
        torch.cuda.synchronize()
        close(dx, x64.grad + (add.double() if with_add else 0.0), tol, f"{mode}: dx")
        if dw is not None:
            close(dw, pre_w.double() + w64.grad, tol, f"{mode}: dw")
        if db is not None:
            close(db, pre_b.double() + b64.grad, tol, f"{mode}: db")
        if mode in ("dw_only", "db_only", "neither"):
            assert torch.isnan(buf[cols:]).all(), f"{mode}: wrote past the buffers it was given"
        if mode == "separate":
            assert torch.isnan(buf[cols:cols + 64]).all()


def test_layernorm_bwd_refusals(pt):
    """cols > 2048 -> EGOMI_E_SHAPE; a partials buffer shorter than min(ceil(rows / 4), 512) * 2 * cols -> EGOMI_E_BADARG"""
    from egoscaler_amd.ops import P, S
    from egoscaler_amd._lib import c_f, c_i, c_i64
    rows, cols = 4104, 2049
    x = torch.zeros(rows, cols, device="cuda")
    w, dw, part = torch.ones(cols, device="cuda"), torch.zeros(2 * cols, device="cuda"), torch.zeros(512 * 2 * 2048, device="cuda")
    assert rc_of("egomi_layernorm_bwd", P(x), P(x), P(w), P(x), P(None), P(dw), P(dw[cols:]), c_i(rows), c_i(cols), c_f(1e-5), P(part),
                 c_i64(part.numel()), c_i(0), S()) == -2
    for rows, cols in ((4104, 384), (66, 100)):
        need = min((rows + 3) // 4, 512) * 2 * cols
        x = torch.zeros(rows, cols, device="cuda")
        args = (P(x), P(x), P(w), P(torch.empty_like(x)), P(None))
        tail = (c_i(rows), c_i(cols), c_f(1e-5), P(part), c_i64(need - 1), c_i(0), S())
        assert rc_of("egomi_layernorm_bwd", *args, P(dw), P(None), *tail) == -1
        assert rc_of("egomi_layernorm_bwd", *args, P(None), P(dw), *tail) == -1
        assert rc_of("egomi_layernorm_bwd", *args, P(None), P(None), *tail) == 0       # no reduction asked for: no partials needed
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ group arg-max, its scatter, group sum
def group_input(BG, M, C, dtype, seed):
    """x [BG*M, C]: even columns from {-2, ..., 2} (ties everywhere), odd columns normal; a few all -inf columns"""
    g = gen(seed)
    x = torch.randn(BG, M, C, generator=g)
    x[:, :, 0::2] = torch.randint(-2, 3, (BG, M, (C + 1) // 2), generator=g).float()
    x[:, :, 3] = 1.0                                                            # every row of the column tied
    x[0, :, 5] = float("-inf")
    x[BG - 1, :, C - 1] = float("-inf")
    return x.to(dtype).reshape(BG * M, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("C", [40, 256, 600])
@pytest.mark.parametrize("M", [1, 16, 32])
def test_group_argmax_scatter_and_sum(pt, M, C, dtype):
    BG = 4096 if C == 256 else 37
    x = group_input(BG, M, C, dtype, seed=M * 1000 + C)
    xd = x.cuda()
    out, idx = pt.group_argmax(xd, BG, M, C)
    xv = x.view(BG, M, C)
    ref_idx = torch.from_numpy(np.argmax(xv.float().numpy(), axis=1).astype(np.int32))    # numpy: the FIRST maximum, like torch.max(dim)
    ref_max = xv.max(1)[0]
    assert torch.equal(idx.cpu(), ref_idx)
    assert torch.equal(out.cpu(), ref_max)
    assert bool((ref_idx[0, 5] == 0) and torch.isneginf(out[0, 5].cpu()))
    if M > 1:
        assert int((ref_idx > 0).sum()) > 0 and bool((ref_idx[:, 3] == 0).all())

    # scatter backward into a concat-layout view (ldx = 2C, the right half untouched), both ways
    dout = randn(BG, C, seed=M + C + 5, dtype=dtype)
    pre = randn(BG * M, 2 * C, seed=M + C + 6, dtype=dtype)
    scat = torch.zeros(BG, M, C, dtype=torch.float64)
    scat.scatter_(1, ref_idx.long()[:, None, :], dout.double()[:, None, :])
    scat = scat.reshape(BG * M, C)
    for accumulate in (False, True):
        full = pre.cuda()
        dxv = full[:, :C]
        assert dxv.stride(0) == 2 * C
        pt.group_max_bwd(dout.cuda(), idx, BG, M, C, dxv, accumulate)
        got = full.cpu()
        assert torch.equal(got[:, C:], pre[:, C:]), "wrote outside the view"
        if accumulate:
            assert torch.equal(got[:, :C], (pre[:, :C].float() + scat.float()).to(dtype))
        else:
            assert torch.equal(got[:, :C], scat.to(dtype))

    # group sum over the same concat layout: out[bg, c] = sum_m x[bg*M + m, c], c < C
    from egoscaler_amd._lib import call, c_i, c_i64
    from egoscaler_amd.ops import P, S, dt
    src = randn(BG * M, 2 * C, seed=M + C + 7, dtype=dtype)
    gs = torch.full((BG, C), float("nan"), dtype=dtype, device="cuda")
    call("egomi_group_sum", P(src.cuda()), c_i(BG), c_i(M), c_i(C), c_i64(2 * C), P(gs), c_i(dt(dtype)), S())
    close(gs, src.double()[:, :C].reshape(BG, M, C).sum(1), TOL[dtype], "group_sum")


# ------------------------------------------------------------------------------------------------ small-K weight gradient
KPAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]     # (x, dy)


@pytest.mark.parametrize("xdt,dydt", KPAIRS, ids=["x32_dy32", "x32_dy16", "x16_dy16"])
@pytest.mark.parametrize("N", [128, 300])
@pytest.mark.parametrize("K", [1, 3, 6, 8])
@pytest.mark.parametrize("R", [1, 511, 512, 513, 131072])
def test_smallk_wgrad(pt, R, K, N, xdt, dydt):
    s = R + 10 * K + N
    dy = randn(R, N, seed=s, dtype=dydt)
    x = randn(R, K, seed=s + 1, dtype=xdt)
    pre = torch.randn(N, K, generator=gen(s + 2))
    dW = pre.cuda()
    pt.smallk_wgrad(dy.cuda(), x.cuda(), dW)
    torch.cuda.synchronize()
    close(dW, pre.double() + dy.double().t() @ x.double(), TOL[dydt], "dW")


def test_smallk_wgrad_refusals(pt):
    from egoscaler_amd.ops import P, S
    from egoscaler_amd._lib import c_i, c_i64
    R, N = 600, 128
    dy32, x16 = torch.zeros(R, N, device="cuda"), torch.zeros(R, 9, dtype=torch.bfloat16, device="cuda")
    dW, part = torch.zeros(N * 9, device="cuda"), torch.zeros(2 * N * 9, device="cuda")
    assert rc_of("egomi_smallk_wgrad", P(dy32), P(x16), c_i(1), c_i64(R), c_i(N), c_i(8), P(dW), P(part), c_i64(part.numel()), c_i(0), S()) == -1
    assert rc_of("egomi_smallk_wgrad", P(dy32), P(dy32), c_i(0), c_i64(R), c_i(N), c_i(9), P(dW), P(part), c_i64(part.numel()), c_i(0), S()) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ DropPath residual
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("with_resid", [True, False], ids=["resid", "noresid"])
@pytest.mark.parametrize("rows,cols", [(513 * 3, 100), (513 * 16, 384), (5, 7)])
def test_rowscale_add(pt, rows, cols, with_resid, dtype):
    """scales 0 (dropped), 1 and 1/keep per sample of 513 rows; 513 * 16 x 384 elements pass the 8192-block grid cap"""
    rps = 513
    ns = -(-rows // rps)
    keep = 0.9
    scale = torch.tensor([(0.0, 1.0, 1.0 / keep)[i % 3] for i in range(ns)], dtype=torch.float32)
    br = randn(rows, cols, seed=rows + cols, dtype=dtype)
    res = randn(rows, cols, seed=rows + cols + 1, dtype=dtype) if with_resid else None
    out = pt.rowscale_add(res.cuda() if with_resid else None, br.cuda(), scale.cuda(), rps)
    torch.cuda.synchronize()
    per_row = scale.double().repeat_interleave(rps)[:rows, None]
    ref = per_row * br.double() + (res.double() if with_resid else 0.0)
    close(out, ref, TOL[dtype], "rowscale_add")
    if with_resid:
        dropped = per_row[:, 0] == 0
        assert torch.equal(out.cpu()[dropped], res[dropped])


# ------------------------------------------------------------------------------------------------ determinism
def test_reducing_entry_points_are_bit_replayable(pt):
    """Every reducing entry point twice at the largest shape: the same bits (ordered two-stage sums, no atomics)"""
    runs = []
    x, gamma, beta, rm, rv, dy = bn_inputs(131072, 512, torch.float32, seed=3)
    lx, lw, ldy = randn(4104, 384, seed=4), randn(384, seed=5), randn(4104, 384, seed=6)
    kdy, kx = randn(131072, 300, seed=7), randn(131072, 8, seed=8)
    gsrc = randn(4096 * 32, 512, seed=9)
    from egoscaler_amd._lib import call, c_i, c_i64
    from egoscaler_amd.ops import P, S
    for _ in range(2):
        res = list(run_bn(pt, x, gamma, beta, rm, rv, dy, True))
        dwdb = torch.zeros(2 * 384, device="cuda")
        res += [pt.layernorm_bwd(ldy.cuda(), lx.cuda(), lw.cuda(), 1e-5, dw=dwdb[:384], db=dwdb[384:]), dwdb]
        dW = torch.zeros(300, 8, device="cuda")
        pt.smallk_wgrad(kdy.cuda(), kx.cuda(), dW)
        gs = torch.empty(4096, 256, device="cuda")
        call("egomi_group_sum", P(gsrc.cuda()), c_i(4096), c_i(32), c_i(256), c_i64(512), P(gs), c_i(0), S())
        res += [dW, gs]
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in res])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i
