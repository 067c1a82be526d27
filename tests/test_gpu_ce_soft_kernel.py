"""GPU: egomi_ce_soft_fwd_bwd (csrc/elementwise.hip) alone, through the C-ABI, against the float64 statement of tests/ce_soft_ref.py on
the values it receives.  The bounds are that file's (derived there, term by term); every case prints its worst error / bound per output
before it asserts, and every element of every row is compared.

A case lays R rows of stride ld between one sentinel row before and one after.  Out of place: the logits' pad columns hold NaN, the
gradient buffer is pre-filled with a sentinel.  In place: the pad columns hold the sentinel.  Every case checks, besides the bounds: in
place == out of place bit for bit, a second launch == the first, pad columns / sentinel rows / the out-of-place logits keep their bits,
ignored rows give exact zeros, loss_sum and nll_sum against the float64 sum of the kernel's own rows.
Rows cycle through CONTENTS x TARGETS (a case with R = 130 holds every pair of them).

Worst error / bound seen on the MI355X over every case below (the bounds were fixed before; these are a record, not their source):
row_loss 0.31, row_nll 0.32, gradient 0.33 with an fp32 output and 0.995 with a bf16 output (there the bound is half a bf16 spacing, which
a correctly rounded value reaches), loss_sum 0.12, nll_sum 0.14."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib, ops
from egoscaler_amd.ops import P, S, dt
from tests import ce_soft_ref as C
from tests.test_gpu_logprob_kernel import at_end

pytestmark = pytest.mark.gpu
c_i, c_i64, c_f, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
OK, BADARG, SHAPE, UNSUPPORTED = 0, -1, -2, -4
SENTINEL = 7.0
PAD = 58                                                                 # ld = V + PAD: an even number of elements that shifts every row's 16-byte phase
CONTENTS = ("gauss", "peak_tgt", "peak_nbr", "peak_out", "offset", "inf_out", "inf_nbr")
TARGETS = ("first", "last", "middle", "near_lo", "near_hi", "below", "above", "text0", "ignored", "negative", "too_big", "random_bin", "vlast")


def raw(lg, ld, tg, R, V, ignore, count, p0, nb, sigma, radius, loss_sum, nll_sum, row_loss, row_nll, dlg, ldd, gs, dtype):
    fn = _lib.lib().egomi_ce_soft_fwd_bwd
    ptr = lambda t: t if isinstance(t, c_p) else P(t)
    return fn(ptr(lg), c_i64(ld), ptr(tg), c_i(R), c_i(V), c_i64(ignore), ptr(count), c_i(p0), c_i(nb), c_f(sigma), c_i(radius), ptr(loss_sum),
              ptr(nll_sum), ptr(row_loss), ptr(row_nll), ptr(dlg), c_i64(ldd), c_f(gs), c_i(dtype), S())


def make_case(R, V, p0, nb, W, dtype, seed=0, first=0):
    """-> (x [R, V] CPU tensor of dtype, targets int64 [R], ignore id).  Row r: content CONTENTS[(first + r) % 7], target TARGETS[((first + r) // 7) % 13]."""
    g = np.random.default_rng(1000 * seed + 7 * V + R + 31 * first + nb)
    ignore = V - 1 if p0 + nb < V else (0 if p0 > 0 else -100)           # the pad id: an id outside the bin window where there is one
    x = g.normal(0.0, 3.0, (R, V))
    tg = np.zeros(R, dtype=np.int64)
    for r in range(R):
        content, kind = CONTENTS[(first + r) % len(CONTENTS)], TARGETS[((first + r) // len(CONTENTS)) % len(TARGETS)]
        out = [c for c in (0, p0 - 1, p0 + nb, V - 2) if 0 <= c < V and not p0 <= c < p0 + nb and c != ignore]
        t = {"first": p0, "last": p0 + nb - 1, "middle": p0 + nb // 2, "near_lo": p0 + min(nb - 1, max(1, W - 1)),
             "near_hi": p0 + max(0, nb - 1 - max(1, W - 1)), "below": out[min(1, len(out) - 1)] if out else p0, "above": out[-1] if out else p0,
             "text0": out[0] if out else p0, "ignored": ignore, "negative": -3, "too_big": V + 5, "random_bin": p0 + int(g.integers(0, nb)),
             "vlast": V - 1}[kind]
        tg[r] = t
        tc = min(max(t, 0), V - 1)
        nbr = tc + 1 if tc + 1 < min(V, p0 + nb) else tc - 1              # a neighbour inside the window where the target is a bin
        nbr = min(max(nbr, 0), V - 1)
        far = np.nonzero(np.abs(np.arange(V) - tc) > W + 1)[0]
        if content == "peak_tgt":
            x[r, tc] = x[r].max() + 80.0
        elif content == "peak_nbr":
            x[r, nbr] = x[r].max() + 80.0
        elif content == "peak_out" and len(far):
            x[r, far[int(g.integers(0, len(far)))]] = x[r].max() + 80.0
        elif content == "offset":
            x[r] += 100.0
        elif content == "inf_out" and len(far):
            x[r, far] = np.where(g.random(len(far)) < 0.5, -np.inf, x[r, far])
        elif content == "inf_nbr" and V > 1 and nbr != tc:
            x[r, nbr] = -np.inf                                           # under q > 0 when the target is a bin with a neighbour
    return torch.from_numpy(x).to(dtype), torch.from_numpy(tg), ignore


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def framed(x, ld, pad_value, keep=None):
    """x [R, V] -> (buffer [R + 2, ld] on the device: sentinel rows around, `pad_value` in the pad columns; its view of the R rows)."""
    R, V = x.shape
    full = torch.full((R + 2, ld), SENTINEL, dtype=x.dtype)
    full[1:R + 1, V:] = pad_value
    full[1:R + 1, :V] = x
    d = full.cuda() if keep is None else at_end(full.cuda(), keep)
    return d, d[1:R + 1, :V]


class Out:
    def __init__(self, R):
        self.sums = torch.zeros(2, dtype=torch.float32, device="cuda")
        self.rows = torch.full((2, R + 2), SENTINEL, dtype=torch.float32, device="cuda")

    def args(self):
        return self.sums[0:1], self.sums[1:2], self.rows[0, 1:-1], self.rows[1, 1:-1]


def launch(lg, tg, ignore, count, spec, out, dlg, gs):
    R, V = lg.shape
    rc = raw(lg, lg.stride(0), tg, R, V, ignore, count, *spec, *out.args(), dlg, dlg.stride(0) if dlg is not None else 0, gs, dt(lg.dtype))
    assert rc == OK, rc


def check(x, tg, ignore, spec, ld, gs, tag, worst, keep=None, count=None):
    R, V = x.shape
    dtype = x.dtype
    tgd = tg.cuda()
    n = max(1, int((tg != ignore).sum())) if count is None else count     # (a case whose only row is ignored: any count will do)
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    x64 = x.to(torch.float64).numpy()
    ref = C.soft_ce(x64, tg.numpy(), ignore, spec, grad_scale=gs, count=n)
    # out of place
    lbuf, lg = framed(x, ld, float("nan"), keep)
    before = bits(lbuf).clone()
    dbuf = torch.full((R + 2, ld), SENTINEL, dtype=dtype, device="cuda")
    o1 = Out(R)
    launch(lg, tgd, ignore, cnt, spec, o1, dbuf[1:R + 1, :V], gs)
    # in place, twice over fresh copies (the second launch must give the first one's bits)
    ins = []
    for _ in range(2):
        ibuf, ilg = framed(x, ld, SENTINEL, keep)
        o = Out(R)
        launch(ilg, tgd, ignore, cnt, spec, o, ilg, gs)
        ins.append((ibuf, o))
    torch.cuda.synchronize()
    assert torch.equal(bits(lbuf), before), tag                          # the logits, their NaN pads and sentinel rows
    frame = torch.full((R + 2, ld), SENTINEL, dtype=dtype, device="cuda")
    for buf in (dbuf, ins[0][0], ins[1][0]):
        assert torch.equal(bits(buf[:, V:]), bits(frame[:, V:])) and torch.equal(bits(buf[0]), bits(frame[0])) and torch.equal(bits(buf[-1]), bits(frame[-1])), tag
    for ibuf, o in ins:
        assert torch.equal(bits(ibuf[1:R + 1, :V]), bits(dbuf[1:R + 1, :V])), tag
        assert torch.equal(bits(o.rows), bits(o1.rows)) and torch.equal(bits(o.sums), bits(o1.sums)), tag
    assert bool((o1.rows[:, 0] == SENTINEL).all()) and bool((o1.rows[:, -1] == SENTINEL).all())
    got_loss, got_nll = o1.rows[0, 1:-1].cpu().numpy(), o1.rows[1, 1:-1].cpu().numpy()
    got_grad = dbuf[1:R + 1, :V].to(torch.float64).cpu().numpy()
    ign = ~ref["keep"]
    assert not got_loss[ign].any() and not got_nll[ign].any() and not got_grad[ign].any(), tag
    r = {"row_loss": C.loss_ratio(got_loss, ref["row_loss"]), "row_nll": C.loss_ratio(got_nll, ref["row_nll"]),
         "grad": C.grad_ratio(got_grad, x64, ref, dtype == torch.bfloat16)}
    sums = o1.sums.cpu().numpy().astype(np.float64)
    for name, got_rows, s in (("loss_sum", got_loss, sums[0]), ("nll_sum", got_nll, sums[1])):
        exact = float(got_rows.astype(np.float64).sum())
        if np.isfinite(exact):
            b = C.sum_bound(got_rows)
            r[name] = abs(s - exact) / b if b > 0 else (0.0 if s == exact else np.inf)
        else:
            r[name] = 0.0 if s == exact else np.inf
    print(f"ce_soft {tag}: worst error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        if v > worst.get(k, (0.0, ""))[0]:
            worst[k] = (v, tag)
    for k, v in r.items():
        assert v <= 1.0, (tag, k, v)


def specs(V):
    """(p0, nb) per V: the window in the row's middle, and ending with the row (the 7B layout in fp32: the next row follows at once)."""
    if V == 16:
        return [(4, 1), (3, 7), (9, 7), (0, 16)]
    if V == 300:
        return [(40, 1), (150, 7), (40, 256), (44, 256)]
    return [(V - 256, 256)]


SIGMAS = [(s, w) for s in (0.5, 1.0, 2.5) for w in (1, C.default_radius(s), 32)]


@pytest.mark.parametrize("V", [16, 300])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_small_rows_against_float64(dtype, V):
    worst, k = {}, 0
    for (p0, nb), (sigma, W), gs in itertools.product(specs(V), SIGMAS, (1.0, 0.37)):
        R, ld = ((130, V + PAD), (130, V), (3, V), (1, V + PAD), (3, V + PAD), (1, V))[k % 6]
        first = 0 if R == 130 else 7 * k
        k += 1
        x, tg, ignore = make_case(R, V, p0, nb, W, dtype, seed=k, first=first)
        check(x, tg, ignore, (p0, nb, sigma, W), ld, gs, f"{dtype} V={V} R={R} ld={ld} p0={p0} nb={nb} sigma={sigma} W={W} gs={gs}", worst)
    for name, (v, tag) in worst.items():
        print(f"ce_soft {dtype} V={V}: worst {name} error / bound {v:.3f} at {tag}")


@pytest.mark.parametrize("V", [32262, 40003])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_long_rows_against_float64(dtype, V):
    """V = 32262 with p0 = V - 256 (the 7B vocabulary: the window ends with the row; the row stays in registers for the statistics) and
    V = 40003 (the two-read form).  In place against out of place in both."""
    worst, keep = {}, []
    p0, nb = V - 256, 256
    for R, ld, (sigma, W), gs, first, end in ((130, V, (1.0, 3), 0.37, 0, False), (3, V + PAD, (2.5, 32), 1.0, 14, True), (1, V, (0.5, 1), 1.0, 35, False),
                                              (3, V, (2.5, 8), 0.37, 3, True)):
        x, tg, ignore = make_case(R, V, p0, nb, W, dtype, seed=R, first=first)
        check(x, tg, ignore, (p0, nb, sigma, W), ld, gs, f"{dtype} V={V} R={R} ld={ld} sigma={sigma} W={W} gs={gs} at_end={end}", worst, keep if end else None)
    for name, (v, tag) in worst.items():
        print(f"ce_soft {dtype} V={V}: worst {name} error / bound {v:.3f} at {tag}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_row_bits_do_not_depend_on_slot_row_count_stride_or_phase(dtype):
    V, nb, gs = 32262, 256, 0.37
    p0, spec = V - 256, (V - 256, 256, 1.0, 3)
    x, tg, ignore = make_case(1, V, p0, nb, 3, dtype, first=7 * 3 + 0)    # a Gaussian row, target near the window's start
    cnt = torch.tensor([100], dtype=torch.int32, device="cuda")          # the same count everywhere: sc is part of the gradient
    alone, agrad = Out(1), torch.empty(1, V, dtype=dtype, device="cuda")
    launch(x.cuda(), tg.cuda(), ignore, cnt, spec, alone, agrad, gs)
    # ld = V + 1 steps the row start by -2 bytes (bf16) or -4 bytes (fp32) modulo 16: slots 0 .. 7 start at every 16-byte phase there is
    for R, slots, ld in ((3, [1], V), (130, [77, 129], V + PAD), (9, list(range(8)), V + 1)):
        other, otg, _ = make_case(R, V, p0, nb, 3, dtype, first=R)
        other[slots], otg[slots] = x[0], tg[0]
        for inplace in (False, True):
            buf, lg = framed(other, ld, SENTINEL)
            grad = lg if inplace else torch.empty(R, V, dtype=dtype, device="cuda")
            o = Out(R)
            launch(lg, otg.cuda(), ignore, cnt, spec, o, grad, gs)
            for slot in slots:
                assert torch.equal(bits(grad[slot]), bits(agrad[0])), (R, slot, ld, inplace)
                assert torch.equal(bits(o.rows[:, 1 + slot]), bits(alone.rows[:, 1])), (R, slot, ld, inplace)


def test_null_dlogits_writes_only_the_four_loss_outputs():
    R, V, p0, nb, W = 9, 300, 40, 256, 3
    x, tg, ignore = make_case(R, V, p0, nb, W, torch.bfloat16, first=2)
    buf, lg = framed(x, V + PAD, float("nan"))
    before = bits(buf).clone()
    cnt = torch.tensor([int((tg != ignore).sum())], dtype=torch.int32, device="cuda")
    a, b = Out(R), Out(R)
    launch(lg, tg.cuda(), ignore, cnt, (p0, nb, 1.0, W), a, None, 1.0)
    launch(lg, tg.cuda(), ignore, cnt, (p0, nb, 1.0, W), b, torch.empty(R, V, dtype=torch.bfloat16, device="cuda"), 1.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), before)
    assert torch.equal(bits(a.rows), bits(b.rows)) and torch.equal(bits(a.sums), bits(b.sums)) and bool((a.rows[:, 1:-1] != SENTINEL).all())


def test_nan_logit_makes_the_rows_outputs_nan_and_leaves_the_others():
    R, V, p0, nb, W = 3, 300, 40, 256, 3
    x = (3 * torch.randn(R, V, generator=torch.Generator().manual_seed(5))).float()
    x[1, 7] = float("nan")
    tg = torch.tensor([p0 + 5, p0 + 9, 298])
    cnt = torch.tensor([3], dtype=torch.int32, device="cuda")
    o, grad = Out(R), torch.empty(R, V, device="cuda")
    launch(x.cuda(), tg.cuda(), -100, cnt, (p0, nb, 1.0, W), o, grad, 1.0)
    rows = o.rows[:, 1:-1].cpu()
    assert bool(rows[:, 1].isnan().all()) and bool(grad[1].isnan().all()) and bool(rows[:, [0, 2]].isfinite().all()) and bool(grad[[0, 2]].isfinite().all())
    assert bool(o.sums.isnan().all())


def test_op_counts_and_sums_like_the_hard_loss():
    """ops.cross_entropy_soft: count is egomi_ce_count's, nll_sum is the hard loss ops.cross_entropy gives for the rows within both kernels' error."""
    R, V, p0, nb, W = 130, 300, 40, 256, 8
    x, tg, ignore = make_case(R, V, p0, nb, W, torch.float32, first=0)
    x[torch.isinf(x)] = -30.0                                            # finite rows: the sums are compared
    lg, tgd = x.cuda(), tg.cuda()
    tgd = torch.where((tgd < 0) | (tgd >= V), torch.full_like(tgd, ignore), tgd)
    ls, nll, cnt = ops.cross_entropy_soft(lg, tgd, ignore, (p0, nb, 2.5, W))
    hs, hcnt = ops.cross_entropy(lg, tgd, ignore)
    ref = C.soft_ce(x.double().numpy(), tgd.cpu().numpy(), ignore, (p0, nb, 2.5, W))
    assert int(cnt) == int(hcnt) == ref["count"]
    assert abs(float(nll) - ref["row_nll"].sum()) <= 1e-5 * ref["row_nll"].sum() and abs(float(hs) - float(nll)) <= 1e-4 * float(nll)
    assert abs(float(ls) - ref["row_loss"].sum()) <= 1e-5 * ref["row_loss"].sum()
    assert torch.equal(lg.cpu(), x)


def test_argument_checks():
    R, V, p0, nb = 2, 64, 40, 16
    lg = torch.zeros(R, V, dtype=torch.float32, device="cuda")
    dl = torch.full((R, V), SENTINEL, dtype=torch.float32, device="cuda")
    tg = torch.tensor([41, 3], device="cuda")
    cnt = torch.tensor([2], dtype=torch.int32, device="cuda")
    o = Out(R)
    ls, ns, rl, rn = o.args()
    base = dict(lg=lg, ld=V, tg=tg, R=R, V=V, ignore=-100, count=cnt, p0=p0, nb=nb, sigma=1.0, radius=3, loss_sum=ls, nll_sum=ns, row_loss=rl,
                row_nll=rn, dlg=dl, ldd=V, gs=1.0, dtype=dt(lg.dtype))
    for name in ("lg", "tg", "count", "loss_sum", "nll_sum", "row_loss", "row_nll"):
        assert raw(**{**base, name: None}) == BADARG, name
    assert raw(**{**base, "dtype": 99}) == BADARG
    for kw in (dict(p0=-1), dict(nb=0), dict(p0=V - nb + 1), dict(p0=V), dict(radius=0), dict(radius=33), dict(radius=-1), dict(sigma=0.0), dict(sigma=-1.0),
               dict(sigma=16.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(ld=V - 1), dict(ldd=V - 1), dict(R=0), dict(V=0)):
        assert raw(**{**base, **kw}) == SHAPE, kw
    assert raw(**{**base, "lg": c_p(lg.data_ptr() + 2)}) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dl == SENTINEL).all()) and bool((o.rows == SENTINEL).all()) and not o.sums.any()     # a refused call launches nothing
    assert raw(**{**base, "p0": V - nb, "sigma": 16.0, "radius": 32}) == OK                          # the limits themselves are accepted
    assert raw(**{**base, "dlg": None, "ldd": 0}) == OK
