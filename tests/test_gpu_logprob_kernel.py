"""GPU: egomi_token_logprob (csrc/logprob.hip) alone, through the C-ABI, against the float64 log_softmax of the values it receives.

Bound: |got - ref| <= BOUND * (1 + |ref|) per row, tests/logprob_cases.py:
    MEASURED = 1.095e-07  worst ratio over every case below on the MI355X (printed by every case before it asserts)
    BOUND    = 4.38e-07   4 x MEASURED
Cases: bf16 and fp32; V in {5, 1023, 1024, 1025, 4099, 32262} and, for the two-pass form, {32768, 32769, 40003}; R in {1, 3, 130};
ld = V and ld = V + 58 with the padding columns poisoned with NaN; the logits at the end of their allocation; the rows of
logprob_cases.KINDS.  Then the bookkeeping (live / eos / pad == eos / eos_id = -1 / the running sum bit for bit), determinism eager against
a captured graph, slot independence, a token id out of range, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib
from egoscaler_amd.decode import _capture
from egoscaler_amd.ops import P, S, dt
from tests import logprob_cases as C

pytestmark = pytest.mark.gpu
c_i, c_i64, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
SEG = 2 << 20
OK, BADARG, SHAPE, UNSUPPORTED = 0, -1, -2, -4


def at_end(src, keep):
    """A copy of `src` whose last byte is the last byte of a fresh device allocation of its own (tests/test_gpu_w8_kernels.py's pattern)."""
    n, es = src.numel(), src.element_size()
    nbytes = max(16 << 20, -(-n * es // SEG) * SEG)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    buf = torch.empty(nbytes // es, dtype=src.dtype, device="cuda")
    keep.append(buf)
    t = buf[buf.numel() - n:].view(src.shape)
    t.copy_(src)
    return t


def raw(lg_ptr, ld, R, V, tok, eos, live, tok_lp, ld_lp, col, sum_lp, n_tok, dtype):
    fn = _lib.lib().egomi_token_logprob
    fn.restype = c_i
    return fn(lg_ptr, c_i64(ld), c_i(R), c_i(V), P(tok), c_i64(eos), P(live), P(tok_lp), c_i64(ld_lp), c_i(col), P(sum_lp), P(n_tok), c_i(dtype), S())


class Run:
    """Output buffers of R rows x T columns and one launch per call."""

    def __init__(self, R, T=1, live=False):
        self.R, self.T = R, T
        self.tok_lp = torch.full((R, T), 7.0, dtype=torch.float32, device="cuda")
        self.sum_lp = torch.zeros(R, dtype=torch.float32, device="cuda")
        self.n_tok = torch.zeros(R, dtype=torch.int32, device="cuda")
        self.live = torch.ones(R, dtype=torch.int32, device="cuda") if live else None

    def step(self, lg, tok, col=0, eos=-1, V=None):
        V = lg.shape[1] if V is None else V
        rc = raw(P(lg), lg.stride(0), self.R, V, tok, eos, self.live, self.tok_lp, self.T, col, self.sum_lp, self.n_tok, dt(lg.dtype))
        assert rc == OK, rc


def _device_rows(x, ld, keep=None):
    """x [R, V] (CPU) -> a device view [R, V] of row stride ld whose padding columns hold NaN."""
    R, V = x.shape
    full = torch.full((R, ld), float("nan"), dtype=x.dtype)
    full[:, :V] = x
    d = full.cuda() if keep is None else at_end(full.cuda(), keep)
    return d[:, :V]


def _check(x, tok, lg, tag):
    R = x.shape[0]
    run = Run(R)
    run.step(lg, tok.cuda())
    got = run.tok_lp[:, 0].cpu().numpy()
    ref = C.ref_logprob(C.received(x), tok.numpy())
    r = C.ratio(got, ref)
    print(f"token_logprob {tag}: worst |got - ref| / (1 + |ref|) = {r:.3e} (BOUND {C.BOUND:.2e})")
    assert r <= C.BOUND, tag
    assert torch.equal(run.sum_lp, run.tok_lp[:, 0]) and bool((run.n_tok == 1).all())
    return r


@pytest.mark.parametrize("V", C.VS + C.VS_LONG)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_against_float64_log_softmax(dtype, V):
    worst, keep = 0.0, []
    for R in C.RS:
        if V in C.VS_LONG and R == 130:
            continue                                                     # the two-pass form differs per row only: 1 and 3 rows reach it
        for first in range(0, len(C.KINDS), R):                          # every kind of row at every R
            x, tok = C.make_rows(R, V, dtype, first_kind=first)
            for ld in (V, V + C.PAD):
                worst = max(worst, _check(x, tok, _device_rows(x, ld), f"{dtype} V={V} R={R} ld={ld} first={first}"))
    x, tok = C.make_rows(3, V, dtype, first_kind=1)
    for ld in (V, V + C.PAD):                                            # the last row ends with its allocation (ld = V: with the row itself)
        worst = max(worst, _check(x, tok, _device_rows(x, ld, keep), f"{dtype} V={V} R=3 ld={ld} at_end"))
    print(f"token_logprob {dtype} V={V}: worst ratio of the case {worst:.3e}")


def test_known_values():
    V = 4099
    x = torch.full((2, V), 1.5)
    run = Run(2)
    run.step(x.cuda(), torch.tensor([0, V - 1]).cuda())
    assert np.abs(run.tok_lp[:, 0].cpu().numpy() + np.log(V)).max() <= C.BOUND * (1 + np.log(V))
    x, tok = C.make_rows(2, V, torch.float32, first_kind=1)             # peak_tok, peak_other
    run = Run(2)
    run.step(x.cuda(), tok.cuda())
    lp = run.tok_lp[:, 0].cpu().numpy()
    assert -1e-6 <= lp[0] <= 0 and -120 < lp[1] <= -80


def _five_steps(R, V, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    lgs = [(3 * torch.randn(R, V, generator=g)).to(dtype).cuda() for _ in range(5)]
    toks = [torch.randint(0, V, (R,), generator=g) for _ in range(5)]
    return lgs, toks


def test_bookkeeping_eos_live_and_running_sum():
    R, V, EOS = 4, 1025, 9
    lgs, toks = _five_steps(R, V, torch.float32)
    for t in range(5):
        toks[t][0] = 10 + t                                              # row 0 never emits eos
        toks[t][1] = EOS if t >= 2 else 10                               # row 1 emits it at step 2 of 5 and is then fed pad == eos
    toks[4][3] = EOS                                                     # row 3 at the last step; row 2 as drawn
    toks = [t.cuda() for t in toks]
    a, b, c = Run(R, 5, live=True), Run(R, 5, live=False), Run(R, 5, live=True)
    for t in range(5):
        a.step(lgs[t], toks[t], col=t, eos=EOS)
        b.step(lgs[t], toks[t], col=t, eos=EOS)                          # live NULL: every row counts at every step
        c.step(lgs[t], toks[t], col=t, eos=-1)                           # eos_id = -1: nothing ever finishes
    torch.cuda.synchronize()
    ends = [int((torch.stack(toks, 1)[r] == EOS).int().argmax()) + 1 if bool((torch.stack(toks, 1)[r] == EOS).any()) else 5 for r in range(R)]
    assert ends[0] == 5 and ends[1] == 3
    assert a.n_tok.tolist() == ends and a.live.tolist() == [int(e == 5 and int(toks[4][r]) != EOS) for r, e in enumerate(ends)]
    for r in range(R):
        assert torch.equal(a.tok_lp[r, :ends[r]], b.tok_lp[r, :ends[r]])              # the eos itself is counted
        assert bool((a.tok_lp[r, ends[r]:] == 0).all())                                # the columns after it are 0
    assert b.n_tok.tolist() == [5] * R and c.n_tok.tolist() == [5] * R and c.live.tolist() == [1] * R
    assert torch.equal(b.tok_lp, c.tok_lp) and bool((b.tok_lp != 7.0).all())
    for run in (a, b, c):                                                # sum_lp = the stored columns added in step order, in fp32, bit for bit
        acc = torch.zeros(R, dtype=torch.float32, device="cuda")
        for t in range(5):
            acc = acc + run.tok_lp[:, t]
        assert torch.equal(acc, run.sum_lp)
    ref = C.ref_logprob(C.received(lgs[0].cpu()), toks[0].cpu().numpy())
    assert C.ratio(a.tok_lp[:, 0].cpu().numpy(), ref) <= C.BOUND


def test_replay_and_graph_are_bit_equal():
    R, V = 3, 4099
    lgs, toks = _five_steps(R, V, torch.bfloat16)
    for t in range(5):
        toks[t] = toks[t] % (V - 6) + 6                                  # no row draws the eos id by chance
    toks[1][2] = 5                                                       # row 2 emits it at step 1
    toks = [t.cuda() for t in toks]

    def go(run):
        for t in range(5):
            run.step(lgs[t], toks[t], col=t, eos=5)
    a, b, c = Run(R, 5, live=True), Run(R, 5, live=True), Run(R, 5, live=True)
    go(a)
    go(b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        go(c)
    for _ in range(2):                                                   # the second replay starts from reset buffers like the first
        c.sum_lp.zero_()
        c.n_tok.zero_()
        c.live.fill_(1)
        g.replay()
        torch.cuda.synchronize()
        for x, y in ((a, b), (a, c)):
            assert torch.equal(x.tok_lp, y.tok_lp) and torch.equal(x.sum_lp, y.sum_lp) and torch.equal(x.n_tok, y.n_tok)
            assert torch.equal(x.live, y.live)
    assert a.n_tok.tolist() == [5, 5, 2]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_row_bits_do_not_depend_on_slot_or_row_count(dtype):
    V = 32262
    x, tok = C.make_rows(1, V, dtype)
    alone = Run(1)
    alone.step(x.cuda(), tok.cuda())
    for R, slot, ld in ((3, 1, V), (130, 77, V), (130, 129, V + C.PAD), (5, 2, V + 1), (5, 4, V + 3)):   # every 16-byte phase of the row start
        other, otok = C.make_rows(R, V, dtype, first_kind=slot)
        other[slot], otok[slot] = x[0], tok[0]
        run = Run(R)
        run.step(_device_rows(other, ld), otok.cuda())
        assert torch.equal(run.tok_lp[slot], alone.tok_lp[0]), (R, slot, ld)
        assert torch.equal(run.sum_lp[slot], alone.sum_lp[0])


def test_token_out_of_range_gives_nan_and_reads_nothing_out_of_range():
    V, keep = 1025, []
    x, tok = C.make_rows(3, V, torch.bfloat16)
    tok[0], tok[2] = -1, V + 10 ** 9
    run = Run(3)
    run.step(_device_rows(x, V, keep), tok.cuda())
    lp = run.tok_lp[:, 0].cpu().numpy()
    assert np.isnan(lp[0]) and np.isnan(lp[2]) and np.isfinite(lp[1])
    assert np.isnan(run.sum_lp.cpu().numpy()[[0, 2]]).all() and run.n_tok.tolist() == [1, 1, 1]


def test_argument_checks():
    R, V = 2, 64
    lg = torch.zeros(R, V, dtype=torch.float32, device="cuda")
    tok = torch.zeros(R, dtype=torch.int64, device="cuda")
    run = Run(R, 4)
    base = dict(lg_ptr=P(lg), ld=V, R=R, V=V, tok=tok, eos=-1, live=None, tok_lp=run.tok_lp, ld_lp=4, col=0, sum_lp=run.sum_lp, n_tok=run.n_tok,
                dtype=dt(lg.dtype))
    assert raw(**base) == OK
    for name in ("tok", "tok_lp", "sum_lp", "n_tok"):
        assert raw(**{**base, name: None}) == BADARG, name
    assert raw(**{**base, "lg_ptr": c_p(None)}) == BADARG
    assert raw(**{**base, "dtype": 99}) == BADARG
    for kw in (dict(R=0), dict(V=0), dict(ld=V - 1), dict(col=-1), dict(col=4), dict(ld_lp=0)):
        assert raw(**{**base, **kw}) == SHAPE, kw
    assert raw(**{**base, "lg_ptr": c_p(lg.data_ptr() + 2)}) == UNSUPPORTED          # fp32 logits at a 2-byte phase
    assert raw(**{**base, "lg_ptr": c_p(lg.data_ptr() + 1), "dtype": dt(torch.bfloat16)}) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((run.tok_lp[:, 1:] == 7.0).all())
