"""GPU: egomi_bin_stats (csrc/logprob.hip) alone, through the C-ABI, against the float64 statistics of the values it receives.

Bound: |got - ref| <= BOUND[name] * (1 + |ref|) per row and output, tests/binstats_cases.py (MEASURED per output on the MI355X over
every case below, BOUND = 4 x MEASURED; every case prints its worst ratios before it asserts).
Cases: bf16 and fp32; V in {5, 261, 32262, 40003} (the last takes the two-read form); nb in {1, 3, 256, 1024}; the window at the row's
start, in its middle and at its end; R in {1, 3, 130}; ld = V and ld = V + 58 with the padding columns poisoned with NaN; the logits at
the end of their allocation; the rows of binstats_cases.KINDS; output columns 0 and ld_out - 1 with the other columns untouched.  Then
NaN logits, determinism eager against a captured graph, independence of slot, row count and 16-byte phase, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib
from egoscaler_amd.decode import _capture
from egoscaler_amd.ops import P, S, dt
from tests import binstats_cases as C
from tests.test_gpu_logprob_kernel import _device_rows

pytestmark = pytest.mark.gpu
c_i, c_i64, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
OK, BADARG, SHAPE, UNSUPPORTED = 0, -1, -2, -4
SENTINEL = 7.0


def raw(lg_ptr, ld, R, V, p0, nb, values, mass, mean, std, ent, ld_out, col, dtype):
    fn = _lib.lib().egomi_bin_stats
    fn.restype = c_i
    return fn(lg_ptr, c_i64(ld), c_i(R), c_i(V), c_i(p0), c_i(nb), P(values), P(mass), P(mean), P(std), P(ent), c_i64(ld_out), c_i(col), c_i(dtype),
              S())


_VALUES = {}


def dev_values(nb):
    if nb not in _VALUES:
        _VALUES[nb] = torch.from_numpy(C.values(nb)).cuda()
    return _VALUES[nb]


class Run:
    """Output buffers of R rows x T columns (pre-filled with a sentinel) and one launch per call."""

    def __init__(self, R, T=1):
        self.R, self.T = R, T
        self.out = {n: torch.full((R, T), SENTINEL, dtype=torch.float32, device="cuda") for n in C.NAMES}

    def step(self, lg, p0, nb, col=0):
        rc = raw(P(lg), lg.stride(0), self.R, lg.shape[1], p0, nb, dev_values(nb), *(self.out[n] for n in C.NAMES), self.T, col, dt(lg.dtype))
        assert rc == OK, rc

    def column(self, col=0):
        return {n: self.out[n][:, col].cpu().numpy() for n in C.NAMES}


def _check(x, lg, p0, nb, tag, worst):
    run = Run(x.shape[0])
    run.step(lg, p0, nb)
    got, ref = run.column(), C.ref_stats(C.received(x), p0, nb)
    r = {n: C.ratio(got[n], ref[n]) for n in C.NAMES}
    print(f"bin_stats {tag}: worst |got - ref| / (1 + |ref|) " + "  ".join(f"{n} {r[n]:.3e}" for n in C.NAMES))
    for n in C.NAMES:
        if r[n] > worst[n][0]:
            worst[n] = (r[n], tag)
    for n in C.NAMES:
        assert r[n] <= C.BOUND[n], (tag, n, r[n], C.BOUND[n])


@pytest.mark.parametrize("V", C.VS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_against_float64_statistics(dtype, V):
    worst, keep = {n: (0.0, "") for n in C.NAMES}, []
    for nb, p0, R in C.cases(V):
        for first in range(0, len(C.KINDS), R):                          # every kind of row at every (nb, p0, R)
            x = C.make_rows(R, V, p0, nb, dtype, first_kind=first)
            for ld in (V, V + C.PAD):
                _check(x, _device_rows(x, ld), p0, nb, f"{dtype} V={V} nb={nb} p0={p0} R={R} ld={ld} first={first}", worst)
    nb = min(256, V)
    x = C.make_rows(3, V, V - nb, nb, dtype, first_kind=1)
    for ld in (V, V + C.PAD):                                            # the last row ends with its allocation, and the window with the row
        _check(x, _device_rows(x, ld, keep), V - nb, nb, f"{dtype} V={V} nb={nb} p0={V - nb} R=3 ld={ld} at_end", worst)
    for n in C.NAMES:
        print(f"bin_stats {dtype} V={V}: worst {n} ratio of the case {worst[n][0]:.3e} at {worst[n][1]}")


def test_known_values():
    V, nb, p0 = 4099, 256, 3001
    v = C.values(nb)
    x = torch.full((4, V), 1.5)
    x[1, :p0] = x[1, p0 + nb:] = float("-inf")                           # row 1: nothing outside the window
    x[2, p0:p0 + nb] = float("-inf")                                     # row 2: two equal bins far apart
    x[2, p0] = x[2, p0 + nb - 1] = 4.0
    x[3, p0:p0 + nb] = float("-inf")                                     # row 3: all its window mass on one bin
    x[3, p0 + 100] = -2.0
    run = Run(4)
    run.step(x.cuda(), p0, nb)
    g = run.column()
    near = lambda n, row, ref: abs(float(g[n][row]) - ref) <= C.BOUND[n] * (1 + abs(ref))
    assert near("mean", 0, v.mean()) and near("ent", 0, np.log(nb)) and near("mass", 0, nb / V) and near("mass", 1, 1.0)
    assert near("std", 2, abs(v[0] - v[-1]) / 2) and near("mean", 2, 0.0) and near("ent", 2, np.log(2))
    assert near("std", 3, 0.0) and g["ent"][3] == 0.0 and g["mean"][3] == np.float32(v[100])      # std against 0: the absolute error


def test_every_bin_minus_inf_and_nan_logits():
    V, nb, p0 = 1025, 16, 500
    x = C.make_rows(4, V, p0, nb, torch.float32)                         # gauss, peak, two, equal
    x[0, p0:p0 + nb] = float("-inf")                                     # Z = 0
    x[1, 3] = float("nan")                                               # a NaN outside the window
    x[2, p0 + 5] = float("nan")                                          # a NaN inside it
    run = Run(4)
    run.step(x.cuda(), p0, nb)
    g = run.column()
    assert g["mass"][0] == 0.0 and all(np.isnan(g[n][0]) for n in ("mean", "std", "ent"))
    assert np.isnan(g["mass"][1]) and all(np.isfinite(g[n][1]) for n in ("mean", "std", "ent"))
    assert all(np.isnan(g[n][2]) for n in C.NAMES)
    assert all(np.isfinite(g[n][3]) for n in C.NAMES)


def test_output_columns_and_untouched_neighbours():
    R, V, nb, p0, T = 3, 261, 3, 129, 5
    x = C.make_rows(R, V, p0, nb, torch.bfloat16)
    lg = x.cuda()
    one = Run(R)
    one.step(lg, p0, nb)
    for col in (0, T - 1):
        run = Run(R, T)
        run.step(lg, p0, nb, col=col)
        torch.cuda.synchronize()
        for n in C.NAMES:
            assert torch.equal(run.out[n][:, col], one.out[n][:, 0]), (n, col)
            others = [c for c in range(T) if c != col]
            assert bool((run.out[n][:, others] == SENTINEL).all()), (n, col)


def test_replay_and_graph_are_bit_equal():
    R, V, nb, p0, T = 3, 4099, 256, 3001, 5
    g = torch.Generator().manual_seed(3)
    lgs = [(3 * torch.randn(R, V, generator=g)).to(torch.bfloat16).cuda() for _ in range(T)]

    def go(run):
        for t in range(T):
            run.step(lgs[t], p0, nb, col=t)
    a, b, c = Run(R, T), Run(R, T), Run(R, T)
    dev_values(nb)
    go(a)
    go(b)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with _capture(gr):
        go(c)
    for _ in range(2):
        for n in C.NAMES:
            c.out[n].fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        for n in C.NAMES:
            assert torch.equal(a.out[n], b.out[n]) and torch.equal(a.out[n], c.out[n]), n
            assert bool((a.out[n] != SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_row_bits_do_not_depend_on_slot_row_count_or_phase(dtype):
    V, nb = 32262, 256
    p0 = V - nb
    x = C.make_rows(1, V, p0, nb, dtype)
    alone = Run(1)
    alone.step(x.cuda(), p0, nb)
    for R, slot, ld in ((3, 1, V), (130, 77, V), (130, 129, V + C.PAD), (5, 2, V + 1), (5, 4, V + 3)):   # every 16-byte phase of the row start
        other = C.make_rows(R, V, p0, nb, dtype, first_kind=slot)
        other[slot] = x[0]
        run = Run(R)
        run.step(_device_rows(other, ld), p0, nb)
        for n in C.NAMES:
            assert torch.equal(run.out[n][slot], alone.out[n][0]), (n, R, slot, ld)
    buf = torch.full((V + 1,), float("nan"), dtype=dtype, device="cuda")  # the same row one element further into its buffer
    buf[1:] = x[0].cuda()
    run = Run(1)
    run.step(buf[1:].view(1, V), p0, nb)
    for n in C.NAMES:
        assert torch.equal(run.out[n], alone.out[n]), n


def test_argument_checks():
    R, V, nb, p0, T = 2, 64, 16, 40, 4
    lg = torch.zeros(R, V, dtype=torch.float32, device="cuda")
    run = Run(R, T)
    base = dict(lg_ptr=P(lg), ld=V, R=R, V=V, p0=p0, nb=nb, values=dev_values(nb), mass=run.out["mass"], mean=run.out["mean"], std=run.out["std"],
                ent=run.out["ent"], ld_out=T, col=0, dtype=dt(lg.dtype))
    assert raw(**base) == OK
    for name in ("values", "mass", "mean", "std", "ent"):
        assert raw(**{**base, name: None}) == BADARG, name
    assert raw(**{**base, "lg_ptr": c_p(None)}) == BADARG
    assert raw(**{**base, "dtype": 99}) == BADARG
    for kw in (dict(R=0), dict(V=0), dict(ld=V - 1), dict(col=-1), dict(col=T), dict(ld_out=0), dict(nb=0), dict(nb=1025, V=2048, ld=2048),
               dict(p0=-1), dict(p0=V - nb + 1), dict(p0=V)):
        assert raw(**{**base, **kw}) == SHAPE, kw
    assert raw(**{**base, "p0": V - nb}) == OK                                        # the window may end with the row
    assert raw(**{**base, "lg_ptr": c_p(lg.data_ptr() + 2)}) == UNSUPPORTED          # fp32 logits at a 2-byte phase
    assert raw(**{**base, "lg_ptr": c_p(lg.data_ptr() + 1), "dtype": dt(torch.bfloat16)}) == UNSUPPORTED
    torch.cuda.synchronize()
    for n in C.NAMES:
        assert bool((run.out[n][:, 1:] == SENTINEL).all())
