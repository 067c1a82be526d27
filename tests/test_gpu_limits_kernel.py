"""GPU: egomi_traj_grammar_init_limits / egomi_traj_grammar_step_limits (csrc/grammar.hip) alone, through the C-ABI, against
tests/limits_ref.py (the limits rule) and tests/grammar_ref.py (the unchanged table).

Layouts: tests/grammar_cases.py's, by import -- V = 16 (nb = 4), V = 300, the 7B vocabulary V = 32262 with the bin window at the very
end of the row, V = 40003 above lp_row's register-path threshold (nb = 1024) -- in bf16 and fp32, R = 8 rows, ld = V + 5 (an odd stride:
bf16 rows of every layout start off a 16-byte boundary on odd rows), a sentinel row before and after the rows, sentinels in the padding
columns, the buffer ending with its allocation.
The eight rows of a launch (ROWS below) are hand-made: a window of width 1 (dmax = 0), a window at bin 0, a window at bin nb - 1 (with the
7B layout it ends with the row), the a > b rule upward and downward, prev = -1 (the box alone), <tsep> committing cur, <ts> resetting
prev, a bin setting cur, a token that moves nothing, and phases that allow no bin.  A second launch without tok_prev and at rem = 8
(no step may open) follows.  With no tolerance: the masked rows, the state, the pose, the padding and the sentinels are limits_ref's;
a second launch on fresh copies is bit-equal; a row alone at ld = V gives the bits it gives in slot r of 8 at ld = V + 5.
Full-range limits: logits, state and mass are bit-equal to egomi_traj_grammar_step's on the same input, limits_mass bit-equal to mass.
mass / limits_mass against float64: |got - ref| <= BOUND * (1 + |ref|) with tests/binstats_cases.py BOUND["mass"], the bound the
grammar's mass is held to (the same summation code over at most nb terms), printed before it asserts.
MEASURED on the MI355X over every case of this file, worst ratio: 5.494e-08 (bf16, V = 300; fp32 worst 4.217e-08 at V = 300; the V = 32262 and
40003 layouts stay under 9e-09); profiles/traj_limits.txt keeps it.
A table nobody checked (entries far outside their ranges) still allows bins only, and at least one.
Then egomi_traj_grammar_init_limits on prompts, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib
from egoscaler_amd.ops import P, S, dt
from tests import binstats_cases as BC
from tests import grammar_cases as C
from tests import grammar_ref as G
from tests import limits_ref as L
from tests.test_gpu_logprob_kernel import at_end

pytestmark = pytest.mark.gpu
c_i, c_i64, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
OK, BADARG, SHAPE, UNSUPPORTED = 0, -1, -2, -4
SENTINEL = 7.0
PADC = 5
INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
DTYPES = [torch.bfloat16, torch.float32]


def spec_args(spec):
    return (c_i64(spec.p0), c_i(spec.nb), c_i64(spec.ts), c_i64(spec.tsep), c_i64(spec.te), c_i64(spec.eos), c_i(spec.min_steps), c_i(spec.max_steps))


def raw_step_limits(lg_ptr, ld, R, V, tok, state, spec, rem, mass, ld_mass, col, lim, pose, lmass, dtype):
    fn = _lib.lib().egomi_traj_grammar_step_limits
    return fn(lg_ptr, c_i64(ld), c_i(R), c_i(V), P(tok), P(state), *spec_args(spec), c_i(rem), P(mass), c_i64(ld_mass), c_i(col), P(lim), P(pose),
              P(lmass), c_i(dtype), S())


def raw_step(lg_ptr, ld, R, V, tok, state, spec, rem, mass, ld_mass, col, dtype):
    fn = _lib.lib().egomi_traj_grammar_step
    return fn(lg_ptr, c_i64(ld), c_i(R), c_i(V), P(tok), P(state), *spec_args(spec), c_i(rem), P(mass), c_i64(ld_mass), c_i(col), c_i(dtype), S())


def raw_init_limits(ids_ptr, ld_ids, mask, ld_mask, R, S0, spec, state, need, pose):
    fn = _lib.lib().egomi_traj_grammar_init_limits
    return fn(ids_ptr, c_i64(ld_ids), P(mask), c_i64(ld_mask), c_i(R), c_i(S0), *spec_args(spec), P(state), P(need), P(pose), S())


def bits(t):
    return t.contiguous().view(INT[t.dtype])


def rows_of(spec, pad):
    """The eight hand-made rows: (state0, pose0, lim, tok_prev).  n = nb - 1, h = nb // 2."""
    nb = spec.nb
    n, h = nb - 1, nb // 2
    b = lambda i: spec.p0 + i
    full = [0] * 6 + [n] * 12
    lim = lambda lo=0, hi=n, dmax=n: [lo] * 6 + [hi] * 6 + [dmax] * 6
    unk = [-1] * 6
    return [
        ((0, 1), [h] * 6 + unk, lim(dmax=0), pad),                                 # nothing moves; width 1 at q = h; steps < min: no <te>
        ((6, 1), [n] * 6 + [0, n, h, h, 1, 2], lim(dmax=1), spec.tsep),            # <tsep> commits cur: q = 0, the window [0, 1] at bin 0, and <te>
        ((2, 2), [0, 0, 0, n, 0, 0] + [1, 1, -1, -1, -1, -1], lim(dmax=1), b(h)),   # a bin sets cur[2]; d = 3, q = n: [n - 1, n] ends the bin ids
        ((9, 0), [h] * 6 + [h] * 6, lim(lo=1 if nb > 2 else 0, hi=n - 1 if nb > 2 else n, dmax=0), spec.ts),   # <ts> resets prev: the box alone
        ((1, 1), [h, 0, h, h, h, h] + [h] + unk[1:], lim(lo=h, dmax=1), pad),      # a > b upward: q = 0 below lo = h by more than 1 -> {1}
        ((5, 3), [h, h, h, h, h, n] + [h] * 5 + [-1], lim(hi=h - 1, dmax=1), spec.eos),   # a > b downward: q = n above hi = h - 1 -> {n - 1}
        ((3, 2), unk + [h, h, h, -1, -1, -1], lim(lo=min(1, n), hi=n, dmax=0), spec.te),  # prev unknown: the box [1, n] whatever dmax is
        ((7, 2), [h] * 6 + unk, full, spec.eos),                                   # eos -> phase 8: no bins, the pose stays
    ]


def make(name, with_tok, rem, seed):
    """One launch's inputs and references: dict(x float64 [8, V], state0, pose0, lim, tok, state1, pose1, keep bool [8, V] under the
    limits, keep_g (the grammar alone))."""
    V, spec, pad = C.spec_of(name)
    rows = rows_of(spec, pad)
    R = len(rows)
    g = np.random.default_rng(1000 * seed + V + rem)
    x = g.normal(0.0, 3.0, (R, V))
    st0 = [r[0] for r in rows]
    pose0 = [tuple(r[1]) for r in rows]
    lim = np.asarray([r[2] for r in rows], dtype=np.int32)
    tok = np.asarray([r[3] for r in rows], dtype=np.int64) if with_tok else None
    st1 = [G.advance(spec, st0[r], tok[r]) for r in range(R)] if with_tok else list(st0)
    pose1 = [L.pose_advance(spec, st0[r], pose0[r], tok[r]) for r in range(R)] if with_tok else list(pose0)
    keep, keep_g = np.zeros((R, V), dtype=bool), np.zeros((R, V), dtype=bool)
    for r in range(R):
        keep[r, L.allowed_limits(spec, st1[r], pose1[r], lim[r], rem)] = True
        keep_g[r, G.allowed(spec, st1[r], rem)] = True
    x[0, int(np.flatnonzero(~keep[0])[3])] = x[0].max() + 20.0           # a peak outside the allowed set
    x[1, np.flatnonzero(keep_g[1])[1::2]] = -np.inf                       # -inf on part of what the grammar allows
    return dict(x=x, state0=np.asarray(st0, dtype=np.int32), pose0=np.asarray(pose0, dtype=np.int32), lim=lim, tok=tok, state1=st1, pose1=pose1,
                keep=keep, keep_g=keep_g, spec=spec, V=V, rem=rem)


def launch(case, x, ld, rows=slice(None), limits=True, lim=None):
    """One launch on a fresh framed copy of x[rows] (CPU tensor): -> (rows [R, V] CPU, mass, limits_mass (numpy [R]), state, pose numpy);
    asserts the frame and the other mass columns untouched.  limits=False: egomi_traj_grammar_step on the same input."""
    xs = x[rows]
    R, V = xs.shape
    frame = torch.full((R + 2, ld), SENTINEL, dtype=x.dtype)
    frame[1:R + 1, :V] = xs
    keep = []
    dev = at_end(frame, keep)
    state = torch.from_numpy(case["state0"][rows].copy()).cuda()
    pose = torch.from_numpy(case["pose0"][rows].copy()).cuda()
    table = torch.from_numpy((case["lim"] if lim is None else lim)[rows].copy()).cuda()
    tok = None if case["tok"] is None else torch.from_numpy(case["tok"][rows].copy()).cuda()
    mass = torch.full((R, 3), SENTINEL, dtype=torch.float32, device="cuda")
    lmass = torch.full((R, 3), SENTINEL, dtype=torch.float32, device="cuda")
    if limits:
        rc = raw_step_limits(c_p(dev[1].data_ptr()), ld, R, V, tok, state, case["spec"], case["rem"], mass, 3, 1, table, pose, lmass, dt(x.dtype))
    else:
        rc = raw_step(c_p(dev[1].data_ptr()), ld, R, V, tok, state, case["spec"], case["rem"], mass, 3, 1, dt(x.dtype))
    assert rc == OK, rc
    torch.cuda.synchronize()
    got = dev.cpu()
    fb, gb = bits(frame), bits(got)
    assert torch.equal(gb[0], fb[0]) and torch.equal(gb[R + 1], fb[R + 1]), "a sentinel row was written"
    assert torch.equal(gb[:, V:], fb[:, V:]), "a padding column was written"
    mass, lmass = mass.cpu(), lmass.cpu()
    for m in (mass, lmass):
        assert bool((m[:, 0] == SENTINEL).all()) and bool((m[:, 2] == SENTINEL).all())
    if not limits:
        assert bool((lmass == SENTINEL).all())
    assert torch.equal(table.cpu(), torch.from_numpy((case["lim"] if lim is None else lim)[rows])), "the table was written"
    del keep[:]
    return got[1:R + 1, :V].contiguous(), mass[:, 1].numpy().copy(), lmass[:, 1].numpy().copy(), state.cpu().numpy(), pose.cpu().numpy()


def ref_mass(keep, x64):
    with np.errstate(invalid="ignore", over="ignore"):
        m = x64.max(1, keepdims=True)
        e = np.exp(x64 - m)
        return np.where(keep, e, 0.0).sum(1) / e.sum(1)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.int32), np.ascontiguousarray(v).view(np.int32)) for u, v in zip(a, b))


@pytest.mark.parametrize("name", list(C.LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_window_pose_state_and_mass(dtype, name):
    V = C.LAYOUTS[name][0]
    worst = 0.0
    for i, (with_tok, rem) in enumerate(((True, 50), (False, 8), (True, 9))):
        case = make(name, with_tok, rem, seed=i)
        x = torch.from_numpy(case["x"]).to(dtype)
        rows, mass, lmass, state, pose = launch(case, x, V + PADC)
        want = x.clone()
        want[torch.from_numpy(~case["keep"])] = float("-inf")
        tag = f"{dtype} {name} tok={with_tok} rem={rem}"
        assert torch.equal(bits(rows), bits(want)), f"{tag}: the masked rows differ from limits_ref"
        assert np.array_equal(state, np.asarray(case["state1"], dtype=np.int32)), f"{tag}: state"
        assert np.array_equal(pose, np.asarray(case["pose1"], dtype=np.int32)), f"{tag}: pose"
        fin = torch.isfinite(rows).numpy() | torch.isnan(rows).numpy()
        assert not (fin & ~case["keep"]).any()
        x64 = x.to(torch.float64).numpy()
        r_l, r_g = BC.ratio(lmass, ref_mass(case["keep"], x64)), BC.ratio(mass, ref_mass(case["keep_g"], x64))
        worst = max(worst, r_l, r_g)
        assert (lmass <= mass).all(), tag                                # a subset of the same non-negative terms, the same order
        if i == 0:                                                       # a second launch on fresh copies is bit-equal
            again = launch(case, x, V + PADC)
            assert torch.equal(bits(rows), bits(again[0])) and same_bits((mass, lmass, state, pose), again[1:]), tag
        for slot in range(8) if i == 0 else (1, 2, 5):                   # the row alone at ld = V: the bits of its slot of 8 at ld = V + 5
            one = launch(case, x, V, rows=slice(slot, slot + 1))
            assert torch.equal(bits(one[0][0]), bits(rows[slot])), (tag, slot)
            assert same_bits((mass[slot:slot + 1], lmass[slot:slot + 1], state[slot], pose[slot]), (one[1], one[2], one[3][0], one[4][0])), (tag, slot)
        if i == 0:                                                       # the windows the rows were made for
            spec = case["spec"]
            n, h = spec.nb - 1, spec.nb // 2
            win = lambda r: (np.flatnonzero(case["keep"][r, spec.p0:spec.p0 + spec.nb]).tolist(), bool(case["keep"][r, spec.te]))
            assert win(0) == ([h], False) and win(1) == ([0, 1], True) and win(2) == ([n - 1, n], False)
            assert win(4) == ([1], False) and win(5) == ([n - 1], False) and win(6)[0] == list(range(min(1, n), n + 1))
            assert win(3)[0] == (list(range(1, n)) if spec.nb > 2 else list(range(spec.nb))) and win(7) == ([], False)
            assert case["pose1"][1][:6] == (0, n, h, h, 1, 2) and case["pose1"][3][:6] == L.UNKNOWN and case["pose1"][2][8] == h
    print(f"grammar_step_limits {dtype} {name}: worst mass / limits_mass |got - ref| / (1 + |ref|) = {worst:.3e} (BOUND {BC.BOUND['mass']:.3e})")
    assert worst <= BC.BOUND["mass"], (name, dtype, worst)


@pytest.mark.parametrize("name", list(C.LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_full_range_limits_are_the_grammar_step(dtype, name):
    V, spec, pad = C.spec_of(name)
    for i, (with_tok, rem) in enumerate(((True, 50), (False, 9), (True, 2))):
        case = C.make_case(name, 8, rem, with_tok, first=13 * i)
        g = np.random.default_rng(i)
        case["pose0"] = g.integers(-1, spec.nb, (8, 12)).astype(np.int32)
        case["lim"] = L.full_range(spec.nb, 8)
        x = torch.from_numpy(case["x"]).to(dtype)
        rows_g, mass_g, _, state_g, pose_g = launch(case, x, V + PADC, limits=False)
        rows_l, mass_l, lmass_l, state_l, _ = launch(case, x, V + PADC)
        assert torch.equal(bits(rows_g), bits(rows_l)), (name, i)
        assert np.array_equal(state_g, state_l) and np.array_equal(state_g, np.asarray(case["state1"], dtype=np.int32))
        assert np.array_equal(mass_g.view(np.int32), mass_l.view(np.int32)), (name, i)
        assert np.array_equal(lmass_l.view(np.int32), mass_l.view(np.int32)), (name, i)
        assert np.array_equal(pose_g, case["pose0"])                     # the plain step knows no pose


def test_unchecked_table_allows_bins_only():
    name = "mid"
    V, spec, pad = C.spec_of(name)
    case = make(name, False, 50, seed=9)
    case["state0"] = np.asarray([(p, 1) for p in (0, 1, 2, 3, 4, 5, 0, 3)], dtype=np.int32)
    case["pose0"] = np.asarray([[100000] * 12, [-7] * 12, [5] * 12, [250] * 12, [0] * 12, [255] * 12, [128] * 12, [-1] * 12], dtype=np.int32)
    bad = np.asarray([[-5] * 6 + [spec.nb + 7] * 6 + [-1] * 6, [900] * 6 + [-900] * 6 + [1 << 30] * 6, [300] * 18, [-300] * 18,
                      [200] * 6 + [100] * 6 + [3] * 6, [-(1 << 31)] * 18, [(1 << 31) - 1] * 18, [255] * 6 + [0] * 6 + [0] * 6], dtype=np.int32)
    x = torch.from_numpy(case["x"]).float()
    rows, mass, lmass, state, pose = launch(case, x, V + PADC, lim=bad)
    fin = torch.isfinite(rows).numpy()
    for r in range(8):
        ids = np.flatnonzero(fin[r])
        assert len(ids) >= 1 and spec.p0 <= ids.min() and ids.max() < spec.p0 + spec.nb, (r, ids)
        assert np.array_equal(ids, np.arange(ids.min(), ids.max() + 1))   # one contiguous window
        assert torch.equal(bits(rows[r, ids]), bits(x[r, ids])) and 0.0 < lmass[r] <= mass[r]
    assert np.array_equal(pose, case["pose0"]) and np.array_equal(state, case["state0"])


def test_init_limits_reads_the_pose_from_the_prompt():
    V, spec, pad = C.spec_of("7b")
    b = spec.p0
    step = lambda *v: [b + i for i in v] + [spec.tsep]
    s1, s2 = step(3, 4, 5, 6, 7, 8), step(250, 0, 255, 1, 2, 9)
    prompts = [
        [11, 12, 13],                                                    # no <ts>
        [11, spec.ts],                                                   # <ts> alone
        [11, spec.ts] + s1,                                              # a complete first step
        [spec.ts] + s1 + s2 + [b + 20, b + 21, b + 22],                  # two steps and a partial open one
        [spec.ts] + s1 + [b + 1] * 4 + [spec.tsep],                      # a short run before <tsep>: prev unknown
        [spec.ts] + s1 + [b + 1] * 9 + [spec.tsep],                      # a long run: its first six
        [spec.ts] + s1 + s2 + [spec.ts] + s2[:4],                        # a second <ts> resets
        [spec.ts] + s1 + [b + 30, b + 31, 11, b + 32],                   # another token ends a run
        [spec.ts] + s1 + s2[:6],                                         # six bins open, no <tsep> yet
    ]
    S0 = max(len(p) for p in prompts)
    R = len(prompts)
    ids = np.full((R, S0 + 2), pad, dtype=np.int64)
    mk = np.zeros((R, S0 + 5), dtype=np.uint8)
    for r, p in enumerate(prompts):
        ids[r, S0 - len(p):S0] = p
        mk[r, S0 - len(p):S0] = 1
    ids[3, 0], mk[3, 0] = spec.ts, 0                                     # a masked <ts> does not count
    mk[2, S0 - 5] = 0                                                    # a masked bin inside the step: five bins -> prev unknown
    d_ids, d_mk = torch.from_numpy(ids).cuda(), torch.from_numpy(mk).cuda()
    for mask in (d_mk, None):
        state = torch.full((R, 2), -5, dtype=torch.int32, device="cuda")
        need = torch.full((R,), -5, dtype=torch.int32, device="cuda")
        pose = torch.full((R + 1, 12), -5, dtype=torch.int32, device="cuda")
        assert raw_init_limits(P(d_ids), S0 + 2, mask, S0 + 5, R, S0, spec, state, need, pose) == OK
        state0 = torch.full((R, 2), -5, dtype=torch.int32, device="cuda")
        need0 = torch.full((R,), -5, dtype=torch.int32, device="cuda")
        fn = _lib.lib().egomi_traj_grammar_init
        assert fn(P(d_ids), c_i64(S0 + 2), P(mask), c_i64(S0 + 5), c_i(R), c_i(S0), *spec_args(spec), P(state0), P(need0), S()) == OK
        assert torch.equal(state, state0) and torch.equal(need, need0)   # the state and need of egomi_traj_grammar_init
        assert bool((pose[R] == -5).all())
        for r in range(R):
            m = mk[r, :S0] if mask is not None else None
            assert tuple(state[r].tolist()) == G.init_state(spec, ids[r, :S0], m), r
            assert tuple(pose[r].tolist()) == L.init_pose(spec, ids[r, :S0], m), (r, pose[r].tolist(), L.init_pose(spec, ids[r, :S0], m))
    P_ = lambda r, m=True: L.init_pose(spec, ids[r, :S0], mk[r, :S0] if m else None)
    assert P_(0) == L.UNKNOWN * 2 and P_(1) == L.UNKNOWN * 2
    assert P_(2, False)[:6] == (3, 4, 5, 6, 7, 8) and P_(2)[:6] == L.UNKNOWN
    assert P_(3) == (250, 0, 255, 1, 2, 9, 20, 21, 22, -1, -1, -1)
    assert P_(4)[:6] == L.UNKNOWN and P_(5)[:6] == (1,) * 6 and P_(6) == L.UNKNOWN + (250, 0, 255, 1, -1, -1)
    assert P_(7) == (3, 4, 5, 6, 7, 8, 32, -1, -1, -1, -1, -1) and P_(8) == (3, 4, 5, 6, 7, 8, 250, 0, 255, 1, 2, 9)


def test_argument_checks():
    V, spec, pad = C.spec_of("mid")
    R = 2
    lg = torch.zeros(R, V, dtype=torch.float32, device="cuda")
    state = torch.zeros(R, 2, dtype=torch.int32, device="cuda")
    pose = torch.zeros(R, 12, dtype=torch.int32, device="cuda")
    lim = torch.from_numpy(L.full_range(spec.nb, R)).cuda()
    mass = torch.full((R, 2), SENTINEL, dtype=torch.float32, device="cuda")
    lmass = torch.full((R, 2), SENTINEL, dtype=torch.float32, device="cuda")
    base = dict(lg_ptr=P(lg), ld=V, R=R, V=V, tok=None, state=state, spec=spec, rem=5, mass=mass, ld_mass=2, col=0, lim=lim, pose=pose, lmass=lmass,
                dtype=dt(lg.dtype))
    bad = lambda **kw: raw_step_limits(**{**base, **kw})
    sp = lambda **kw: spec._replace(**kw)
    for kw in (dict(lg_ptr=c_p(None)), dict(state=None), dict(mass=None), dict(lim=None), dict(pose=None), dict(lmass=None), dict(dtype=99)):
        assert bad(**kw) == BADARG, kw
    for kw in (dict(R=0), dict(V=0), dict(ld=V - 1), dict(col=-1), dict(col=2), dict(ld_mass=0), dict(rem=0), dict(spec=sp(nb=0)),
               dict(spec=sp(nb=1025)), dict(spec=sp(p0=V - 255)), dict(spec=sp(ts=V)), dict(spec=sp(te=spec.p0)), dict(spec=sp(min_steps=6))):
        assert bad(**kw) == SHAPE, kw
    assert bad(lg_ptr=c_p(lg.data_ptr() + 2)) == UNSUPPORTED
    ids = torch.zeros(R, 4, dtype=torch.int64, device="cuda")
    need = torch.full((R,), -5, dtype=torch.int32, device="cuda")
    ini = lambda **kw: raw_init_limits(**{**dict(ids_ptr=P(ids), ld_ids=4, mask=None, ld_mask=0, R=R, S0=4, spec=spec, state=state, need=need,
                                                 pose=pose), **kw})
    for kw in (dict(ids_ptr=c_p(None)), dict(state=None), dict(need=None), dict(pose=None)):
        assert ini(**kw) == BADARG, kw
    for kw in (dict(R=0), dict(S0=0), dict(ld_ids=3), dict(spec=sp(nb=1025)), dict(spec=sp(min_steps=6))):
        assert ini(**kw) == SHAPE, kw
    torch.cuda.synchronize()                                             # none of them launched
    assert bool((lg == 0).all()) and bool((state == 0).all()) and bool((pose == 0).all()) and bool((mass == SENTINEL).all())
    assert bool((lmass == SENTINEL).all()) and bool((need == -5).all())
    assert bad() == OK and ini() == OK
