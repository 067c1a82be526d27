"""GPU: egomi_traj_grammar_init / egomi_traj_grammar_step (csrc/grammar.hip) alone, through the C-ABI, against tests/grammar_ref.py.

Layouts (grammar_cases.LAYOUTS), bf16 and fp32: V = 16 (below one chunk), V = 300, the 7B vocabulary V = 32262 with the bin window at the
very end of the row and three specials just below it, V = 40003 (the two-read form).  R in {1, 3, 130}, ld in {V, V + 58}.  The logits
buffer ends with its allocation; a sentinel row lies before and after the rows and sentinels fill the padding columns.  Rows cycle through
all ten phases x steps in {0, min - 1, min, max - 1, max}; the launches through rem in {1, 2, 8, 9, 10, 50}; row kinds: Gaussian, a peak
outside the allowed set, -inf on part of the allowed set, -inf on all of it; tok_prev NULL, or per row legal / illegal / pad.
With no tolerance: allowed elements keep their bits, every other element of [0, V) is -inf, sentinels and padding are unchanged, the state
is grammar_ref's, a second launch on fresh copies is bit-equal, and a row gives the same bits at R = 1 and inside R = 130 at either ld.
mass: |got - ref| <= BOUND * (1 + |ref|) with tests/binstats_cases.py's BOUND["mass"] (grammar_cases.py says why), printed before it asserts.
Then egomi_traj_grammar_init on prompts, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from egoscaler_amd import _lib
from egoscaler_amd.ops import P, S, dt
from tests import binstats_cases as BC
from tests import grammar_cases as C
from tests import grammar_ref as G
from tests.test_gpu_logprob_kernel import at_end

pytestmark = pytest.mark.gpu
c_i, c_i64, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
OK, BADARG, SHAPE, UNSUPPORTED = 0, -1, -2, -4
SENTINEL = 7.0
INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def raw_step(lg_ptr, ld, R, V, tok, state, spec, rem, mass, ld_mass, col, dtype):
    fn = _lib.lib().egomi_traj_grammar_step
    return fn(lg_ptr, c_i64(ld), c_i(R), c_i(V), P(tok), P(state), c_i64(spec.p0), c_i(spec.nb), c_i64(spec.ts), c_i64(spec.tsep), c_i64(spec.te),
              c_i64(spec.eos), c_i(spec.min_steps), c_i(spec.max_steps), c_i(rem), P(mass), c_i64(ld_mass), c_i(col), c_i(dtype), S())


def raw_init(ids_ptr, ld_ids, mask, ld_mask, R, S0, spec, state, need):
    fn = _lib.lib().egomi_traj_grammar_init
    return fn(ids_ptr, c_i64(ld_ids), P(mask), c_i64(ld_mask), c_i(R), c_i(S0), c_i64(spec.p0), c_i(spec.nb), c_i64(spec.ts), c_i64(spec.tsep),
              c_i64(spec.te), c_i64(spec.eos), c_i(spec.min_steps), c_i(spec.max_steps), P(state), P(need), S())


def bits(t):
    return t.contiguous().view(INT[t.dtype])


def launch(case, x, ld, keep):
    """One launch on a fresh framed copy of x (CPU tensor [R, V]): -> (rows [R, V] CPU, mass [R] numpy, state [R, 2] numpy); asserts the
    frame (sentinel rows, padding columns) and the other mass columns untouched."""
    R, V = x.shape
    frame = torch.full((R + 2, ld), SENTINEL, dtype=x.dtype)
    frame[1:R + 1, :V] = x
    dev = at_end(frame, keep)
    state = torch.from_numpy(case["state0"].copy()).cuda()
    tok = None if case["tok"] is None else torch.from_numpy(case["tok"]).cuda()
    mass = torch.full((R, 3), SENTINEL, dtype=torch.float32, device="cuda")
    rc = raw_step(c_p(dev[1].data_ptr()), ld, R, V, tok, state, case["spec"], case["rem"], mass, 3, 1, dt(x.dtype))
    assert rc == OK, rc
    torch.cuda.synchronize()
    got = dev.cpu()
    fb, gb = bits(frame), bits(got)
    assert torch.equal(gb[0], fb[0]) and torch.equal(gb[R + 1], fb[R + 1]), "a sentinel row was written"
    assert torch.equal(gb[:, V:], fb[:, V:]), "a padding column was written"
    mass = mass.cpu()
    assert bool((mass[:, 0] == SENTINEL).all()) and bool((mass[:, 2] == SENTINEL).all())
    del keep[:]
    return got[1:R + 1, :V].contiguous(), mass[:, 1].numpy().copy(), state.cpu().numpy()


def check(case, x, rows, mass, state, tag, worst):
    assert torch.equal(bits(rows), bits(C.expected_rows(case, x))), f"{tag}: the masked rows differ from mask_ref"
    want = np.asarray(case["state1"], dtype=np.int32)
    assert np.array_equal(state, want), f"{tag}: state"
    r = BC.ratio(mass, C.ref_mass(case, x.to(torch.float64).numpy()))
    worst[0] = max(worst[0], r)
    return r


@pytest.mark.parametrize("name", list(C.LAYOUTS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_mask_state_and_mass(dtype, name):
    V = C.LAYOUTS[name][0]
    keep, worst, ratios = [], [0.0], []
    for i, rem in enumerate(C.REMS):
        with_tok = bool(i % 2)
        lds = (V, V + C.PAD_COLS) if i % 2 else (V + C.PAD_COLS, V)
        case = C.make_case(name, 130, rem, with_tok, first=17 * i)
        x = torch.from_numpy(case["x"]).to(dtype)
        rows, mass, state = launch(case, x, lds[0], keep)
        ratios.append(check(case, x, rows, mass, state, f"{dtype} {name} R=130 rem={rem} ld={lds[0]} tok={with_tok}", worst))
        if i < 2:                                                        # a second launch on fresh copies is bit-equal
            rows2, mass2, state2 = launch(case, x, lds[0], keep)
            assert torch.equal(bits(rows), bits(rows2)) and np.array_equal(mass.view(np.int32), mass2.view(np.int32)) and np.array_equal(state, state2)
        for slot in (0, 77, 129) if i < 3 else (3 + 11 * i,):            # the same row alone, at the other ld
            one = dict(case, state0=case["state0"][slot:slot + 1], tok=None if case["tok"] is None else case["tok"][slot:slot + 1],
                       state1=case["state1"][slot:slot + 1], keep=case["keep"][slot:slot + 1])
            rows1, mass1, state1 = launch(one, x[slot:slot + 1], lds[1], keep)
            assert torch.equal(bits(rows1[0]), bits(rows[slot])), (name, rem, slot)
            assert mass1.view(np.int32)[0] == mass.view(np.int32)[slot] and np.array_equal(state1[0], state[slot]), (name, rem, slot)
        if i in (1, 4):                                                  # R = 3 at both strides, other states
            for ld in (V, V + C.PAD_COLS):
                c3 = C.make_case(name, 3, rem, not with_tok, first=5 * i + ld)
                x3 = torch.from_numpy(c3["x"]).to(dtype)
                ratios.append(check(c3, x3, *launch(c3, x3, ld, keep), f"{dtype} {name} R=3 rem={rem} ld={ld}", worst))
    print(f"grammar_step {dtype} {name}: worst mass |got - ref| / (1 + |ref|) = {worst[0]:.3e} (BOUND {BC.BOUND['mass']:.3e})")
    assert worst[0] <= BC.BOUND["mass"], (name, dtype, worst[0], ratios)


def test_all_inf_rows_nan_rows_and_single_support():
    name = "mid"
    V, spec, pad = C.spec_of(name)
    st = [(6, 1), (7, 2), (8, 2), (9, 0), (3, 1), (0, 5)]
    R = len(st)
    x = torch.randn(R, V, generator=torch.Generator().manual_seed(5)) * 3
    x[0, spec.tsep] = float("-inf")                                      # the one allowed logit is already -inf: mass 0, the row all -inf
    x[4, 7] = float("nan")                                               # a NaN inside the allowed window: it stays, mass NaN
    x[5, 290] = float("nan")                                             # a NaN outside the allowed set: masked, mass NaN
    keepm = np.zeros((R, V), dtype=bool)
    for r in range(R):
        keepm[r, G.allowed(spec, st[r], 20)] = True
    case = dict(state0=np.asarray(st, dtype=np.int32), tok=torch.tensor([pad, spec.eos, 9, spec.ts, spec.p0, spec.te]).numpy(), spec=spec, rem=20,
                keep=None, state1=None)
    st1 = [G.advance(spec, s, t) for s, t in zip(st, case["tok"])]       # (6,1) pad -> stays; (7,2) eos -> 8; 8 absorbs; 9 ts -> 0; bin -> 4; te -> 7
    keepm[:] = False
    for r in range(R):
        keepm[r, G.allowed(spec, st1[r], 20)] = True
    case.update(keep=keepm, state1=st1)
    rows, mass, state = launch(case, x, V + 3, [])
    assert torch.equal(bits(rows), bits(C.expected_rows(case, x)))
    assert np.array_equal(state, np.asarray(st1, dtype=np.int32))
    assert mass[0] == 0.0 and bool(torch.isinf(rows[0]).all())
    assert np.isnan(mass[4]) and np.isnan(mass[5]) and bool(torch.isnan(rows[4, 7])) and rows[5, 290] == float("-inf")
    for r in (1, 2):                                                     # a one-token support: exactly one finite element
        assert int(torch.isfinite(rows[r]).sum()) == 1 and 0.0 < mass[r] < 1.0
    assert int(torch.isfinite(rows[3]).sum()) == spec.nb                 # (0, 0) below min_steps with room: the bins and nothing else


def test_init_reads_the_prompt():
    V, spec, pad = C.spec_of("7b")
    b, step = spec.p0, [spec.p0 + 3] * 6 + [spec.tsep]
    prompts = [[11, 12, 13], [11, spec.ts], [11, spec.ts] + step, [spec.ts] + step * 2 + [b, b, b], [spec.ts] + step + [b] * 9,
               [spec.ts] + step * 3 + [spec.ts] + step[:4], [spec.ts] + step * 6, [spec.ts, b, b, 11, b], [spec.ts] + step * 5 + [b] * 6]
    S0 = max(len(p) for p in prompts)
    R = len(prompts)
    ids = np.full((R, S0 + 2), pad, dtype=np.int64)                      # left-padded, a row stride above S0
    mk = np.zeros((R, S0 + 5), dtype=np.uint8)
    for r, p in enumerate(prompts):
        ids[r, S0 - len(p):S0] = p
        mk[r, S0 - len(p):S0] = 1
    ids[3, 0], mk[3, 0] = spec.ts, 0                                     # a masked <ts> and masked bins do not count
    ids[7, S0 - 2], mk[7, S0 - 2] = b, 0
    d_ids, d_mk = torch.from_numpy(ids).cuda(), torch.from_numpy(mk).cuda()
    for mask in (d_mk, None):
        state = torch.full((R, 2), -5, dtype=torch.int32, device="cuda")
        need = torch.full((R,), -5, dtype=torch.int32, device="cuda")
        assert raw_init(P(d_ids), S0 + 2, mask, S0 + 5, R, S0, spec, state, need) == OK
        for r in range(R):
            want = G.init_state(spec, ids[r, :S0], mk[r, :S0] if mask is not None else None)
            assert tuple(state[r].tolist()) == want, (r, want)
            assert int(need[r]) == G.need(spec, want), (r, want)
    assert G.init_state(spec, ids[6, :S0], mk[6, :S0]) == (0, 6) and G.need(spec, (0, 6)) == G.NEVER


def test_argument_checks():
    V, spec, pad = C.spec_of("mid")
    R = 2
    lg = torch.zeros(R, V, dtype=torch.float32, device="cuda")
    state = torch.zeros(R, 2, dtype=torch.int32, device="cuda")
    mass = torch.full((R, 2), SENTINEL, dtype=torch.float32, device="cuda")
    base = dict(lg_ptr=P(lg), ld=V, R=R, V=V, tok=None, state=state, spec=spec, rem=5, mass=mass, ld_mass=2, col=0, dtype=dt(lg.dtype))
    bad = lambda **kw: raw_step(**{**base, **kw})
    sp = lambda **kw: spec._replace(**kw)
    assert bad(lg_ptr=c_p(None)) == BADARG and bad(state=None) == BADARG and bad(mass=None) == BADARG and bad(dtype=99) == BADARG
    for kw in (dict(R=0), dict(V=0), dict(ld=V - 1), dict(col=-1), dict(col=2), dict(ld_mass=0), dict(rem=0), dict(spec=sp(nb=0)),
               dict(spec=sp(nb=1025)), dict(spec=sp(p0=-1)), dict(spec=sp(p0=V - 255)), dict(spec=sp(ts=V)), dict(spec=sp(eos=-1)),
               dict(spec=sp(te=spec.p0)), dict(spec=sp(tsep=spec.p0 + spec.nb - 1)), dict(spec=sp(ts=spec.tsep)),
               dict(spec=sp(min_steps=6)), dict(spec=sp(min_steps=-1))):
        assert bad(**kw) == SHAPE, kw
    assert bad(lg_ptr=c_p(lg.data_ptr() + 2)) == UNSUPPORTED
    assert bad(lg_ptr=c_p(lg.data_ptr() + 1), dtype=dt(torch.bfloat16)) == UNSUPPORTED
    ids = torch.zeros(R, 4, dtype=torch.int64, device="cuda")
    need = torch.full((R,), -5, dtype=torch.int32, device="cuda")
    ini = lambda **kw: raw_init(**{**dict(ids_ptr=P(ids), ld_ids=4, mask=None, ld_mask=0, R=R, S0=4, spec=spec, state=state, need=need), **kw})
    assert ini(ids_ptr=c_p(None)) == BADARG and ini(state=None) == BADARG and ini(need=None) == BADARG
    for kw in (dict(R=0), dict(S0=0), dict(ld_ids=3), dict(mask=torch.ones(R, 4, dtype=torch.uint8, device="cuda"), ld_mask=3),
               dict(spec=sp(nb=1025)), dict(spec=sp(min_steps=6)), dict(spec=sp(te=spec.p0 + 1))):
        assert ini(**kw) == SHAPE, kw
    torch.cuda.synchronize()                                             # none of them launched
    assert bool((lg == 0).all()) and bool((state == 0).all()) and bool((mass == SENTINEL).all()) and bool((need == -5).all())
    assert bad() == OK and ini() == OK
