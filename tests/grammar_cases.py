"""For tests/test_gpu_grammar_kernel.py: the layouts egomi_traj_grammar_step is pinned on, the rows, and the bound of its `mass`.  Not a
test file; numpy / torch-CPU only.

mass = (float) Z / s is the construction of egomi_bin_stats' mass (Z in float64 over the allowed ids from fp32 expf(x - m), s the fp32 sum
of egomi_token_logprob's row pass, one fp32 division), so it is held to the same bound, tests/binstats_cases.py BOUND["mass"] = 7.63e-07,
in that file's metric |got - ref| <= BOUND * (1 + |ref|) against the float64 reference grammar_ref.mass_ref on the values the kernel
receives.  The allowed set is a sub-window of at most 1025 ids, exactly bin_stats' case with one more term.
MEASURED on the MI355X over every case of tests/test_gpu_grammar_kernel.py (printed per dtype and layout before it asserts), worst ratio:
    MASS_MEASURED = 9.129e-08   (bf16, V = 16; fp32 worst 7.704e-08 at V = 300; the V = 32262 and 40003 layouts stay under 8e-09)
It is below binstats_cases.BOUND["mass"] = 4 x 1.907e-07, so that bound is the one asserted, unchanged."""
import numpy as np
import torch

from tests import grammar_ref as G

MASS_MEASURED = 9.129e-08
MIN_STEPS, MAX_STEPS = 2, 5
STEPS = (0, MIN_STEPS - 1, MIN_STEPS, MAX_STEPS - 1, MAX_STEPS)
REMS = (1, 2, 8, 9, 10, 50)
RS = (1, 3, 130)
PAD_COLS = 58                                     # ld = V + 58 shifts every row's 16-byte phase
KINDS = ("gauss", "peak_out", "part_inf", "all_inf")
TOK_KINDS = ("legal", "illegal", "pad")

# name: (V, spec without limits, pad id)
LAYOUTS = {
    "below_one_chunk": (16, dict(p0=8, nb=4, ts=1, tsep=3, te=13, eos=15), 0),
    "mid": (300, dict(p0=5, nb=256, ts=2, tsep=4, te=261, eos=299), 1),
    "7b": (32262, dict(p0=32006, nb=256, ts=32003, tsep=32004, te=32005, eos=2), 0),          # the window ends with the row
    "two_read": (40003, dict(p0=100, nb=1024, ts=99, tsep=1124, te=40002, eos=2), 0),
}


def spec_of(name):
    V, ids, pad = LAYOUTS[name]
    return V, G.Spec(min_steps=MIN_STEPS, max_steps=MAX_STEPS, **ids), pad


def states(R, first=0):
    """R states (phase, steps): row r takes entry first + r of the cycle over all ten phases x STEPS."""
    cyc = [(p, s) for s in STEPS for p in G.PHASES]
    return [cyc[(first + r) % len(cyc)] for r in range(R)]


def make_case(name, R, rem, with_tok, first=0, seed=0):
    """One launch's inputs and reference.  -> dict(x float64 [R, V] (the rows before the dtype rounding), state0 [R, 2], tok int64 [R] or
    None, state1 (list, after tok), keep bool [R, V] (the allowed ids of state1 at rem))."""
    V, spec, pad = spec_of(name)
    g = np.random.default_rng(977 * seed + 31 * V + 7 * R + rem + 1000 * first + (5 if with_tok else 0))
    x = g.normal(0.0, 3.0, (R, V))
    st0 = states(R, first)
    tok, st1 = None, list(st0)
    if with_tok:
        tok = np.zeros(R, dtype=np.int64)
        for r in range(R):
            kind = TOK_KINDS[int(g.integers(0, 3))]
            legal = G.allowed(spec, st0[r], rem + 1)
            if kind == "legal" and legal:
                tok[r] = legal[int(g.integers(0, len(legal)))]
            elif kind == "illegal":
                tok[r] = next(t for t in (spec.ts, spec.tsep, spec.te, spec.eos, spec.p0) if t not in legal)
            else:
                tok[r] = pad
            st1[r] = G.advance(spec, st0[r], tok[r])
    keep = np.zeros((R, V), dtype=bool)
    for r in range(R):
        ids = G.allowed(spec, st1[r], rem)
        keep[r, ids] = True
        kind = KINDS[int(g.integers(0, len(KINDS)))]
        if kind == "peak_out":
            x[r, int(np.flatnonzero(~keep[r])[int(g.integers(0, V - len(ids)))])] = x[r].max() + 20.0
        elif kind == "part_inf":
            x[r, ids[1::2]] = -np.inf
        elif kind == "all_inf":
            x[r, ids] = -np.inf
    return dict(x=x, state0=np.asarray(st0, dtype=np.int32), tok=tok, state1=st1, keep=keep, spec=spec, V=V, rem=rem)


def ref_mass(case, x64):
    """float64 mass per row of the values the kernel received, x64 [R, V]."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = x64.max(1, keepdims=True)
        e = np.exp(x64 - m)
        return np.where(case["keep"], e, 0.0).sum(1) / e.sum(1)


def expected_rows(case, x):
    """x (CPU tensor [R, V] of the kernel's dtype) with -inf over every id that is not allowed."""
    out = x.clone()
    out[torch.from_numpy(~case["keep"])] = float("-inf")
    return out
