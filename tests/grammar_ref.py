"""Shared by the grammar tests (tests/test_grammar_host.py on the CPU, tests/test_gpu_grammar_*.py on the GPU): the trajectory grammar of
csrc/grammar.hip restated in numpy.  Not a test file; numpy only.

A spec is any object with the fields p0, nb, ts, tsep, te, eos, min_steps, max_steps (traj.GrammarSpec, or Spec below); a state is the
pair (phase, steps).  Here are the transition table (advance), allowed(state, rem), need(state), the state a prompt leaves (init_state),
mask_ref(row, state, rem), the float64 mass, and the strict validator."""
import collections

import numpy as np

Spec = collections.namedtuple("Spec", "p0 nb ts tsep te eos min_steps max_steps")
NEVER = 1 << 30                                   # need of a state from which no legal close exists (EGOMI_GRAMMAR_NEVER)
PHASES = tuple(range(10))


def is_bin(spec, tok):
    return spec.p0 <= tok < spec.p0 + spec.nb


def advance(spec, state, tok):
    """The state after `tok`.  A transition looks at the token alone; a token without a transition leaves the state as it is."""
    phase, steps = state
    tok = int(tok)
    if phase == 9:
        return (0, 0) if tok == spec.ts else state
    if phase == 0:
        return (1, steps) if is_bin(spec, tok) else ((7, steps) if tok == spec.te else state)
    if 1 <= phase <= 5:
        return (phase + 1, steps) if is_bin(spec, tok) else state
    if phase == 6:
        return (0, steps + 1) if tok == spec.tsep else state
    if phase == 7:
        return (8, steps) if tok == spec.eos else state
    return state                                  # 8 absorbs


def allowed(spec, state, rem):
    """The sorted list of the ids the state allows when the loop still emits `rem` tokens, this one included."""
    phase, steps = state
    bins, sp = False, None
    if phase == 9:
        sp = spec.ts
    elif phase == 0:
        bins = steps < spec.max_steps and rem >= 9
        if steps >= spec.min_steps or not bins:
            sp = spec.te
    elif 1 <= phase <= 5:
        bins = True
    elif phase == 6:
        sp = spec.tsep
    elif phase in (7, 8):
        sp = spec.eos
    ids = list(range(spec.p0, spec.p0 + spec.nb)) if bins else []
    return sorted(ids + ([sp] if sp is not None else []))


def need(spec, state):
    """Tokens from the state to the earliest legal close `... <te> eos` with min_steps <= n <= max_steps; NEVER where there is none."""
    phase, steps = state
    mn, mx = spec.min_steps, spec.max_steps

    def from0(s):
        return NEVER if s > mx else 7 * max(0, mn - s) + 2
    if phase == 8:
        n = 0 if mn <= steps <= mx else NEVER
    elif phase == 7:
        n = 1 if mn <= steps <= mx else NEVER
    elif phase == 0:
        n = from0(steps)
    elif 1 <= phase <= 6:
        n = (6 - phase) + 1 + from0(steps + 1)
    elif phase == 9:
        n = 1 + from0(0)
    else:
        n = NEVER
    return min(n, NEVER)


def init_state(spec, ids, mask=None):
    """The state a prompt leaves: from its last <ts>, steps = the <tsep> after it, phase = the trailing run of bins (capped at 6); no <ts>:
    (9, 0).  Positions with mask == 0 are skipped."""
    seen, steps, run = False, 0, 0
    for j, t in enumerate(np.asarray(ids).tolist()):
        if mask is not None and not mask[j]:
            continue
        if t == spec.ts:
            seen, steps, run = True, 0, 0
        elif not seen:
            continue
        elif t == spec.tsep:
            steps, run = steps + 1, 0
        elif is_bin(spec, t):
            run = min(run + 1, 6)
        else:
            run = 0
    return (run, steps) if seen else (9, 0)


def mask_ref(spec, row, state, rem):
    """A copy of `row` (numpy floats [..., V]) with -inf over every id the state does not allow; the allowed elements keep their bits."""
    out = np.array(row, copy=True)
    keep = np.zeros(out.shape[-1], dtype=bool)
    keep[allowed(spec, state, rem)] = True
    out[..., ~keep] = -np.inf
    return out


def mass_ref(spec, row64, state, rem):
    """float64: the probability the row gives the allowed set, sum exp(x_a - m) / sum exp(x - m).  NaN for a row with a NaN (or all -inf)."""
    x = np.asarray(row64, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max()
        e = np.exp(x - m)
        return float(e[allowed(spec, state, rem)].sum() / e.sum())


def prompt_tail(spec, ids, mask=None):
    """The prompt from its last <ts> on (masked positions dropped); [] without a <ts>."""
    ids = [int(t) for j, t in enumerate(np.asarray(ids).tolist()) if mask is None or mask[j]]
    last = max((j for j, t in enumerate(ids) if t == spec.ts), default=None)
    return [] if last is None else ids[last:]


def valid(spec, tail, gen, pad=None):
    """The strict validator.  `gen` (the generated span) is appended to `tail` (prompt_tail) and the whole is cut after its first eos; that
    must read <ts> (bin{6} <tsep>){n} <te> eos with min_steps <= n <= max_steps, and only pad or eos may follow the cut."""
    seq = [int(t) for t in tail] + [int(t) for t in np.asarray(gen).tolist()]
    if spec.eos not in seq:
        return False
    cut = seq.index(spec.eos) + 1
    body, rest = seq[:cut], seq[cut:]
    if any(t != spec.eos and t != pad for t in rest):
        return False
    if len(body) < 3 or body[0] != spec.ts or body[-2] != spec.te:
        return False
    mid = body[1:-2]
    if len(mid) % 7:
        return False
    n = len(mid) // 7
    for i in range(n):
        step = mid[7 * i:7 * i + 7]
        if not all(is_bin(spec, t) for t in step[:6]) or step[6] != spec.tsep:
            return False
    return spec.min_steps <= n <= spec.max_steps


def state_prompt(spec, state):
    """A shortest token sequence from <ts> that leaves the table in `state` ([] for phase 9), for tests that start from a given state."""
    phase, steps = state
    if phase == 9:
        return []
    seq = [spec.ts] + ([spec.p0] * 6 + [spec.tsep]) * steps
    if 1 <= phase <= 6:
        seq += [spec.p0 + spec.nb - 1] * phase
    elif phase >= 7:
        seq += [spec.te] + ([spec.eos] if phase == 8 else [])
    return seq
