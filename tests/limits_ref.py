"""Shared by the motion-limits tests (tests/test_limits_host.py on the CPU, tests/test_gpu_limits_*.py on the GPU): the limits rule of
csrc/grammar.hip restated in numpy.  Not a test file; numpy only.  The grammar's own table (advance, allowed, need, init_state) is
tests/grammar_ref.py's and is imported, not restated.

A limits row is 18 integers lo[6] | hi[6] | dmax[6] in bins; a pose is 12 integers prev[6] | cur[6] (prev = the bins of the last closed
step, -1 unknown; cur = the bins of the open step seen so far).  Here are the window rule (window), the pose's move with a token
(pose_advance), the pose a prompt leaves (init_pose), allowed_limits(state, pose, lim, rem), mask_ref / mass_ref under the limits, and a
step-by-step count of the violations of a sequence (violations) for the validator traj.limits_violations to be held against."""
import numpy as np

from tests import grammar_ref as G

UNKNOWN = (-1,) * 6


def full_range(nb, rows=1):
    """The table that limits nothing: lo 0, hi nb - 1, dmax nb - 1."""
    return np.tile(np.asarray([0] * 6 + [nb - 1] * 12, dtype=np.int32), (rows, 1))


def window(lo, hi, dmax, q):
    """The inclusive window (a, b) of bin indices: the box [lo, hi] cut to within dmax of q, the bin the last closed step chose
    (q < 0: unknown, the box alone).  Empty means q lies farther than dmax outside the box: then the cap wins and the window is the one
    bin dmax nearer to the box."""
    if q < 0:
        return lo, hi
    a, b = max(lo, q - dmax), min(hi, q + dmax)
    if a > b:
        e = lo if q < lo else hi
        a = b = min(max(e, q - dmax), q + dmax)
    return a, b


def pose_advance(spec, state, pose, tok):
    """The pose after `tok` taken in `state` (the state BEFORE the token).  It moves only where G.advance moves the phase."""
    tok = int(tok)
    phase = state[0]
    new = G.advance(spec, state, tok)
    prev, cur = list(pose[:6]), list(pose[6:])
    if new[0] != phase:
        if 0 <= phase <= 5 and new[0] == phase + 1:                      # a bin at phase p
            cur[phase] = tok - spec.p0
        elif phase == 6:                                                 # <tsep>
            prev = list(cur)
        elif phase == 9:                                                 # <ts>
            prev = [-1] * 6
    return tuple(prev + cur)


def init_pose(spec, ids, mask=None):
    """The pose a prompt leaves, beside G.init_state: prev is committed at a <tsep> only when the run before it held six bins, else it is
    unknown; <ts> resets it; cur holds the bins of the trailing run and -1 elsewhere.  No <ts>: all -1."""
    seen, run = False, 0
    prev, cur = [-1] * 6, [-1] * 6
    for j, t in enumerate(np.asarray(ids).tolist()):
        if mask is not None and not mask[j]:
            continue
        if t == spec.ts:
            seen, run, prev, cur = True, 0, [-1] * 6, [-1] * 6
        elif not seen:
            continue
        elif t == spec.tsep:
            prev = list(cur) if run == 6 else [-1] * 6
            run, cur = 0, [-1] * 6
        elif G.is_bin(spec, t):
            if run < 6:
                cur[run] = t - spec.p0
                run += 1
        else:
            run, cur = 0, [-1] * 6
    return tuple(prev + cur)


def allowed_limits(spec, state, pose, lim, rem):
    """The sorted ids allowed under the limits: G.allowed with its bin ids cut to the window of dimension = phase."""
    ids = G.allowed(spec, state, rem)
    phase = state[0]
    if not 0 <= phase <= 5 or not any(G.is_bin(spec, t) for t in ids):
        return ids
    a, b = window(int(lim[phase]), int(lim[6 + phase]), int(lim[12 + phase]), int(pose[phase]))
    return [t for t in ids if not G.is_bin(spec, t) or a <= t - spec.p0 <= b]


def mask_ref(spec, row, state, pose, lim, rem):
    out = np.array(row, copy=True)
    keep = np.zeros(out.shape[-1], dtype=bool)
    keep[allowed_limits(spec, state, pose, lim, rem)] = True
    out[..., ~keep] = -np.inf
    return out


def mass_ref(spec, row64, state, pose, lim, rem):
    """float64: the probability the row gives the set allowed under the limits."""
    x = np.asarray(row64, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max()
        e = np.exp(x - m)
        return float(e[allowed_limits(spec, state, pose, lim, rem)].sum() / e.sum())


def violations(spec, ids, lim, start=0):
    """The bin tokens of one sequence, at positions >= start, that lie outside their window: the table stepped token by token from
    phase 9 (state and pose by G.advance / pose_advance), a bin taken at phase 0 .. 5 held against the window of the pose before it."""
    state, pose, n = (9, 0), UNKNOWN + UNKNOWN, 0
    ids = [int(t) for t in np.asarray(ids).tolist()]
    last = max((j for j, t in enumerate(ids) if t == spec.ts), default=None)
    if last is None:
        return 0
    for j in range(last, len(ids)):
        t = ids[j]
        if t == spec.eos:
            break
        new = G.advance(spec, state, t)
        if G.is_bin(spec, t) and 0 <= state[0] <= 5 and new[0] == state[0] + 1 and j >= start:
            d = state[0]
            a, b = window(int(lim[d]), int(lim[6 + d]), int(lim[12 + d]), pose[d])
            n += not a <= t - spec.p0 <= b
        pose = pose_advance(spec, state, pose, t)
        state = new
    return n
