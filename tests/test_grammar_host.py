"""CPU: the trajectory grammar's transition table (tests/grammar_ref.py, the numpy restatement of csrc/grammar.hip) closes every row it
promises to close.

Exhaustive over every start state with steps <= 3, (min_steps, max_steps) in {(0, 0), (0, 3), (2, 2), (1, 3)} and every T from 1 to 40:
a walk that takes an allowed token at every step (always the first of the allowed set, always the last, alternating, and seeded random
picks) passes the strict validator whenever need(state) <= T.  And every prefix of a valid sequence is accepted by the table."""
import itertools
import random

import pytest

from egoscaler_amd import _abi
from tests import grammar_ref as G

LIMITS = ((0, 0), (0, 3), (2, 2), (1, 3))
PAD = 2


def spec_of(mn, mx):
    return G.Spec(p0=10, nb=4, ts=5, tsep=6, te=7, eos=8, min_steps=mn, max_steps=mx)


def walk(spec, state, T, pick):
    gen = []
    for t in range(T):
        ids = G.allowed(spec, state, T - t)
        assert ids, (state, T - t)
        tok = pick(t, ids)
        gen.append(tok)
        state = G.advance(spec, state, tok)
    return gen, state


PICKS = {"first": lambda t, ids: ids[0], "last": lambda t, ids: ids[-1], "alternate": lambda t, ids: ids[0] if t % 2 else ids[-1]}


@pytest.mark.parametrize("mn,mx", LIMITS)
def test_every_walk_from_every_state_closes(mn, mx):
    spec = spec_of(mn, mx)
    rnd = random.Random(7)
    picks = dict(PICKS, random=lambda t, ids: rnd.choice(ids))
    closed = 0
    for phase, steps in itertools.product(G.PHASES, range(4)):
        if phase == 9 and steps:
            continue
        state = (phase, steps)
        tail = G.state_prompt(spec, state)
        assert G.init_state(spec, [3, 3] + tail) == state or phase >= 7          # (a prompt never leaves phases 7 / 8: init reads no <te>)
        n = G.need(spec, state)
        for T in range(1, 41):
            if n > T:
                continue
            for name, pick in picks.items():
                gen, end = walk(spec, state, T, pick)
                assert G.valid(spec, tail, gen, pad=PAD), (state, T, name, gen)
                assert end[0] == 8 and mn <= end[1] <= mx, (state, T, name, end)
                closed += 1
    assert closed > 0


@pytest.mark.parametrize("mn,mx", LIMITS)
def test_need_is_the_shortest_close(mn, mx):
    """need(state) tokens suffice (the walk above), and need - 1 do not: no walk of that length reaches phase 8."""
    spec = spec_of(mn, mx)
    for phase, steps in itertools.product(G.PHASES, range(4)):
        n = G.need(spec, (phase, steps))
        if n == G.NEVER or n == 0 or (phase == 9 and steps):
            continue
        frontier = {(phase, steps)}
        for t in range(n - 1):
            frontier = {G.advance(spec, s, tok) for s in frontier for tok in G.allowed(spec, s, 1000)}
        assert all(s[0] != 8 for s in frontier), ((phase, steps), n)


def test_states_without_a_legal_close():
    spec = spec_of(1, 2)
    assert G.need(spec, (0, 3)) == G.NEVER and G.need(spec, (4, 2)) == G.NEVER and G.need(spec, (7, 0)) == G.NEVER
    assert G.need(spec, (0, 2)) == 2 and G.need(spec, (4, 1)) == 5 and G.need(spec, (9, 0)) == 10 and G.need(spec, (8, 1)) == 0


@pytest.mark.parametrize("mn,mx", LIMITS)
def test_every_prefix_of_a_valid_sequence_is_accepted(mn, mx):
    spec = spec_of(mn, mx)
    for n in range(mn, mx + 1):
        seq = [spec.ts] + ([spec.p0, spec.p0 + 3, spec.p0 + 1, spec.p0, spec.p0 + 2, spec.p0 + 3] + [spec.tsep]) * n + [spec.te, spec.eos]
        for extra in (0, 1, 5):                                                  # the loop may be longer than the sequence
            state, T = (9, 0), len(seq) + extra
            for t, tok in enumerate(seq):
                assert tok in G.allowed(spec, state, T - t), (n, t, tok, state)
                state = G.advance(spec, state, tok)
            assert state == (8, n)
            assert G.valid(spec, [], seq + [PAD] * extra, pad=PAD)
            for cut in range(len(seq)):                                          # and a prefix of it leaves the state its prompt scan gives
                if cut:
                    want = (9, 0)
                    for tok in seq[:cut]:
                        want = G.advance(spec, want, tok)
                    if want[0] < 7:
                        assert G.init_state(spec, seq[:cut]) == want, (n, cut)


def test_validator_refuses():
    spec = spec_of(1, 2)
    step = [10, 11, 12, 13, 10, 11, 6]
    ok = [5] + step + [7, 8]
    assert G.valid(spec, [], ok) and G.valid(spec, ok[:3], ok[3:] + [PAD, 8], pad=PAD)
    assert not G.valid(spec, [], [5, 7, 8])                                      # n = 0 < min_steps
    assert not G.valid(spec, [], [5] + step * 3 + [7, 8])                        # n = 3 > max_steps
    assert not G.valid(spec, [], [5] + step[:5] + [6, 7, 8])                     # a step of five bins
    assert not G.valid(spec, [], [5] + step + [7])                               # no eos
    assert not G.valid(spec, [], [5] + step + [8])                               # no <te>
    assert not G.valid(spec, [], ok + [11], pad=PAD)                             # a bin after the eos
    assert not G.valid(spec, [], step + [7, 8])                                  # no <ts>


def test_masked_prompt_positions_are_skipped():
    spec = spec_of(0, 3)
    ids = [5, 10, 11, 6, 5, 10, 3, 11]
    assert G.init_state(spec, ids) == (1, 0)                                     # the 3 ends the run of bins
    assert G.init_state(spec, ids, [1, 1, 1, 1, 0, 1, 0, 1]) == (2, 1)
    assert G.init_state(spec, [3, 3]) == (9, 0)


def test_entry_points_are_declared():
    for name in ("egomi_traj_grammar_init", "egomi_traj_grammar_step"):
        assert name in _abi.PROTOS
    assert _abi.EGOMI_GRAMMAR_NEVER == G.NEVER
