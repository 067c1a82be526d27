"""GPU: generate(traj_grammar=..., traj_limits=...) on the tiny model with seeded weights (16 bins): every returned row keeps the motion
limits, and exactly so.

The inputs are those of tests/test_gpu_grammar_generate.py (its fixture, by import): prompts cut after the first <tsep>, so the prompt
holds step 0 and the first generated step is already limited by it; min_steps = max_steps = 4.  The validator is
traj.limits_violations (pinned against tests/limits_ref.py on the CPU in tests/test_limits_host.py) and the strict grammar validator.
1. greedy, sampled, num_return_sequences = 4 with and without share_prompt, with per-prompt tables (dmax = 1, 2, 3 bins for the three
   prompts, so a wrong expansion to the K rows shows): 0 violations in every row, every row parses, limits_mass <= grammar_mass with
   0 after a row's eos -- and the grammar-only call on the same seed violates the same table (asserted first: on these weights the
   choice among 16 bins is near-uniform, so 18 bin tokens within 2 bins of their predecessors do not happen by chance).
2. the same decoder, another table (a box [3, 12] and dmax = 1): honoured, through the SAME graph (one graph key with "limits"); the
   first table again replays bit-equal.  Decoder.greedy(limits=...) keeps them too; beam() refuses.
3. step by step: a Decoder stepped eagerly under the limits gives, at every step, limits_ref's masked row, state and pose, bit for bit.
4. traj_limits absent: the launches of sample(grammar=spec) are those of sample() plus the init launch at the head and one
   egomi_traj_grammar_step directly before every token kernel, argument by argument (tests/decode_trace.py's recorder), none of the
   *_limits symbols; with the table the same positions hold the *_limits launches and nothing is added.  generate(traj_grammar=...) is
   bit-equal before and after a call with limits.
5. refusals: num_beams = 2, traj_limits without traj_grammar, a bad table.
Every test here needs the keyword, so every one fails without the feature."""
import numpy as np
import pytest
import torch

from egoscaler_amd import traj
from egoscaler_amd.decode import Decoder, argmax_rows, traj_grammar_init_limits, traj_grammar_step_limits
from egoscaler_amd.ops import dt
from tests import binstats_cases as BC
from tests import decode_trace as DT
from tests import grammar_ref as G
from tests import limits_ref as L
from tests.test_gpu_grammar_generate import B, T, all_valid, setup, tails  # noqa: F401  (setup: the module's fixture)

pytestmark = pytest.mark.gpu
DT_F32 = dt(torch.float32)                                               # the tiny model runs in fp32


def table(s, dmax=(1, 2, 3), lo=0, hi=None):
    nb = s.tok.num_bins
    return traj.motion_limits_bins(lo=lo, hi=nb - 1 if hi is None else hi, dmax=np.asarray(dmax)[:, None].repeat(6, 1), nb=nb, rows=B)


def viol(s, out, lim, K=1):
    return traj.limits_violations(out.sequences, s.tok, lim.repeat_interleave(K, 0), start=s.Lp)


def check_limited(s, out, lim, K, tag):
    v = viol(s, out, lim, K)
    assert v.tolist() == [0] * (B * K), (tag, v.tolist(), out.sequences[:, s.Lp:].tolist())
    ref = [L.violations(s.spec, row, l, start=s.Lp) for row, l in zip(out.sequences.cpu().numpy(), lim.repeat_interleave(K, 0).numpy())]
    assert ref == [0] * (B * K), (tag, ref)
    assert all(all_valid(s, out, tails(s, rep=K))), tag
    lm, gm = out.limits_mass, out.grammar_mass
    assert lm.shape == gm.shape == (B * K, len(out.scores)) and bool((lm <= gm).all()) and bool((lm >= 0).all())
    ends = (out.sequences[:, s.Lp:] == s.tok.eos).int().argmax(1).cpu().numpy()
    for r in range(B * K):
        assert bool((lm[r, ends[r] + 1:] == 0).all()) and bool((lm[r, :ends[r] + 1] > 0).all()), (tag, r)
    assert bool((lm < gm).any()), tag                                    # somewhere the limits cut mass the grammar allowed


def test_limited_rows_keep_the_limits_and_grammar_only_rows_do_not(setup):
    s = setup
    lim = table(s)
    for tag, kw, K in (("greedy", dict(do_sample=False), 1), ("sampled", dict(seed=11), 1),
                       ("K=4", dict(seed=12, num_return_sequences=4), 4), ("K=4 shared", dict(seed=12, num_return_sequences=4, share_prompt=True), 4)):
        free = s.m.generate(**s.inputs(traj_grammar=s.spec, **kw))
        assert free.limits_mass is None
        v = viol(s, free, lim, K)
        print(f"traj_limits {tag}: grammar-only violations per row {v.tolist()}")
        assert int((v > 0).sum()) >= 1, f"{tag}: the grammar-only rows all keep the limits: the inputs show nothing"
        check_limited(s, s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=lim, **kw)), lim, K, tag)


def limit_graphs(s):
    return [k for d in s.m._decoders.values() for k in getattr(d, "_graphs", {}) if "limits" in k]


def test_another_table_replays_the_same_graph(setup):
    s = setup
    kw = dict(seed=31, top_k=9)
    lim_a, lim_b = table(s, dmax=(2, 2, 2)), table(s, dmax=(1, 1, 1), lo=3, hi=12)
    first = s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=lim_a, **kw))
    check_limited(s, first, lim_a, 1, "table a")
    n0 = len([k for k in limit_graphs(s) if 9 in k[:6]])
    other = s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=lim_b, **kw))
    check_limited(s, other, lim_b, 1, "table b")
    assert int(viol(s, first, lim_b).sum()) > 0, "table b asks nothing table a's rows do not already keep"
    bins = other.sequences[:, s.Lp + 7:s.Lp + 13] - s.tok.p0              # the second generated step: from any bin 0 .. 15 of the prompt's step,
    assert bool(((bins >= 2) & (bins <= 13)).all())                      # two moves of dmax = 1 toward the box [3, 12] end in [2, 13]
    again = s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=lim_a, **kw))
    assert n0 == 1 and len([k for k in limit_graphs(s) if 9 in k[:6]]) == 1, limit_graphs(s)          # one capture served all three
    assert torch.equal(again.sequences, first.sequences) and torch.equal(again.limits_mass, first.limits_mass)
    assert torch.equal(again.grammar_mass, first.grammar_mass) and all(torch.equal(a, b) for a, b in zip(again.scores, first.scores))
    key = next(k for k in limit_graphs(s) if 9 in k[:6])
    assert key[key.index("grammar") + 1:] == tuple(s.spec) + ("limits",)  # one constant element beside the grammar's


def prefilled(s):
    kw = s.inputs()
    dec = Decoder(s.m.engine, B, s.Lp + T)
    dec.prefill(kw["input_ids"], kw["attention_mask"], kw["point_clouds"], kw["fps_start"].cuda(), T)
    return dec, kw


def test_decoder_greedy_takes_limits_and_beam_refuses(setup):
    s = setup
    lim = table(s)
    dec, _ = prefilled(s)
    seq, _ = dec.greedy(T, use_graph=False, keep_scores=False, grammar=s.spec, limits=lim)
    assert traj.limits_violations(seq, s.tok, lim, start=s.Lp).tolist() == [0] * B
    dec, _ = prefilled(s)
    free, _ = dec.greedy(T, use_graph=False, keep_scores=False, grammar=s.spec)
    assert int(traj.limits_violations(free, s.tok, lim, start=s.Lp).sum()) > 0
    with pytest.raises(ValueError, match="grammar"):
        dec.greedy(T, use_graph=False, limits=lim)
    with pytest.raises(ValueError, match="limits"):
        dec.beam(T, limits=lim)


def test_hand_driven_steps_are_the_restatement(setup):
    s = setup
    lim = table(s, dmax=(0, 1, 3), lo=2, hi=13)
    lim_h = lim.numpy()
    dec, kw = prefilled(s)
    state = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    need = torch.zeros(B, dtype=torch.int32, device="cuda")
    pose = torch.zeros(B, 12, dtype=torch.int32, device="cuda")
    mass, lmass = (torch.zeros(B, T, dtype=torch.float32, device="cuda") for _ in range(2))
    traj_grammar_init_limits(kw["input_ids"], kw["attention_mask"].to(torch.uint8), s.spec, state, need, pose)
    prompts = s.toks[:B, :s.Lp].numpy()
    ref = [G.init_state(s.spec, row) for row in prompts]
    rpose = [L.init_pose(s.spec, row) for row in prompts]
    assert state.tolist() == [list(r) for r in ref] == [[0, 1]] * B and pose.tolist() == [list(p) for p in rpose]
    assert all(min(p[:6]) >= 0 for p in rpose)                           # the prompt's step is known
    prev = None
    for t in range(T):
        raw = dec.lg.clone()
        traj_grammar_step_limits(dec.lg, None if t == 0 else dec.tok.view(-1), state, s.spec, T - t, mass, t, lim.cuda(), pose, lmass)
        if t:
            rpose = [L.pose_advance(s.spec, ref[r], rpose[r], prev[r]) for r in range(B)]
            ref = [G.advance(s.spec, ref[r], prev[r]) for r in range(B)]
        got, raw_h = dec.lg.cpu().numpy(), raw.cpu().numpy()
        for r in range(B):
            want = L.mask_ref(s.spec, raw_h[r], ref[r], rpose[r], lim_h[r], T - t)
            assert np.array_equal(got[r].view(np.int32), want.view(np.int32)), (t, r)
            m64 = L.mass_ref(s.spec, raw_h[r], ref[r], rpose[r], lim_h[r], T - t)
            assert BC.ratio([float(lmass[r, t])], [m64]) <= BC.BOUND["mass"], (t, r, float(lmass[r, t]), m64)      # the kernel test's bound
        assert state.tolist() == [list(r) for r in ref] and pose.tolist() == [list(p) for p in rpose], t
        argmax_rows(dec.lg, dec.tok.view(-1), dec.seq, s.Lp + t)
        prev = dec.tok.view(-1).cpu().numpy()
        if t + 1 < T:
            dec.step(s.Lp + t)
    hand = dec.seq[:, :s.Lp + T]
    assert traj.limits_violations(hand, s.tok, lim, start=s.Lp).tolist() == [0] * B
    out = s.m.generate(**s.inputs(do_sample=False, traj_grammar=s.spec, traj_limits=lim))
    n = out.sequences.shape[1]
    eos_at = (hand[:, s.Lp:] == s.tok.eos).int().argmax(1)
    for r in range(B):
        e = s.Lp + int(eos_at[r]) + 1
        assert torch.equal(out.sequences[r, :e], hand[r, :e]) and bool((out.sequences[r, e:n] == s.tok.pad).all()), r


def test_without_the_table_the_launches_are_the_grammars(setup):
    s = setup
    lim = table(s)
    kw = dict(eos=s.tok.eos, pad=s.tok.pad, seed=5, use_graph=False)
    extra = ("gr_state", "gr_need", "gr_mass", "gr_lim", "gr_pose", "gr_limits_mass")

    def run(**more):
        dec, _ = prefilled(s)
        with DT.trace() as rec:
            seq, _ = dec.sample(T, **kw, **more)
        named = DT.named_buffers(dec) + [(n, getattr(dec, n)) for n in extra if getattr(dec, n, None) is not None]
        return rec.resolved(named), seq.clone(), dec
    plain, _, _ = run()
    gram, seq_g, dec_g = run(grammar=s.spec)
    limd, seq_l, dec_l = run(grammar=s.spec, limits=lim)
    assert dec_g.gr_lim is None and dec_g.gr_pose is None and dec_g.gr_limits_mass is None
    is_gr = lambda l: l[0].startswith("egomi_traj_grammar")
    assert DT.first_difference([l for l in gram if not is_gr(l)], plain) is None
    assert DT.first_difference([l for l in limd if not is_gr(l)], plain) is None
    stream = None                                                        # the default stream, as every launch of `plain` records it
    sp = list(s.spec)
    R, V, ld_seq, ld_mask, ld_mass = B, dec_g.lg.shape[1], dec_g.seq_buf.stride(0), dec_g.mask_buf.stride(0), dec_g.gr_mass.stride(0)
    init = ["egomi_traj_grammar_init", ["seq_buf", 0], ld_seq, ["mask_buf", 0], ld_mask, R, s.Lp] + sp + [["gr_state", 0], ["gr_need", 0], stream]
    step = lambda t: (["egomi_traj_grammar_step", ["lg", 0], V, R, V, None if t == 0 else ["tok", 0], ["gr_state", 0]] + sp
                      + [T - t, ["gr_mass", 0], ld_mass, t, DT_F32, stream])
    want, t = [init], 0
    for l in plain:                                                      # one step launch directly before every token kernel
        if l[0] == "egomi_sample_rows":
            want.append(step(t))
            t += 1
        want.append(l)
    assert t == T and DT.first_difference(gram, want) is None
    init_l = ["egomi_traj_grammar_init_limits"] + init[1:-1] + [["gr_pose", 0], stream]
    step_l = lambda t: (["egomi_traj_grammar_step_limits"] + step(t)[1:-2] + [["gr_lim", 0], ["gr_pose", 0], ["gr_limits_mass", 0], DT_F32, stream])
    want_l, t = [init_l], 0
    for l in plain:
        if l[0] == "egomi_sample_rows":
            want_l.append(step_l(t))
            t += 1
        want_l.append(l)
    assert DT.first_difference(limd, want_l) is None and len(limd) == len(gram)
    assert int(traj.limits_violations(seq_l, s.tok, lim, start=s.Lp).sum()) == 0 < int(traj.limits_violations(seq_g, s.tok, lim, start=s.Lp).sum())
    # generate(traj_grammar=...) before and after a call with limits: bit-equal, and under its own graph key
    gk = dict(seed=21, top_k=7, traj_grammar=s.spec)
    before = s.m.generate(**s.inputs(**gk))
    s.m.generate(**s.inputs(traj_limits=lim, **gk))
    after = s.m.generate(**s.inputs(**gk))
    assert before.limits_mass is None and after.limits_mass is None
    assert torch.equal(before.sequences, after.sequences) and torch.equal(before.grammar_mass, after.grammar_mass)
    assert all(torch.equal(a, b) for a, b in zip(before.scores, after.scores))
    keys = [k for d in s.m._decoders.values() for k in getattr(d, "_graphs", {}) if 7 in k[:6] and "grammar" in k]
    assert sorted(len(k) - k.index("grammar") for k in keys) == [1 + len(s.spec), 2 + len(s.spec)], keys


def test_refusals(setup):
    s = setup
    lim = table(s)
    with pytest.raises(ValueError, match="num_beams"):
        s.m.generate(**s.inputs(num_beams=2, do_sample=False, traj_grammar=s.spec, traj_limits=lim))
    with pytest.raises(ValueError, match="traj_grammar"):
        s.m.generate(**s.inputs(traj_limits=lim))
    bad = lim.clone()
    bad[1, 3], bad[1, 9] = 5, 4                                          # lo > hi
    with pytest.raises(ValueError, match="lo <= hi"):
        s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=bad))
    with pytest.raises(ValueError, match="traj_limits"):
        s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=lim[:2]))
    with pytest.raises(ValueError, match="traj_limits"):
        s.m.generate(**s.inputs(traj_grammar=s.spec, traj_limits=lim.cuda()))
    with pytest.raises(ValueError, match="traj_limits"):
        s.m.generate(**s.inputs(seed=3, num_return_sequences=4, traj_grammar=s.spec, traj_limits=lim.repeat_interleave(4, 0)))   # one row per PROMPT
