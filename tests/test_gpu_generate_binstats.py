"""GPU: generate(output_bin_stats=True) / score(output_bin_stats=True) on the tiny model (B = 2, K = 4, T = 8, fp32): the per-step statistics
of the raw distribution over the waypoint bins (egomi_bin_stats inside the token loop), and the driver's --soft_decode.
  * the option changes no existing field (sampled and greedy, dense and shared prompt, with and without output_logprobs), has a graph of
    its own, and the graph's results equal the eager steps' bit for bit
  * bin_*[:, t] against egomi_bin_stats on the raw logits of model.forward() on the returned sequences (teacher forcing),
    |got - ref| <= 2 * REL * max|logits|: the bound tests/test_gpu_generate_logprobs.py holds token_logprobs to in the same comparison
  * the arg-max bin of a greedy row against bin_mean where bin_mass > 0.99 (a sanity property)
  * score() on the sequences of a shared-prompt run against that run's statistics (tests/test_gpu_score.py's bound between the two paths),
    zeros after each eos
  * fp8 KV cache, int4 decode weights, the refusals, and the driver."""
import json
import os

import numpy as np
import pytest
import torch

from egoscaler_amd import traj as TR
from egoscaler_amd.decode import bin_stats_rows
from tests.test_gpu_best_of_k import PLAIN, REL, SEED, _kw, _tiny_model

pytestmark = pytest.mark.gpu
K, T = 4, 8
STATS = ("bin_mass", "bin_mean", "bin_std", "bin_entropy")
OLD = ("sequences", "token_logprobs", "sequences_logprobs", "sequences_lengths", "sample_scores", "rank")


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _bins(dims):
    return (dims.tok.p0, dims.tok.num_bins)


def _same(a, b, fields):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        assert x is None or torch.equal(x, y), f
    assert len(a.scores) == len(b.scores) and all(torch.equal(p, q) for p, q in zip(a.scores, b.scores))


def _forward_stats(m, dims, out, masks, Lp, pts, k, t_new):
    """egomi_bin_stats on the raw logits of model.forward() on the returned sequences: -> ({field: [rows, t_new]}, max|logits|)."""
    seq = out.sequences
    am = torch.cat([masks[:, :Lp].cuda().repeat_interleave(k, 0), torch.ones(seq.shape[0], t_new, dtype=masks.dtype, device="cuda")], 1)
    with torch.no_grad():
        lg = m(input_ids=seq, attention_mask=am, point_clouds=pts.cuda().repeat_interleave(k, 0),
               fps_start=torch.tensor([0, 17]).repeat_interleave(k)).logits
    lg = lg[:, Lp - 1:Lp - 1 + t_new].float().contiguous()
    p0, nb = _bins(dims)
    ref = [torch.zeros(seq.shape[0], t_new, dtype=torch.float32, device="cuda") for _ in STATS]
    values = TR.bin_edges(nb, "cuda")
    for t in range(t_new):
        bin_stats_rows(lg[:, t], p0, nb, values, *ref, t)
    return dict(zip(STATS, ref)), float(lg.abs().max())


@pytest.mark.parametrize("share", [True, False], ids=["shared", "dense"])
@pytest.mark.parametrize("sample", [True, False], ids=["sampled", "greedy"])
def test_option_leaves_every_existing_field_bit_equal_and_matches_teacher_forcing(tiny, sample, share):
    m, dims, toks, masks, Lp, pts = tiny
    mode = dict(PLAIN, seed=SEED) if sample else dict(do_sample=False, eos_token_id=None)
    kw = dict(_kw(toks, masks, Lp, pts, T), **mode, num_return_sequences=K, share_prompt=share)
    on = dict(output_bin_stats=True, bin_token_ids=_bins(dims))
    base, out = m.generate(**kw), m.generate(**kw, **on)
    _same(base, out, OLD)
    assert all(getattr(base, f) is None for f in STATS) and out.token_logprobs is None
    base_lp, out_lp = m.generate(**kw, output_logprobs=True), m.generate(**kw, output_logprobs=True, **on)
    _same(base_lp, out_lp, OLD)
    assert out_lp.token_logprobs is not None and torch.equal(out_lp.sequences, out.sequences)
    ref, mx = _forward_stats(m, dims, out, masks, Lp, pts, K, T)
    for f in STATS:
        got = getattr(out, f)
        assert got.shape == (2 * K, T) and got.dtype == torch.float32 and torch.equal(got, getattr(out_lp, f)), f
        err = float((got.double() - ref[f].double()).abs().max())
        print(f"generate bin stats tiny fp32 sample={sample} share={share}: {f} worst |got - ref| {err:.3e}, bound {2 * REL * mx:.3e}")
        assert err <= 2 * REL * mx, f
    assert bool((out.bin_mass > 0).all()) and bool((out.bin_mass < 1).all()) and bool((out.bin_mean.abs() <= 1).all())
    assert bool((out.bin_std >= 0).all()) and bool((out.bin_std <= 1).all())
    assert bool((out.bin_entropy >= 0).all()) and bool((out.bin_entropy <= np.log(dims.tok.num_bins) + 1e-5).all())


def test_graph_equals_eager_and_the_option_has_a_graph_of_its_own(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED)
    on = dict(output_bin_stats=True, bin_token_ids=_bins(dims))
    m.__dict__.pop("_decoders", None)
    plain = m.generate(**kw)
    dec = list(m._decoders.values())[-1]
    assert len(dec._graphs) == 1 and dec.bs_mass is None               # decoders that never ask hold no statistics buffers
    a = m.generate(**kw, **on)
    assert len(dec._graphs) == 2
    e = m.generate(**kw, **on, use_graph=False)
    c = m.generate(**kw, **on)                                         # replays the cached graph
    assert len(dec._graphs) == 2
    for x in (e, c):
        _same(a, x, OLD + STATS)
    both = m.generate(**kw, **on, output_logprobs=True)                # with the log-probs: a third graph, the same statistics
    assert len(dec._graphs) == 3
    _same(a, both, ("sequences",) + STATS)
    other = m.generate(**kw, output_bin_stats=True, bin_token_ids=(dims.tok.p0, dims.tok.num_bins - 1))    # another window is another graph
    assert len(dec._graphs) == 4 and not torch.equal(other.bin_mass, a.bin_mass)
    again = m.generate(**kw)                                           # the first graph is undisturbed
    _same(plain, again, OLD)
    from egoscaler_amd.decode import Decoder                           # Decoder.greedy(bin_stats=...): generate()'s greedy numbers
    g = m.generate(**dict(_kw(toks, masks, Lp, pts, 6), do_sample=False, eos_token_id=None), **on)
    d2 = Decoder(m.engine, 2, Lp + 6)
    d2.prefill(toks[:, :Lp].cuda(), masks[:, :Lp].cuda(), pts.cuda(), [0, 17], 6)
    seq, _ = d2.greedy(6, use_graph=True, keep_scores=False, bin_stats=_bins(dims))
    assert torch.equal(seq, g.sequences)
    for f, buf in zip(STATS, (d2.bs_mass, d2.bs_mean, d2.bs_std, d2.bs_ent)):
        assert torch.equal(buf[:, :6], getattr(g, f)), f


def _bin_heavy_model():
    """The tiny model with an lm_head that speaks bins only: the rows of every other token zeroed, the bin rows eight times as large.  On the
    seeded Gaussian head a step puts about 5 % of its mass on the 16 bins; here nearly all of it."""
    m, dims, toks, masks, Lp, pts = _tiny_model()
    p0, nb = _bins(dims)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    head = sd["lm_head.weight"]
    keep = 8.0 * head[p0:p0 + nb]
    head.zero_()
    head[p0:p0 + nb] = keep
    m.load_state_dict(sd)
    return m.eval(), dims, toks, masks, Lp, pts


@pytest.mark.parametrize("model", [_tiny_model, _bin_heavy_model], ids=["gaussian_head", "bin_head"])
def test_greedy_argmax_bin_lies_near_the_mean_where_the_mass_is_on_the_bins(model):
    m, dims, toks, masks, Lp, pts = model()
    p0, nb = _bins(dims)
    out = m.generate(**dict(_kw(toks, masks, Lp, pts, T), do_sample=False, eos_token_id=None), output_bin_stats=True, bin_token_ids=(p0, nb))
    lg = torch.stack(out.scores, 1)                                    # greedy scores are the raw logits [rows, T, V]
    best = lg[:, :, p0:p0 + nb].argmax(2)
    v = TR.bin_edges(nb, "cuda")[best].float()
    sure = out.bin_mass > 0.99
    near = (v - out.bin_mean).abs() <= torch.maximum(out.bin_std, torch.full_like(out.bin_std, 2.0 / (nb - 1)))
    print(f"greedy bin stats: {int(sure.sum())} of {sure.numel()} steps put more than 0.99 of their mass on the bins")
    assert bool(near[sure].all())
    if model is _bin_heavy_model:                                      # there the property is not vacuous, and the greedy token is that bin
        assert int(sure.sum()) >= sure.numel() // 2
        assert torch.equal(out.sequences[:, Lp:][sure], (p0 + best)[sure])
    mass =torch.softmax(lg.double(), 2)[:, :, p0:p0 + nb].sum(2)      # and the mass is the softmax's mass on the window
    assert float((out.bin_mass.double() - mass).abs().max()) <= 1e-5


def test_score_gives_the_statistics_of_the_run_that_sampled(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    on = dict(output_bin_stats=True, bin_token_ids=_bins(dims))
    kw = dict(_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED)
    gen = m.generate(**kw, **on)
    skw = _kw(toks, masks, Lp, pts, 0)
    del skw["max_length"]
    cand = gen.sequences[:, Lp:].reshape(2, K, T)
    plain = m.score(**skw, candidates=cand, eos_token_id=None)
    sc = m.score(**skw, candidates=cand, eos_token_id=None, **on)
    _same(plain, sc, OLD)
    assert all(getattr(plain, f) is None for f in STATS)
    mx = float(torch.stack(gen.scores).abs().max())                    # PLAIN: the processed scores are the raw logits
    bound = 2 * REL * mx
    for f in STATS:
        got = getattr(sc, f)
        assert got.shape == (2, K, T) and got.dtype == torch.float32, f
        err = float((got.reshape(2 * K, T) - getattr(gen, f)).abs().max())
        print(f"score bin stats tiny fp32: {f} |score - generate| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f
    one = m.score(**skw, candidates=cand, eos_token_id=None, row_budget=1, **on)      # one clip per pass: the same launches on smaller chunks
    for f in STATS:
        assert float((getattr(one, f) - getattr(sc, f)).abs().max()) <= bound, f
    eos = int(cand[0, 0, 2])                                           # a token the run did emit: row 0 ends at step 2 or earlier
    cut = m.score(**skw, candidates=cand, eos_token_id=eos, **on)
    lens = cut.sequences_lengths.long()
    assert int(lens[0]) <= 3
    after = (torch.arange(T, device="cuda")[None, :] >= lens[:, None]).reshape(2, K, T)
    for f in STATS:                                                    # zeros from the eos on; before it the run without an eos
        assert bool((getattr(cut, f)[after] == 0).all()), f
        assert float((getattr(cut, f)[~after] - getattr(sc, f)[~after]).abs().max()) <= bound, f
    assert bool(after.any()) and bool((cut.bin_mass[~after] > 0).all())
    gcut = m.generate(**{**kw, "eos_token_id": eos, "pad_token_id": int(dims.tok.pad)}, **on)      # generate() cuts at the eos the same way
    from egoscaler_amd.decode import candidate_lengths
    glen = candidate_lengths(gcut.sequences[:, Lp:], eos).long()
    gafter = torch.arange(gcut.bin_mass.shape[1], device="cuda")[None, :] >= glen[:, None]
    assert bool(gafter.any()) and all(bool((getattr(gcut, f)[gafter] == 0).all()) for f in STATS) and bool((gcut.bin_mass[~gafter] > 0).all())


@pytest.mark.parametrize("extra", [dict(kv_cache_dtype="fp8"), dict(decode_weight_dtype="int4")], ids=["fp8_cache", "int4_weights"])
def test_bf16_fp8_cache_and_int4_weights(extra):
    m, dims, toks, masks, Lp, pts = _tiny_model(torch.bfloat16)
    kw = dict(_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=2, seed=SEED, output_bin_stats=True, bin_token_ids=_bins(dims), **extra)
    a, e = m.generate(**kw), m.generate(**kw, use_graph=False)
    for f in STATS:
        got = getattr(a, f)
        assert got.shape == (4, T) and bool(torch.isfinite(got).all()), f
    _same(a, e, ("sequences",) + STATS)
    assert bool((a.bin_mass > 0).all()) and bool((a.bin_mass < 1).all())


def test_refusals(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, 4), eos_token_id=None)
    with pytest.raises(ValueError, match="num_beams == 1"):
        m.generate(**kw, num_beams=2, output_bin_stats=True, bin_token_ids=_bins(dims))
    with pytest.raises(ValueError, match="bin_token_ids"):
        m.generate(**kw, output_bin_stats=True)
    V = dims.lm.vocab_size
    for bad in ((V - 3, 4), (-1, 4), (0, 0), (0, 1025), (V, 1), "ab", (1, 2, 3)):
        with pytest.raises(ValueError, match="bin_token_ids"):
            m.generate(**kw, output_bin_stats=True, bin_token_ids=bad)
    skw = _kw(toks, masks, Lp, pts, 0)
    del skw["max_length"]
    cand = torch.zeros(2, 1, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="bin_token_ids"):
        m.score(**skw, candidates=cand, output_bin_stats=True)
    with pytest.raises(ValueError, match="bin_token_ids"):
        m.score(**skw, candidates=cand, output_bin_stats=True, bin_token_ids=(V - 3, 4))
    out = m.generate(**kw, bin_token_ids=_bins(dims))                  # the tuple alone asks for nothing
    assert out.bin_mass is None


# ------------------------------------------------------------------------------------------------ driver
ARGV = ["eval", "--tiny", "--num_samples", "4", "--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5", "--max_traj_token", "48"]
BASE_KEYS = {"ADE", "FDE", "ADE_as_called", "GD", "n", "minADE", "minFDE", "n_min", "K"}
SOFT_KEYS = {"ADE_soft", "FDE_soft", "n_soft", "sigma_mean", "bin_mass_min"}


def _eval(tmp, capsys, extra, argv=ARGV):
    from egoscaler_amd import driver
    os.makedirs(tmp, exist_ok=True)
    torch.manual_seed(3)
    driver.main(argv + ["--out_dir", tmp] + extra)
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return rec, json.load(open(os.path.join(tmp, "test_gen_trajs.json")))


def test_driver_soft_decode_adds_exactly_its_keys(tmp_path, capsys):
    rec0, dump0 = _eval(str(tmp_path / "plain"), capsys, [])
    rec1, dump1 = _eval(str(tmp_path / "soft"), capsys, ["--soft_decode"])
    assert set(rec0) == BASE_KEYS and set(rec1) == BASE_KEYS | SOFT_KEYS
    assert json.dumps(rec0, sort_keys=True) == json.dumps({k: rec1[k] for k in rec0}, sort_keys=True)
    soft = dump1.pop("soft")
    assert dump0 == dump1 and "soft" not in dump0
    assert rec1["n_soft"] == rec1["n"] == len(soft) == 4 and set(soft) == set(dump1)
    for i, entry in soft.items():
        assert set(entry) == {"mean", "std"}
        mean, std = np.array(entry["mean"]), np.array(entry["std"])
        assert mean.shape == std.shape == (5, 6) and np.isfinite(mean).all() and (std >= 0).all()
        assert (std[0] == 0).all()                                     # the step the prompt holds is known
        assert np.array(dump1[i][0]).shape == mean.shape               # beside sample 0's hard trajectory, step for step
    assert rec1["ADE_soft"] >= 0 and rec1["FDE_soft"] >= 0 and rec1["sigma_mean"] >= 0 and 0 <= rec1["bin_mass_min"] <= 1
    greedy = ["eval", "--tiny", "--val_greedy", "--dtype", "fp32", "--bs", "2", "--n_val", "2", "--num_steps", "5", "--max_traj_token", "48"]
    rec2, dump2 = _eval(str(tmp_path / "greedy"), capsys, ["--soft_decode"], greedy)
    assert set(rec2) == {"ADE", "FDE", "ADE_as_called", "GD", "n"} | SOFT_KEYS and set(dump2["soft"]) == set(dump2) - {"soft"}
    from egoscaler_amd import driver
    with pytest.raises(SystemExit):
        driver.parse_args(greedy + ["--soft_decode", "--num_beams", "2"])


def test_driver_one_hot_statistics_give_the_hard_metrics(tmp_path, capsys, monkeypatch):
    from egoscaler_amd.config import dims_tiny
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    tok = dims_tiny().tok
    real = TrajPointLLMForCausalLM.generate

    def one_hot(self, *a, **kw):
        out = real(self, *a, **kw)
        gen = out.sequences[:, out.sequences.shape[1] - out.bin_mean.shape[1]:]
        isbin = (gen >= tok.p0) & (gen < tok.p0 + tok.num_bins)
        centre = TR.bin_edges(tok.num_bins, gen.device)[(gen - tok.p0).clamp(0, tok.num_bins - 1)].float()
        out.bin_mean = torch.where(isbin, centre, out.bin_mean)
        out.bin_std = torch.zeros_like(out.bin_std)
        return out
    monkeypatch.setattr(TrajPointLLMForCausalLM, "generate", one_hot)
    rec, dump = _eval(str(tmp_path / "onehot"), capsys, ["--soft_decode"])
    assert rec["n_soft"] == rec["n"] > 0
    assert rec["ADE_soft"] == rec["ADE"] and rec["FDE_soft"] == rec["FDE"] and rec["sigma_mean"] == 0.0
    for i, entry in dump["soft"].items():
        assert entry["mean"] == dump[i][0]                             # the soft trajectory is sample 0's hard one
