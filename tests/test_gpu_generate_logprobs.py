"""GPU: generate(output_logprobs=True) on the tiny model: the per-token log-probs of the RAW distribution (egomi_token_logprob inside the
token loop), their per-sequence sums and lengths, the per-clip ranking (egomi_seq_rank), and the driver's --select.
  * fp32, sampled, K = 4, T = 8, shared prompt and expanded: token_logprobs against float64 log_softmax of model.forward() on the returned
    sequences (teacher forcing), |got - ref| <= 2 * REL * max|logits| (REL = 1e-3, the bar tests/test_gpu_best_of_k.py holds the scores
    to: both the chosen logit and the log-sum-exp move by at most the logits' error)
  * the reference's default sampling: the log-probs are those of the raw logits, not of the processed scores
  * eos bookkeeping, flag on / off bit-equality of every existing field, graph == eager, a second graph beside the first, the ranking rule,
    beams rejected, bf16 + fp8 cache + fp8 weights, LoRA, and the driver."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_best_of_k import PLAIN, REL, SEED, _kw, _tiny_model

pytestmark = pytest.mark.gpu
K, T = 4, 8


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _forward_logprobs(m, out, masks, Lp, pts, k, t_new):
    """float64 log_softmax of model.forward() on the returned sequences at positions Lp - 1 + t, gathered at the generated tokens:
    -> (ref [rows, t_new], max|logits|)."""
    seq = out.sequences
    am = torch.cat([masks[:, :Lp].cuda().repeat_interleave(k, 0), torch.ones(seq.shape[0], t_new, dtype=masks.dtype, device="cuda")], 1)
    with torch.no_grad():
        lg = m(input_ids=seq, attention_mask=am, point_clouds=pts.cuda().repeat_interleave(k, 0),
               fps_start=torch.tensor([0, 17]).repeat_interleave(k)).logits
    lg = lg[:, Lp - 1:Lp - 1 + t_new].double()
    ref = torch.log_softmax(lg, -1).gather(2, seq[:, Lp:Lp + t_new, None]).squeeze(2)
    return ref, float(lg.abs().max())


def _rank_ref(sums, lens, k, lp):
    s, n = sums.cpu().numpy().astype(np.float32).reshape(-1, k), lens.cpu().numpy().reshape(-1, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(n > 0, s / np.power(n.astype(np.float32), np.float32(lp)), -np.inf).astype(np.float32)
    order = np.stack([np.lexsort((np.arange(k), -score[b].astype(np.float64))) for b in range(score.shape[0])]).astype(np.int32)
    return score, order


@pytest.mark.parametrize("share", [True, False], ids=["shared", "expanded"])
def test_token_logprobs_match_teacher_forcing(tiny, share):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=share, seed=SEED)
    out = m.generate(**kw, output_logprobs=True)
    assert out.token_logprobs.shape == (2 * K, T) and out.token_logprobs.dtype == torch.float32
    assert out.sequences_logprobs.shape == (2 * K,) and out.sequences_lengths.dtype == torch.int32
    ref, mx = _forward_logprobs(m, out, masks, Lp, pts, K, T)
    err = float((out.token_logprobs.double() - ref).abs().max())
    print(f"generate logprobs tiny fp32 share={share}: worst |got - ref| {err:.3e}, bound {2 * REL * mx:.3e} (max|logits| {mx:.3f})")
    assert err <= 2 * REL * mx
    assert bool((out.token_logprobs < 0).all())
    acc = torch.zeros(2 * K, dtype=torch.float32, device="cuda")
    for t in range(T):
        acc = acc + out.token_logprobs[:, t]
    assert torch.equal(acc, out.sequences_logprobs)                    # the row sums, in step order
    assert bool((out.sequences_lengths == T).all())
    base = m.generate(**kw)                                            # the same seeded call without the flag: every existing field bit-equal
    assert torch.equal(base.sequences, out.sequences) and all(torch.equal(a, b) for a, b in zip(base.scores, out.scores))
    assert base.token_logprobs is None and base.rank is None
    score, order = _rank_ref(out.sequences_logprobs, out.sequences_lengths, K, 1.0)
    assert out.sample_scores.shape == (2, K) and out.rank.shape == (2, K) and out.rank.dtype == torch.int32
    assert np.array_equal(out.sample_scores.cpu().numpy(), score) and np.array_equal(out.rank.cpu().numpy(), order)
    by_sum = m.generate(**kw, output_logprobs=True, rank_length_penalty=0)
    assert torch.equal(by_sum.sample_scores.view(-1), by_sum.sequences_logprobs)
    assert np.array_equal(by_sum.rank.cpu().numpy(), _rank_ref(by_sum.sequences_logprobs, by_sum.sequences_lengths, K, 0.0)[1])


def test_default_sampling_reports_the_raw_distribution(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    out = m.generate(**_kw(toks, masks, Lp, pts, T), num_return_sequences=K, share_prompt=True, seed=SEED, eos_token_id=None,
                     output_logprobs=True)                             # top-k 50, top-p 0.95, temperature 1.0
    sc = torch.stack(out.scores, 1)                                    # [rows, T, V] processed
    tok = out.sequences[:, Lp:, None]
    chosen = sc.gather(2, tok).squeeze(2)
    assert bool(torch.isinf(sc).any()) and bool(torch.isfinite(chosen).all())
    assert bool(torch.isfinite(out.token_logprobs).all())             # finite where the scores are
    proc = torch.log_softmax(sc.double(), -1).gather(2, tok).squeeze(2)
    diff = proc - out.token_logprobs.double()                          # the processed row has lost mass: its log-probs are higher
    assert float(diff.min()) > -1e-4 and float(diff.max()) > 1e-3
    ref, mx = _forward_logprobs(m, out, masks, Lp, pts, K, T)
    assert float((out.token_logprobs.double() - ref).abs().max()) <= 2 * REL * mx


def test_eos_lengths_and_zero_columns(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, T), **{**PLAIN, "eos_token_id": None}, num_return_sequences=K, share_prompt=True, seed=SEED)
    free = m.generate(**kw, output_logprobs=True)
    gen = free.sequences[:, Lp:]
    eos = int(gen[0, 2])                                               # a token the seeded run does emit: row 0 at step 2 (or earlier)
    pad = int(dims.tok.pad)
    for pad_id in (pad if pad != eos else pad + 1, eos):               # and with pad == eos
        out = m.generate(**{**kw, "eos_token_id": eos, "pad_token_id": pad_id}, output_logprobs=True)
        g = out.sequences[:, Lp:]
        Tc = g.shape[1]
        hit = g == eos
        first = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full((2 * K,), Tc, device="cuda"))
        assert int(first[0]) <= 3 and int(first.min()) < Tc            # some row did finish early
        assert torch.equal(out.sequences_lengths.long(), first)
        cols = torch.arange(Tc, device="cuda")[None, :]
        after = cols >= first[:, None]
        assert bool((out.token_logprobs[after] == 0).all()) and bool((out.token_logprobs[~after] < 0).all())
        assert bool((g[after] == pad_id).all())
        same = ~after & (cols < int(first.min()))                      # until the first row finishes the run is the free run
        assert torch.equal(out.token_logprobs[:, :int(first.min())], free.token_logprobs[:, :int(first.min())]) and bool(same.any())
        acc = torch.zeros(2 * K, dtype=torch.float32, device="cuda")
        for t in range(Tc):
            acc = acc + out.token_logprobs[:, t]
        assert torch.equal(acc, out.sequences_logprobs)
        score, order = _rank_ref(out.sequences_logprobs, out.sequences_lengths, K, 1.0)
        assert np.array_equal(out.rank.cpu().numpy(), order)


def test_greedy_flag_leaves_sequences_and_scores_bit_equal(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, 6), do_sample=False, eos_token_id=None)
    a, b = m.generate(**kw), m.generate(**kw, output_logprobs=True)
    assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    ref = torch.log_softmax(torch.stack(b.scores, 1).double(), -1).gather(2, b.sequences[:, Lp:, None]).squeeze(2)
    assert float((b.token_logprobs.double() - ref).abs().max()) < 1e-5      # greedy scores are the raw logits: the arg-max's log-prob
    assert b.sample_scores is None and b.rank is None and bool((b.sequences_lengths == 6).all())
    from egoscaler_amd.decode import Decoder                           # Decoder.greedy(logprobs=True): the same numbers
    dec = Decoder(m.engine, 2, Lp + 6)
    dec.prefill(kw["input_ids"], kw["attention_mask"], kw["point_clouds"], kw["fps_start"], 6)
    seq, _ = dec.greedy(6, use_graph=True, keep_scores=False, logprobs=True)
    assert torch.equal(seq, b.sequences) and torch.equal(dec.lp_tok[:, :6], b.token_logprobs) and torch.equal(dec.lp_sum, b.sequences_logprobs)


def test_graph_equals_eager_and_the_flag_has_a_graph_of_its_own(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    kw = dict(_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED)
    m.__dict__.pop("_decoders", None)
    plain = m.generate(**kw)
    dec = list(m._decoders.values())[-1]
    assert len(dec._graphs) == 1 and getattr(dec, "lp_tok", None) is None     # decoders that never ask hold no log-prob buffers
    a = m.generate(**kw, output_logprobs=True)
    assert len(dec._graphs) == 2
    e = m.generate(**kw, output_logprobs=True, use_graph=False)
    c = m.generate(**kw, output_logprobs=True)                         # replays the cached graph
    assert len(dec._graphs) == 2
    for x in (e, c):
        assert torch.equal(a.sequences, x.sequences) and all(torch.equal(p, q) for p, q in zip(a.scores, x.scores))
        assert torch.equal(a.token_logprobs, x.token_logprobs) and torch.equal(a.sequences_logprobs, x.sequences_logprobs)
        assert torch.equal(a.sequences_lengths, x.sequences_lengths) and torch.equal(a.rank, x.rank)
    again = m.generate(**kw)                                           # the first graph is undisturbed
    assert len(dec._graphs) == 2
    assert torch.equal(plain.sequences, again.sequences) and all(torch.equal(p, q) for p, q in zip(plain.scores, again.scores))
    assert torch.equal(plain.sequences, a.sequences)


def test_beams_are_rejected(tiny):
    m, dims, toks, masks, Lp, pts = tiny
    with pytest.raises(ValueError, match="sequences_scores"):
        m.generate(**_kw(toks, masks, Lp, pts, 4), num_beams=2, output_logprobs=True, eos_token_id=None)


def test_bf16_fp8_cache_and_fp8_weights():
    m, dims, toks, masks, Lp, pts = _tiny_model(torch.bfloat16)
    out = m.generate(**_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=2, seed=SEED, kv_cache_dtype="fp8", decode_weight_dtype="fp8",
                     output_logprobs=True)
    assert out.token_logprobs.shape == (4, T) and bool(torch.isfinite(out.token_logprobs).all()) and bool((out.token_logprobs < 0).all())
    assert bool((out.sequences_lengths == T).all()) and bool(torch.isfinite(out.sample_scores).all())
    assert sorted(out.rank[0].tolist()) == [0, 1]


def test_lora_adapters():
    from egoscaler_amd import lora
    m, dims, toks, masks, Lp, pts = _tiny_model(lora_r=8, lora_alpha=16.0, lora_target_modules=",".join(lora.TARGETS))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B.weight"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    m.load_state_dict(m.state_dict())
    out = m.generate(**_kw(toks, masks, Lp, pts, T), **PLAIN, num_return_sequences=K, share_prompt=True, seed=SEED, output_logprobs=True)
    ref, mx = _forward_logprobs(m, out, masks, Lp, pts, K, T)
    assert float((out.token_logprobs.double() - ref).abs().max()) <= 2 * REL * mx


# ------------------------------------------------------------------------------------------------ driver
ARGV = ["eval", "--tiny", "--num_samples", "4", "--dtype", "fp32", "--bs", "2", "--n_val", "4", "--num_steps", "5", "--max_traj_token", "48"]


def _eval(tmp, capsys, extra):
    from egoscaler_amd import driver
    os.makedirs(tmp, exist_ok=True)
    torch.manual_seed(3)
    driver.main(ARGV + ["--out_dir", tmp] + extra)
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return rec, json.load(open(os.path.join(tmp, "test_gen_trajs.json")))


def _clip_ades(dump):
    """Per image id: the ADE of each of the K dumped trajectories against the split's ground truth (NaN for an unparsed one)."""
    from egoscaler_amd import driver, traj as TR
    from egoscaler_amd.config import dims_tiny
    a = driver.parse_args(ARGV)
    data = driver.make_data(a, dims_tiny(), None, a.split, TR.TargetNorm(a.do_norm, a.do_standard), a.n_val, 977)
    batch = data.batch(list(range(a.n_val)), torch.device("cuda"), a.max_traj_token)
    gt, ids = batch["trajectories"], batch["image_ids"].cpu().tolist()
    res = {}
    for b, i in enumerate(ids):
        ades = []
        for tr in dump[str(int(i))]:
            if tr is None:
                ades.append(float("nan"))
            else:
                g = torch.tensor(tr, dtype=torch.float32, device="cuda")[None]
                ades.append(float(TR.metrics_batch(g, None, gt[b:b + 1])[0][0]))
        res[str(int(i))] = ades
    return res


@pytest.mark.parametrize("mode", ["logprob", "medoid"])
def test_driver_select(tmp_path, capsys, mode):
    rec, dump = _eval(str(tmp_path / mode), capsys, ["--select", mode])
    assert {"ADE_sel", "FDE_sel", "n_sel", "select", "minADE", "minFDE", "K"} <= set(rec) and rec["select"] == mode
    sel = dump.pop("selected")
    assert len(dump) == 4 and set(sel) == set(dump)
    ades, picked = _clip_ades(dump), []
    for i, a in ades.items():
        j = sel[i]
        parsed = [x for x in a if not np.isnan(x)]
        assert (0 <= j < 4) or (j == -1 and not parsed)
        if mode == "medoid":
            assert (j >= 0 and not np.isnan(a[j])) if parsed else j == -1          # the medoid is a parsed sample whenever there is one
        if j >= 0 and not np.isnan(a[j]):
            assert min(parsed) <= a[j]                                 # minADE_K <= ADE_sel, clip by clip
            picked.append(a[j])
    assert rec["n_sel"] == len(picked) <= rec["n_min"]
    if picked:
        assert abs(rec["ADE_sel"] - float(np.mean(picked))) < 1e-9     # the record's mean is the mean of these


def test_driver_select_none_is_the_run_without_the_flag(tmp_path, capsys):
    rec0, dump0 = _eval(str(tmp_path / "plain"), capsys, [])
    rec1, dump1 = _eval(str(tmp_path / "none"), capsys, ["--select", "none"])
    assert dump0 == dump1 and "selected" not in dump1
    assert set(rec1) == {"ADE", "FDE", "ADE_as_called", "GD", "n", "minADE", "minFDE", "n_min", "K"}
    assert json.dumps(rec0, sort_keys=True) == json.dumps(rec1, sort_keys=True)
    from egoscaler_amd import driver
    with pytest.raises(ValueError):
        driver.main(["eval", "--tiny", "--num_samples", "1", "--select", "medoid", "--dtype", "fp32", "--bs", "2", "--n_val", "2", "--num_steps", "5",
                     "--max_traj_token", "48", "--out_dir", str(tmp_path / "bad")])
