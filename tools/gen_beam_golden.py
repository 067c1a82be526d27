"""Records tests/golden/beam_search.npz: HF transformers' own beam search / beam sampling (GenerationMixin._beam_search) on the tiny
model, for tests/test_gpu_beam.py.  `python tools/gen_beam_golden.py [out.npz]` (CPU, seconds).

Model: dims_tiny() with synth.synth_state_dict(seed 0), the batch of tests/test_gpu_model.py::tiny and its golden fps_start; the LLaMA
part as a CPU fp32 HF LlamaForCausalLM carrying the same weights.  Prompt embeddings are the spliced ones of oracle.pointllm.forward
(point features in place of the patch tokens); generate() gets input_ids (so `sequences` carries the prompt ids and the repetition penalty
sees them), inputs_embeds, the attention mask and position_ids 0..S0-1 (the project's positions: left padding is masked, not shifted).

Per case: sequences, sequences_scores, beam_indices, scores [iterations, B*nb, V], and `margin`: the smallest gap, over every step and
item, between the K-th and (K+1)-th accumulated score (the candidate cut) and between the nb-th and (nb+1)-th of the running choice, so
fp32 rounding on the device cannot flip a recorded decision.  The beam-sampling case records HF's step-0 processed log-probs only
(torch.multinomial's stream is not reproducible)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from egoscaler_amd import synth                         # noqa: E402
from egoscaler_amd.config import dims_tiny              # noqa: E402
from oracle import pointllm as OPL                      # noqa: E402

T_NEW = 6
EOS_EARLY = None          # chosen below: a token the tiny model ranks high, so hypotheses finish before max_length


def tiny_setup():
    dims = dims_tiny()
    sd = synth.synth_state_dict(dims, 0)
    toks, masks, Lp = synth.synth_batch(dims, 2, text_len=8, num_steps=4, max_traj_token=40)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(2)])
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_model.npz"), allow_pickle=False)
    return dims, sd, toks[:, :Lp].clone(), masks[:, :Lp].clone(), pts, g["fps_start"]


def hf_model(dims, sd):
    from transformers import LlamaConfig, LlamaForCausalLM
    lm = dims.lm
    cfg = LlamaConfig(vocab_size=lm.vocab_size, hidden_size=lm.hidden_size, intermediate_size=lm.intermediate_size,
                      num_hidden_layers=lm.num_hidden_layers, num_attention_heads=lm.num_attention_heads,
                      num_key_value_heads=lm.num_attention_heads, max_position_embeddings=lm.max_position_embeddings,
                      rms_norm_eps=lm.rms_norm_eps, rope_theta=lm.rope_theta, tie_word_embeddings=False, attn_implementation="eager",
                      pad_token_id=dims.tok.pad, bos_token_id=1, eos_token_id=dims.tok.eos)
    m = LlamaForCausalLM(cfg).eval()
    own = m.state_dict()
    m.load_state_dict({k: sd[k].float() for k in own}, strict=True)
    return m


def embeds(dims, sd, ids, mask, pts, start):
    taps = {}
    with torch.no_grad():
        OPL.forward({k: v.float() for k, v in sd.items()}, dims, ids, mask, pts, start, taps=taps)
    return taps["inputs_embeds"].detach().float()


def run(m, ids, emb, mask, **kw):
    torch.manual_seed(0)
    S0 = ids.shape[1]
    with torch.no_grad():
        return m.generate(input_ids=ids, inputs_embeds=emb, attention_mask=mask.long(), position_ids=torch.arange(S0)[None].expand(ids.shape[0], -1),
                          max_new_tokens=T_NEW, min_new_tokens=0, output_scores=True, return_dict_in_generate=True, use_cache=True, **kw)


def margins(out, nb, eos, S0, lpen, es):
    """Smallest decision gap of a recorded HF beam-search run: HF's bookkeeping (_beam_search) replayed on its own recorded scores, and
    at every step the gap at each comparison that decides something: the K-th vs (K+1)-th accumulated candidate (where the K-th is chosen
    to continue; otherwise neither is used), the nb-th vs (nb+1)-th
    of the running choice, the nb-th vs (nb+1)-th of the finished merge (where a real hypothesis is at stake), and the early-stop
    heuristic's best-possible vs worst-finished.  The replay must reproduce HF's sequences_scores (a check of the replay itself)."""
    K = 2 * nb
    sc = torch.stack(out.scores, 0)
    it, R, V = sc.shape
    B = R // nb
    T = int(out.beam_indices.shape[1]) if it else 0
    max_len = S0 + T_NEW
    run_s = torch.full((B, nb), -1e9)
    run_s[:, 0] = 0
    fin_s, fin_f, heur = torch.full((B, nb), -1e9), torch.zeros(B, nb, dtype=torch.bool), torch.ones(B, dtype=torch.bool)
    gap = float("inf")
    real = lambda x: x > -1e8
    for t in range(it):
        cur = S0 + t
        acc = (sc[t].view(B, nb, V) + run_s[:, :, None]).view(B, nb * V)
        top_v, top_i = torch.topk(acc, K + 1, dim=1)
        tk_s, tok = top_v[:, :K], top_i[:, :K] % V
        hit = (tok == eos) | (cur + 1 >= max_len) if eos is not None else torch.full_like(tok, cur + 1 >= max_len, dtype=torch.bool)
        rs = tk_s + hit.float() * -1e9
        rv, ri = torch.sort(rs, 1, descending=True)
        for b in range(B):
            if real(rv[b, nb]):
                gap = min(gap, float(rv[b, nb - 1] - rv[b, nb]))
            if (ri[b, :nb] == K - 1).any():                              # the K-th candidate continues: the cut at K decided it
                gap = min(gap, float(top_v[b, K - 1] - top_v[b, K]))
        run_s = rv[:, :nb].clone()
        f = tk_s / float((cur + 1 - S0) ** lpen)
        f = f + (fin_f.all(1, keepdim=True) & (es is True)).float() * -1e9
        f = f + (~heur[:, None]).float() * -1e9
        did = hit & (torch.arange(K) < nb)[None]
        f = f + (~did).float() * -1e9
        ms = torch.cat([fin_s, f], 1)
        mf = torch.cat([fin_f, did], 1)
        mv, mi = torch.sort(ms, 1, descending=True)
        for b in range(B):
            if real(mv[b, nb]):
                gap = min(gap, float(mv[b, nb - 1] - mv[b, nb]))
        fin_s, fin_f = mv[:, :nb].clone(), torch.gather(mf, 1, mi[:, :nb])
        L = (max_len - S0) if (es == "never" and lpen > 0) else (cur + 1 - S0)
        best = run_s[:, 0] / float(L ** lpen)
        worst = torch.where(fin_f, fin_s.min(1, keepdim=True)[0], torch.full_like(fin_s, -1e9))
        for b in range(B):
            for j in range(nb):
                if real(worst[b, j]) and real(best[b]):
                    gap = min(gap, abs(float(best[b] - worst[b, j])))
        heur = heur & (best[:, None] > worst).any(1)
    nrs = out.sequences_scores.shape[0] // B
    assert torch.allclose(fin_s[:, :nrs].reshape(-1), out.sequences_scores, rtol=0, atol=1e-5), "replay of HF's bookkeeping"
    return gap


def main(path=os.path.join(ROOT, "tests", "golden", "beam_search.npz")):
    torch.manual_seed(0)
    dims, sd, ids, mask, pts, start = tiny_setup()
    m = hf_model(dims, sd)
    emb = embeds(dims, sd, ids, mask, pts, start)
    out = {"prompt_ids": ids.numpy(), "prompt_mask": mask.numpy().astype(np.uint8), "fps_start": np.asarray(start), "t_new": np.int64(T_NEW)}
    # the eos of the early-finishing case: the token greedy beam search ranks first at step 2 in item 0 and never in item 1's top beam
    probe = run(m, ids, emb, mask, num_beams=4, do_sample=False, eos_token_id=None, pad_token_id=dims.tok.pad)
    S0 = ids.shape[1]
    eos_early = int(probe.sequences[0, S0 + 2])
    mask_lp = mask.clone()
    ids_lp = ids.clone()
    mask_lp[1, :2] = False                                              # left padding in item 1: two masked keys
    ids_lp[1, :2] = dims.tok.pad
    emb_lp = embeds(dims, sd, ids_lp, mask_lp, pts, start)
    cases = {
        "nb4": (dict(num_beams=4, num_return_sequences=1), None),
        "nb3_lp0_es": (dict(num_beams=3, num_return_sequences=3, length_penalty=0.0, early_stopping=True, repetition_penalty=1.1), None),
        "nb4_lp2_never": (dict(num_beams=4, num_return_sequences=2, length_penalty=2.0, early_stopping="never"), None),
        "rep13": (dict(num_beams=4, num_return_sequences=2, repetition_penalty=1.3), None),
        "leftpad": (dict(num_beams=4, num_return_sequences=2), "lp"),
        "eos": (dict(num_beams=4, num_return_sequences=4, eos_token_id=eos_early), None),
        "eos_es": (dict(num_beams=4, num_return_sequences=4, eos_token_id=eos_early, early_stopping=True), None),
        "eos_never_lp2": (dict(num_beams=4, num_return_sequences=4, eos_token_id=eos_early, early_stopping="never", length_penalty=2.0), None),
    }
    names = []
    for name, (kw, variant) in cases.items():
        kw = dict(kw)
        kw.setdefault("eos_token_id", dims.tok.eos)
        kw.setdefault("length_penalty", 1.0)
        kw.setdefault("early_stopping", False)
        kw.setdefault("repetition_penalty", 1.0)
        i_, e_, m_ = (ids_lp, emb_lp, mask_lp) if variant == "lp" else (ids, emb, mask)
        o = run(m, i_, e_, m_, do_sample=False, pad_token_id=dims.tok.pad, **kw)
        gap = margins(o, kw["num_beams"], kw["eos_token_id"], i_.shape[1], kw["length_penalty"], kw["early_stopping"])
        es = {False: 0, True: 1, "never": 2}[kw["early_stopping"]]
        out[f"{name}/sequences"] = o.sequences.numpy()
        out[f"{name}/sequences_scores"] = o.sequences_scores.numpy()
        out[f"{name}/beam_indices"] = o.beam_indices.numpy().astype(np.int64)
        out[f"{name}/scores"] = torch.stack(o.scores, 0).numpy()
        out[f"{name}/args"] = np.array([kw["num_beams"], kw["num_return_sequences"], kw["length_penalty"], es, kw["repetition_penalty"],
                                        kw["eos_token_id"], 1 if variant == "lp" else 0], dtype=np.float64)
        out[f"{name}/margin"] = np.float64(gap)
        names.append(name)
        print(f"{name}: iterations {len(o.scores)} seq {tuple(o.sequences.shape)} margin {gap:.3g} scores {o.sequences_scores.tolist()}")
    # beam sampling: HF's step-0 processed log-probs (repetition penalty, temperature, top-k 50, top-p 0.95, min_tokens_to_keep = 2)
    o = run(m, ids, emb, mask, num_beams=4, do_sample=True, temperature=0.7, top_k=50, top_p=0.95, repetition_penalty=1.1,
            eos_token_id=dims.tok.eos, pad_token_id=dims.tok.pad, max_length=None)
    out["sample/scores0"] = o.scores[0].numpy()
    out["sample/args"] = np.array([4, 0.7, 50, 0.95, 1.1], dtype=np.float64)
    out["cases"] = np.array(names)
    np.savez(path, **out)
    return out


if __name__ == "__main__":
    main(*sys.argv[1:])
