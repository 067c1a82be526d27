"""The launch trace of decode.Decoder: every library call of a prefill + token loop, as data.

trace() wraps the `call` name bound in every loaded egoscaler_amd module and records each launch as [symbol, argument, ...]: scalars by
value, device pointers as [buffer name, byte offset] (named through the Decoder's public buffers and the engine's weights, RoPE tables
and workspace), NULL as None, a descriptor passed by reference as the list of its fields.  A pointer into no named buffer is an error.
Two decoders that record the same trace for a case issue the same launches in the same order with the same arguments: same results, same
speed.  tests/golden/decode_launch_trace.json holds the trace of every case in CASES as recorded by tools/debug/record_decode_trace.py
on the commit before Decoder's cache layouts became objects (the two *_bs cases: on the commit before the per-step readouts of sample() /
greedy() / score() were written once); tests/test_gpu_decode_trace.py replays the cases against it.

Shapes: LLaMA-7B width (the slab-fused step needs it) with one decoder layer, 4 decoder rows (grouped modes: 2 prompts x 2), a text-only
prompt of 24 tokens, 3 new tokens = two step() calls, eager (use_graph=False)."""
import os
import types

import torch

from tests.launch_trace import Recorder, first_difference, trace  # noqa: F401  (the recording core: tests/launch_trace.py)

ROWS, S0, T = 4, 24, 3
PREFILL_ONLY = "egomi_kv_append"          # during prefill only the decoder's own launches are recorded, not the engine's

# name: (model, Decoder kwargs, EGOMI_DECODE_FUSED, loop, fused as the case must find it, also record prefill_chunked(chunk=1))
ALL, NONE, NO_QKV = "all", "none", "no_qkv"
GROUP = dict(max_new_tokens=T)
CASES = {
    "bf16_greedy": ("bf16", {}, "1", "greedy", ALL, True),
    "bf16_greedy_unfused": ("bf16", {}, "0", "greedy", NONE, False),
    "kv8_sample_logprobs": ("bf16", dict(kv_dtype="fp8"), "1", "sample_lp", ALL, True),
    "w8_greedy": ("bf16", dict(weight_dtype="fp8"), "1", "greedy", ALL, False),
    "w8_kv8_greedy": ("bf16", dict(weight_dtype="fp8", kv_dtype="fp8"), "1", "greedy", ALL, False),
    "beam2": ("bf16", dict(num_beams=2), "1", "beam", ALL, False),
    "beam2_kv8": ("bf16", dict(num_beams=2, kv_dtype="fp8"), "1", "beam", ALL, False),
    "shared2_sample": ("bf16", dict(samples_per_prompt=2, **GROUP), "1", "sample", NO_QKV, True),
    "shared2_w8_sample": ("bf16", dict(samples_per_prompt=2, weight_dtype="fp8", **GROUP), "1", "sample", NO_QKV, False),
    "split_beam2": ("bf16", dict(num_beams=2, split_cache=True, **GROUP), "1", "beam", NO_QKV, False),
    "split_beam2_w8": ("bf16", dict(num_beams=2, split_cache=True, weight_dtype="fp8", **GROUP), "1", "beam", NO_QKV, False),
    "lora_greedy": ("lora", {}, "1", "greedy", ALL, False),
    "fp32_tiny_greedy": ("tiny", {}, "1", "greedy", NONE, False),
    "sample_lp_bs": ("bf16", {}, "1", "sample_lp_bs", ALL, False),
    "greedy_bs": ("bf16", {}, "1", "greedy_bs", ALL, False),
}

DECODER_BUFFERS = ("kc", "vc", "ks", "vs", "kp", "vp", "ksfx", "vsfx", "kv_row", "lp_tok", "lp_sum", "lp_n", "lp_live", "bs_mass", "bs_mean", "bs_std",
                   "bs_ent", "lg", "seq_buf", "mask_buf",
                   "x", "h", "qkv", "ao", "x_mid", "h2", "gu", "act", "hn", "tok", "gws", "rng", "done_buf", "fin_seq", "bidx", "fin_bidx",
                   "run_score", "fin_score", "fin_flag", "heur", "ctl")


def make_model(kind, layers=1, **flags):
    """bf16: LLaMA-7B width, `layers` decoder layers; lora: the same with r=8 adapters on q_proj and o_proj; tiny: dims_tiny in fp32.
    flags: further fields of the model's args (tests/train_trace.py: what is trainable, other adapter targets).  The trace does not
    depend on the weights' values: they are drawn on the device."""
    from egoscaler_amd.config import dims_7b, dims_tiny
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dims = dims_tiny() if kind == "tiny" else dims_7b()
    if kind != "tiny":
        dims.lm.num_hidden_layers = layers
    args = types.SimpleNamespace(unfreeze_pc_encoder=False, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None)
    if kind == "lora":
        args.lora_r, args.lora_alpha, args.lora_target_modules = 8, 16, "q_proj,o_proj"
    args.__dict__.update(flags)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=torch.float32 if kind == "tiny" else torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(7)
    with torch.no_grad():
        for n, p in list(m.named_parameters()) + list(m.named_buffers()):
            leaf = n.rsplit(".", 1)[-1]
            if leaf == "num_batches_tracked":
                continue
            if leaf == "running_var" or (leaf == "weight" and p.dim() == 1):
                p.fill_(1.0)
            elif leaf == "running_mean":
                p.zero_()
            else:
                p.copy_(torch.empty(p.shape, dtype=torch.float32, device="cuda").normal_(0, 0.02, generator=g))
    m.engine.prepared = False
    return m.eval()


def prompt(n):
    """n text-only prompts of S0 tokens (no point tokens, no special ids)."""
    return torch.randint(3, 200, (n, S0), generator=torch.Generator().manual_seed(11)).cuda()


def named_buffers(dec):
    """[(name, tensor)] in resolution order: the decoder's buffers, its stacked / merged / quantized weights, then the engine's."""
    eng, out = dec.eng, []
    for n in DECODER_BUFFERS:
        out.append((n, getattr(dec, n, None)))
    for T_new, t in dec._scores.items():
        out.append((f"scores[{T_new}]", t))
    for nb, t in dec._bs_values.items():
        out.append((f"bs_values[{nb}]", t))
    for K, ts in getattr(dec, "_cands", {}).items():
        out += [(f"cands[{K}][{i}]", t) for i, t in enumerate(ts)]
    for name in ("wqkv", "wgu", "wo", "wdown"):
        out += [(f"{name}[{l}]", t) for l, t in enumerate(getattr(dec, name) or [])]
    for l, q in enumerate(dec.w8 or []):
        out += [(f"w8[{l}][{n}][{i}]", t) for n, pair in q.items() for i, t in enumerate(pair)]
    out += [(f"eng.w[{n}]", t) for n, t in eng.w.items()]
    out += [("eng.cos", eng.cos), ("eng.sin", eng.sin)]
    out += [(f"eng.ws[{n}]", t) for n, t in eng.ws.bufs.items()]
    return [(n, t) for n, t in out if isinstance(t, torch.Tensor) and t.is_cuda]


def check_fused(dec, expect):
    f = dec.fused
    if expect == ALL:
        assert all(f.values()), f
    elif expect == NONE:
        assert not any(f.values()), f
    else:
        assert f["qkv"] == 0 and f["o"] and f["down"], f


def run_case(models, name):
    """Runs case `name` on models[kind] (made on first use); -> {"prefill": [...], "loop": [...], and for some "prefill_chunked": [...]}."""
    from egoscaler_amd.decode import Decoder
    kind, kw, fused_env, loop, expect, chunked = CASES[name]
    if kind not in models:
        models[kind] = make_model(kind)
    m = models[kind]
    tok = m.dims.tok
    nb = kw.get("num_beams", 1)
    ids = prompt(ROWS // (nb * kw.get("samples_per_prompt", 1)))
    old = os.environ.get("EGOMI_DECODE_FUSED")
    os.environ["EGOMI_DECODE_FUSED"] = fused_env
    try:
        dec = Decoder(m.engine, ROWS, S0 + T, **kw)
    finally:
        if old is None:
            del os.environ["EGOMI_DECODE_FUSED"]
        else:
            os.environ["EGOMI_DECODE_FUSED"] = old
    check_fused(dec, expect)
    out = {}
    with trace(PREFILL_ONLY) as rec:
        dec.prefill(ids, None, None, None, T, nb=nb)
    out["prefill"] = rec.resolved(named_buffers(dec))
    bins = (tok.p0, tok.num_bins) if loop.endswith("_bs") else None
    with trace() as rec:
        if loop in ("greedy", "greedy_bs"):
            dec.greedy(T, use_graph=False, bin_stats=bins)
        elif loop == "beam":
            dec.beam(T, eos=tok.eos, pad=tok.pad, use_graph=False)
        else:
            dec.sample(T, eos=tok.eos, pad=tok.pad, seed=5, use_graph=False, logprobs=loop.startswith("sample_lp"), bin_stats=bins)
    out["loop"] = rec.resolved(named_buffers(dec))
    if chunked:
        with trace(PREFILL_ONLY) as rec:
            dec.prefill_chunked(ids, None, None, None, T, chunk=1, nb=nb)
        out["prefill_chunked"] = rec.resolved(named_buffers(dec))
    torch.cuda.synchronize()
    assert out["prefill"] and out["loop"]
    return out
