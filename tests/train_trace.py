"""The launch trace of the training step (engine.Engine behind model.loss_and_backward) and of the prefill forward, as data.

Every case records, unfiltered, the library calls of one or two loss_and_backward() calls or of one forward_hidden(save=False) call, in
the form tests/launch_trace.py describes.  Two engines that record the same trace for a case issue the same launches in the same order
with the same arguments: same results, same GPU time.  tests/golden/train_launch_trace.json holds the trace of every case in CASES as
recorded by tools/debug/record_train_trace.py; tests/test_gpu_train_trace.py replays the cases against it.

Pointers are named by key path, in this order, through the engine's workspace (ws.qkv), main_grad and layer_flat, the saved context
(ctx.layers[1].qkv, ctx.x_last, ctx.pb_ctx.blocks[0].xs; dictionary keys sorted, so the order in which the engine fills the
context does not matter), the parameters (w.lm_head.weight), the derived weights (wT, wqkv, wgu, wgu_cat, wqkvT, wguT, folded, lm_wT, cos, sin),
the grow-only scratch buffers (lora_ws, ops.tail_ws, pointbert_train.partials), the call's inputs (in.*) and what it returned (out).
What none of these holds after the call (out=None results inside ops, the PointBERT trainer's temporaries, loss_and_backward's own) is
named tmp[k] by trace(keep=True): k counts such allocations in the order in which the launches first point into them.

State that would make a case depend on what ran before it in the process is reset first: the derived weights are prepared before the
recording, the padded lm_head transpose is marked stale (every step records its refresh), and the grow-only scratch buffers whose size
is an argument of the launches (the engine's lora_ws, pointbert_train's partials) are dropped, so they have the size the case itself asks for.

Shapes.  7B width (dims_7b with num_hidden_layers = 2: a lower layer and the top layer), B = 3 samples of S = 620 tokens (8 text tokens,
one 513-token point segment, 96 trajectory tokens), prompt_len = 532: M = B*S = 1860 rows, the loss window R = 89, B*R = 267 rows.
gate|up takes the 256x256 kernel at both heights (8 x 86 and 2 x 86 tiles of 256 x 256, at least 128).  At M = 1860 the library K-slices
tile rows of all five products whose tail the engine can defer (q|k|v from row 1280; o_proj, down_proj and the two dgrads, 128 tiles
each, every row), which B = 4 at the same S does not (one round of whole tiles); B*S is a multiple of 4,
as the k-major weight-gradient kernel asks of its reduction length.  Tiny: dims_tiny in fp32, B = 2, S = 84."""
import torch

from tests import decode_trace as DT
from tests.launch_trace import first_difference, trace  # noqa: F401

SEVEN = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
# name: (decode_trace.make_model kind, further model args, batch size)
MODELS = {
    "frozen": ("bf16", {}, 3),
    "unfrozen": ("bf16", dict(unfreeze_language_model=True), 3),
    "lora": ("lora", dict(lora_target_modules=SEVEN), 3),
    "tiny": ("tiny", {}, 2),
    "tiny_unfrozen": ("tiny", dict(unfreeze_language_model=True), 2),
    "tiny_pc": ("tiny", dict(unfreeze_pc_encoder=True), 2),
}
ARMS_OFF = dict(use_top_rows=False, use_fused_swiglu=False, use_tail_fuse=False)
# name: (model, engine switches, point clouds given, loss_and_backward calls (0: forward_hidden(save=False) with a no-op kv_sink))
CASES = {
    "frozen_bf16": ("frozen", {}, True, 1),
    "frozen_bf16_arms_off": ("frozen", ARMS_OFF, True, 1),
    "frozen_bf16_text_only": ("frozen", {}, False, 1),
    "unfrozen_bf16": ("unfrozen", {}, True, 2),             # the second step accumulates
    "lora_bf16": ("lora", {}, True, 1),
    "prefill_bf16": ("frozen", {}, True, 0),
    "tiny_fp32_frozen": ("tiny", {}, True, 1),
    "tiny_fp32_unfrozen": ("tiny_unfrozen", {}, True, 1),
    "tiny_pc_unfrozen": ("tiny_pc", {}, True, 1),
}
TAILS = {"egomi_rmsnorm_fwd_tail", "egomi_rope_qkv_tail", "egomi_rmsnorm_bwd_tail"}


def make_model(kind):
    """-> (model in train() mode with prepared derived weights, its batch: ids, mask, clouds, prompt_len, fps starts)."""
    from egoscaler_amd import synth
    base, flags, B = MODELS[kind]
    m = DT.make_model(base, layers=2, **flags).train()
    m.engine.prepare()
    tiny = base == "tiny"
    ids, mask, Lp = synth.synth_batch(m.dims, B, text_len=8, num_steps=4 if tiny else 8, max_traj_token=40 if tiny else 96)
    pts = torch.stack([synth.synth_cloud(m.dims, i) for i in range(B)])
    return m, (ids.cuda(), mask.cuda(), pts.cuda(), Lp, [(7 * i + 3) % m.dims.pb.npoints for i in range(B)])


def _paths(prefix, obj):
    """[(key path, tensor)] of the tensors inside nested dictionaries (keys sorted), lists and tuples."""
    if isinstance(obj, torch.Tensor):
        return [(prefix, obj)]
    if isinstance(obj, dict):
        return [p for k in sorted(obj, key=str) for p in _paths(f"{prefix}.{k}", obj[k])]
    if isinstance(obj, (list, tuple)):
        return [p for i, v in enumerate(obj) for p in _paths(f"{prefix}[{i}]", v)]
    return []


def named_buffers(eng, ctx, io):
    """[(name, tensor)] in resolution order (module docstring)."""
    from egoscaler_amd import ops, pointbert_train
    out = _paths("ws", eng.ws.bufs) + _paths("main_grad", eng.main_grad) + _paths("layer_flat", eng.layer_flat) + _paths("ctx", ctx) + _paths("w", eng.w)
    for attr in ("wT", "wqkv", "wgu", "wgu_cat", "wqkvT", "wguT", "folded", "lm_wT", "cos", "sin"):
        out += _paths(attr, getattr(eng, attr, None))
    out += _paths("lora_ws", eng._lora_ws) + _paths("ops.tail_ws", list(ops._TAIL_WS.values())) + _paths("pointbert_train.partials", list(pointbert_train._PART.values()))
    out += _paths("in", io[0]) + _paths("out", io[1])
    return [(n, t) for n, t in out if t.is_cuda]


def _step(m, batch, points):
    """One loss_and_backward under the recorder; -> the resolved launches.  backward_hidden drops engine.ctx when it is done: the
    context is taken as backward_hidden is entered."""
    eng = m.engine
    ids, mask, pts, Lp, start = batch
    seen = {}

    def backward_hidden(d_hn):
        seen["ctx"] = eng.ctx
        return type(eng).backward_hidden(eng, d_hn)
    eng.backward_hidden = backward_hidden
    try:
        with trace(keep=True) as rec:
            loss = m.loss_and_backward(ids, mask, pts if points else None, Lp, m.dims.tok.pad, fps_start=start if points else None)
        return rec.resolved(named_buffers(eng, seen["ctx"], (dict(ids=ids, mask=mask, points=pts), loss)))
    finally:
        del eng.backward_hidden


def _prefill(m, batch):
    eng = m.engine
    ids, mask, pts, _, start = batch
    sunk = []
    with trace(keep=True) as rec:
        hn = eng.forward_hidden(ids, mask, pts, start, save=False, kv_sink=lambda l, qkv, B, S: sunk.append(l))
    assert sunk == list(range(m.dims.lm.num_hidden_layers)) and eng.ctx is None
    return rec.resolved(named_buffers(eng, None, (dict(ids=ids, mask=mask, points=pts), hn)))


def _gemms(launches, **fields):
    """The egomi_gemm descriptors (as {field: value}) whose fields have the given values."""
    from egoscaler_amd.ops import GemmDesc
    names = [f for f, _ in GemmDesc._fields_]
    ds = [dict(zip(names, r[1])) for r in launches if r[0] == "egomi_gemm"]
    return [d for d in ds if all(d[k] == v for k, v in fields.items())]


def check_case(name, m, batch, out):
    """What the case is there for was taken: without this a case could pass on the wrong path."""
    from egoscaler_amd import _abi, ops
    eng, lm = m.engine, m.dims.lm
    d, Fd = lm.hidden_size, lm.intermediate_size
    B, S = batch[0].shape
    syms = [{r[0] for r in launches} for launches in out.values()]
    if name in ("frozen_bf16", "frozen_bf16_text_only"):
        R = eng.top_rows_taken
        assert R == S - batch[3] + 1 > 0 and ops.gemm_kernel_id(B * S, 2 * Fd, d) == 2 and ops.gemm_kernel_id(B * R, 2 * Fd, d) == 2
        assert TAILS <= syms[0] and not {"egomi_swiglu_il_fwd", "egomi_swiglu_fwd", "egomi_swiglu_bwd"} & syms[0], sorted(syms[0])
        assert len(_gemms(out["step0"], epilogue=_abi.EGOMI_EPI_SWIGLU)) == 2 and _gemms(out["step0"], epilogue=_abi.EGOMI_EPI_SWIGLU_BWD)
        assert len(_gemms(out["step0"], epilogue=_abi.EGOMI_EPI_SWIGLU, M=B * R)) == 1           # the windowed top layer's own decision
        assert ("egomi_fps" in syms[0]) == ("egomi_splice_scan" in syms[0]) == (name == "frozen_bf16")
    elif name == "frozen_bf16_arms_off":
        assert eng.top_rows_taken == 0 and not TAILS & syms[0] and {"egomi_swiglu_il_fwd", "egomi_swiglu_il_bwd"} <= syms[0]
    elif name == "unfrozen_bf16":
        for step, acc in (("step0", 0), ("step1", 1)):
            wg = [g for g in _gemms(out[step], a_layout=1, b_layout=1) if g["M"] in (3 * d, 2 * Fd)]
            assert {g["M"] for g in wg} == {3 * d, 2 * Fd} and all(g["accumulate"] == acc for g in wg), (step, wg)     # _wgrad_stacked, k-major
            assert _gemms(out[step], a_layout=0, b_layout=1, K=3 * d, N=d)                       # k-major dgrad over [Wq;Wk;Wv] in place
    elif name == "lora_bf16":
        assert set(eng.lora_groups) == {"qkv", "o", "gu", "down"} and {"egomi_lora_down", "egomi_lora_up", "egomi_lora_wgrad"} <= syms[0]
        assert not TAILS & syms[0] and "egomi_swiglu_il_fwd" in syms[0]                          # every adapted product keeps its plain epilogue
    elif name == "prefill_bf16":
        assert "egomi_attn_fwd" in syms[0] and not {"egomi_attn_bwd", "egomi_ce_fwd_bwd"} & syms[0]
    elif name.startswith("tiny_fp32"):
        assert not eng.wqkv and not eng.wgu and {"egomi_softmax_fwd", "egomi_softmax_bwd", "egomi_swiglu_fwd"} <= syms[0]
        assert _gemms(out["step0"], a_layout=0, b_layout=1, ab_dtype=ops.F32)                    # generic dgrad
        assert bool(_gemms(out["step0"], a_layout=1, b_layout=1, M=Fd)) == (name == "tiny_fp32_unfrozen")
    elif name == "tiny_pc_unfrozen":
        assert {"egomi_bn_train_fwd", "egomi_bn_train_bwd", "egomi_group_argmax", "egomi_layernorm_bwd"} <= syms[0]


def run_case(models, name, **switches):
    """Runs case `name` on models[kind] (made on first use) with the case's engine switches (and `switches` on top);
    -> {"step0": [...], "step1": [...]} or {"forward": [...]}."""
    kind, sw, points, steps = CASES[name]
    if kind not in models:
        models[kind] = make_model(kind)
    m, batch = models[kind]
    eng = m.engine
    sw = {**sw, **switches}
    old = {k: getattr(eng, k) for k in sw}
    eng.__dict__.update(sw)
    from egoscaler_amd import pointbert_train
    eng.lm_wT_stale, eng._lora_ws, m.accumulate_grads = True, None, False
    pointbert_train._PART.clear()
    try:
        if steps == 0:
            out = {"forward": _prefill(m, batch)}
        else:
            out = {}
            for i in range(steps):
                m.accumulate_grads = i > 0
                out[f"step{i}"] = _step(m, batch, points)
        torch.cuda.synchronize()
        if not switches:
            check_case(name, m, batch, out)
    finally:
        eng.__dict__.update(old)
        m.accumulate_grads = False
    assert all(out.values())
    return out
