"""GPU: one train-mode step of the full-size point backbone (--unfreeze_pc_encoder; PointBERT v1.2 dims: 512 groups x 32 points, trans_dim
384, 12 blocks) at the geometry `bench.py --mode pc` runs (8 clouds: R = 131072 BatchNorm rows, 4104 LayerNorm rows), driven through
PointBackboneTrainer directly, against the oracle (oracle.pointbert.group + point_transformer_from_groups(training=True)) in float64 with
autograd.  tests/test_gpu_pc_unfrozen.py pins the same path at tiny size only (1024 BatchNorm rows, 66 LayerNorm rows), where the
column reductions take one partial row per lane and the weight gradients split 4 ways instead of 128."""
import types

import numpy as np
import pytest
import torch

from egoscaler_amd import synth
from egoscaler_amd.config import dims_7b

pytestmark = pytest.mark.gpu
REL = 1e-3                       # fp32: the bound of test_gpu_pc_unfrozen.py (features, every gradient from reduce_dim / pos_embed up)
# fp32, the mini-PointNet's gradients (encoder.*): 131072 rows pass two ReLUs, and where fp32 rounding moves a pre-ReLU value across 0 the
# gradient of that element switches on or off.  Measured on MI355X: worst 1.34e-3 (second_conv.0.weight); a float32 run of the oracle itself
# lands 5e-3 from its float64 run.  Gradients whose exact value is 0: 2.1e-3 absolute (first_conv.0.bias, other gradients reach ~15).
ENC_REL, ZERO_ABS = 3e-3, 5e-3
PICK_GAP = 1e-4                  # fp32 group arg-max picks: maxima to within this (relative to the largest |value|); measured 8e-8
PRE = "model.point_backbone."
B = 8
START = [0, 17, 5, 4000, 8191, 123, 2048, 777]
CONV_BIAS = (PRE + "encoder.first_conv.0.bias", PRE + "encoder.second_conv.0.bias")     # in front of a train-mode BatchNorm: exact gradient 0
# (so is first_conv.3.bias': it shifts every row of a group alike, the group max and the concat pass the shift on to second_conv.1)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _dims():
    dims = dims_7b()
    dims.lm.num_hidden_layers = 1
    dims.lm.hidden_size, dims.lm.intermediate_size, dims.lm.vocab_size, dims.lm.num_attention_heads = 64, 64, 64, 2
    return dims


def _drop(depth):
    """[depth, 2, B] DropPath branch scales: some samples drop a branch (0), some keep it scaled (1 / keep), some keep it as is"""
    d = torch.empty(depth, 2, B)
    for i in range(depth):
        for j in range(2):
            for b in range(B):
                d[i, j, b] = 0.0 if (2 * i + j + b) % 5 == 2 else (1.0 / 0.9 if (i + b) % 2 else 1.0)
    return d


def _is_param(k, v):
    return k.startswith(PRE) and v.dtype.is_floating_point and "running_" not in k


def _preact_spread(sd, nb):
    """per-channel std of the two BatchNorm inputs (first_conv.0 and second_conv.0 outputs), float64, from the oracle's own ops"""
    import torch.nn.functional as F
    e = PRE + "encoder."
    BG, M, C = nb.shape[0] * nb.shape[1], nb.shape[2], nb.shape[3]
    with torch.no_grad():
        x = nb.reshape(BG, M, C).transpose(2, 1)
        h1 = F.conv1d(x, sd[e + "first_conv.0.weight"], sd[e + "first_conv.0.bias"])
        s1 = h1.transpose(1, 2).reshape(-1, h1.shape[1]).std(0)
        y1 = F.relu(F.batch_norm(h1, sd[e + "first_conv.1.running_mean"].clone(), sd[e + "first_conv.1.running_var"].clone(),
                                 sd[e + "first_conv.1.weight"], sd[e + "first_conv.1.bias"], training=True, momentum=0.1, eps=1e-5))
        h2 = F.conv1d(y1, sd[e + "first_conv.3.weight"], sd[e + "first_conv.3.bias"])
        cat = torch.cat([h2.max(dim=2, keepdim=True)[0].expand(-1, -1, M), h2], 1)
        h3 = F.conv1d(cat, sd[e + "second_conv.0.weight"], sd[e + "second_conv.0.bias"])
        s3 = h3.transpose(1, 2).reshape(-1, h3.shape[1]).std(0)
    return s1, s3


@pytest.fixture(scope="module")
def inp():
    return make_inputs()


def make_inputs():
    """inputs, the oracle's grouping and the spread of the two BatchNorm inputs"""
    from oracle import pointbert as OPB
    dims = _dims()
    pb = dims.pb
    sd = synth.synth_state_dict(dims, 0)
    pts = torch.stack([synth.synth_cloud(dims, i) for i in range(B)])
    d_feats = torch.randn(B, pb.point_token_len, pb.trans_dim, generator=torch.Generator().manual_seed(7))
    nb, center, _, _ = OPB.group(pts.numpy(), pb.num_group, pb.group_size, np.asarray(START))
    nb64, c64 = torch.from_numpy(nb).double(), torch.from_numpy(center).double()
    spread = _preact_spread({k: v.double() for k, v in sd.items() if k.startswith(PRE)}, nb64)
    return types.SimpleNamespace(dims=dims, sd=sd, pts=pts, d_feats=d_feats, drop=_drop(pb.depth), nb64=nb64, c64=c64, spread=spread)


def oracle_step(inp, picks):
    """the float64 oracle step (features, every backbone gradient, running statistics after) with the mini-PointNet's group maxima taking
    the product's picks: at full size fp32 rounding moves near-tied maxima to another of the 32 points (a float32 run of this same oracle
    lands 5e-3 from its float64 run on second_conv.3.weight that way), and the gradient follows the pick.  pick_gap checks that every
    pick is a maximum to within rounding."""
    from oracle import pointbert as OPB
    pb = inp.dims.pb
    sd64 = {k: v.double().clone().requires_grad_(_is_param(k, v)) for k, v in inp.sd.items() if k.startswith(PRE) and v.dtype.is_floating_point}
    taps = {}
    out = OPB.point_transformer_from_groups(sd64, PRE, inp.nb64, inp.c64, pb.depth, pb.num_heads, taps=taps, training=True,
                                            drop=inp.drop.double(), picks=picks)
    (out * inp.d_feats.double()).sum().backward()
    grads = {k: v.grad.detach() for k, v in sd64.items() if v.requires_grad}
    running = {k: v.detach().clone() for k, v in sd64.items() if "running_" in k}
    zero = {k for k, g in grads.items() if float(g.abs().max()) < 1e-9}
    assert set(CONV_BIAS) <= zero and len(zero) == 3, zero
    return types.SimpleNamespace(feats=out.detach(), grads=grads, running=running, zero=zero, gap=max(taps["pick_gap1"], taps["pick_gap2"]))


def _step(inp, dtype, sd=None):
    """a fresh model in train() mode, one PointBackboneTrainer forward + backward; returns features, main_grads, state after, the group
    arg-max picks"""
    from egoscaler_amd.pointbert_train import PointBackboneTrainer
    from egoscaler_amd.pointllm import TrajPointLLMForCausalLM
    dims = inp.dims
    args = types.SimpleNamespace(unfreeze_pc_encoder=True, unfreeze_language_model=False, num_bins=dims.tok.num_bins, model_name=None)
    m = TrajPointLLMForCausalLM(args, dims, None, device="cuda", dtype=dtype)
    m.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in (sd or inp.sd).items()})
    m.train()
    eng = m.engine
    assert eng.pb_train_mode and eng.pb_trainable
    for k, v in inp.sd.items():
        if _is_param(k, v):
            eng.grad_buffer(k).zero_()
    tr = PointBackboneTrainer(eng)
    feats, ctx = tr.forward(inp.pts.cuda(), START, inp.drop.cuda().contiguous())
    tr.backward(inp.d_feats.to(dtype).cuda(), ctx)
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in eng.main_grad.items() if k.startswith(PRE)}
    state = {k: v.clone() for k, v in eng.w.items() if k.startswith(PRE) and ("running_" in k or "num_batches" in k)}
    picks = (ctx["am2"].cpu(), ctx["am4"].cpu())
    out = feats.float().cpu()
    del m, eng, tr, ctx
    torch.cuda.empty_cache()
    return out, grads, state, picks


def _check_running(inp, ref_step, state, bound, shift=None):
    for k, ref in ref_step.running.items():
        if shift is not None and k.endswith("running_mean"):
            ref = ref + 0.1 * shift.get(k.replace("1.running_mean", "0.bias"), 0.0)            # momentum x the shift of the batch mean
        assert rel(state[k], ref) < bound, (k, rel(state[k], ref))
    for k in (PRE + "encoder.first_conv.1.num_batches_tracked", PRE + "encoder.second_conv.1.num_batches_tracked"):
        assert int(state[k]) == int(inp.sd[k]) + 1, k


def _errors(ref, feats, grads, skip=()):
    """max-relative error of the features and of every gradient with a nonzero exact value; max |g| of those whose exact value is 0"""
    assert sorted(grads) == sorted(ref.grads)
    g_max = {k: rel(grads[k], r) for k, r in ref.grads.items() if k not in ref.zero and k not in skip}
    g_fro = {k: fro(grads[k], r) for k, r in ref.grads.items() if k not in ref.zero and k not in skip}
    zero = {k: float(grads[k].abs().max()) for k in ref.zero if k not in skip}
    return rel(feats, ref.feats), fro(feats, ref.feats), g_max, g_fro, zero


def _show(tag, ref, f_max, f_fro, g_max, g_fro, zero):
    wm, wf = max(g_max, key=g_max.get), max(g_fro, key=g_fro.get)
    print(f"[{tag}] pick gap {ref.gap:.1e}; features max {f_max:.2e} fro {f_fro:.2e}; gradients worst max {g_max[wm]:.2e} ({wm[len(PRE):]}) "
          f"worst fro {g_fro[wf]:.2e} ({wf[len(PRE):]}); exact-zero gradients " + ", ".join(f"{k[len(PRE):]} {v:.1e}" for k, v in zero.items()))


def test_fullsize_pc_train_step_fp32(inp):
    feats, grads, state, picks = _step(inp, torch.float32)
    ref = oracle_step(inp, picks)
    f_max, f_fro, g_max, g_fro, zero = _errors(ref, feats, grads)
    _show("pc fullsize fp32", ref, f_max, f_fro, g_max, g_fro, zero)
    assert ref.gap < PICK_GAP, ref.gap
    assert f_max < REL, f_max
    bad = {k: e for k, e in g_max.items() if e >= (ENC_REL if k.startswith(PRE + "encoder.") else REL)}
    assert not bad, bad
    assert max(zero.values()) < ZERO_ABS, zero
    _check_running(inp, ref, state, REL)


def test_fullsize_pc_train_step_bf16(inp):
    """bf16 weights and activations (fp32 main_grad) against the float64 oracle (group maxima through the bf16 path's picks, which are
    maxima to within bf16 rounding): the blocks take the fused head_dim-64 attention and _wgrad_into for their weight gradients.
    Bounds are ~2x the error measured on MI355X (printed below): features Frobenius 1.21e-2 / max 2.43e-2, gradients worst Frobenius 1.00e-1 /
    max 9.95e-2 (encoder.first_conv.1.bias; the blocks' stay near 1e-2), exact-zero gradients 8.6 absolute, running statistics 4.7e-3, picks
    6.2e-3 from the maximum.  A layout, routing or dropped-partial bug is an O(1) error (dropping one _wg slice: 0.23)."""
    feats, grads, state, picks = _step(inp, torch.bfloat16)
    ref = oracle_step(inp, picks)
    f_max, f_fro, g_max, g_fro, zero = _errors(ref, feats, grads)
    _show("pc fullsize bf16", ref, f_max, f_fro, g_max, g_fro, zero)
    r_max = max(rel(state[k], r) for k, r in ref.running.items())
    print(f"[pc fullsize bf16] running stats {r_max:.2e}")
    assert ref.gap < 1.5e-2, ref.gap
    assert f_fro < 2.5e-2 and f_max < 5e-2, (f_fro, f_max)
    assert max(g_fro.values()) < 2e-1 and max(g_max.values()) < 2e-1
    assert max(zero.values()) < 2e1, zero
    _check_running(inp, ref, state, 1e-2)


def test_fullsize_pc_train_step_fp32_ignores_channel_shift(inp):
    """Some channels of the two conv biases in front of the train-mode BatchNorms moved by 1e2 - 1e3 x that channel's spread (measured on
    the oracle's ops): in exact arithmetic BatchNorm removes a per-channel shift, so features and every gradient but those two biases'
    must still meet the fp32 bounds against the UNshifted oracle; running_mean moves by momentum x the shift, running_var not at all.
    Features and the gradients from reduce_dim / pos_embed up keep REL.  The mini-PointNet's do not quite: first_conv.0's output is itself
    an fp32 value of magnitude 1e3 x its spread (3e-5 x spread of rounding), so more pre-ReLU values cross 0 than above; measured on MI355X
    worst 4.9e-3 (first_conv.1.bias), exact-zero 2.8e-3, bound 1e-2.  With the former uncentred batch variance: 0.28, features 2.5e-2."""
    s1, s3 = inp.spread
    sd = dict(inp.sd)
    for name, s in zip(CONV_BIAS, (s1, s3)):
        d = torch.zeros(s.numel(), dtype=torch.float64)
        for c in range(1, s.numel(), 4):
            d[c] = (1e2, -1e3, 1e3, -1e2)[(c // 4) % 4] * float(s[c])
        sd[name] = (sd[name].double() + d).float()
    shift = {k: (sd[k].double() - inp.sd[k].double()) for k in CONV_BIAS}         # what the fp32 biases actually moved by
    feats, grads, state, picks = _step(inp, torch.float32, sd)
    ref = oracle_step(inp, picks)
    f_max, f_fro, g_max, g_fro, zero = _errors(ref, feats, grads, skip=CONV_BIAS)
    _show("pc fullsize fp32, shifted channels", ref, f_max, f_fro, g_max, g_fro, zero)
    assert ref.gap < PICK_GAP, ref.gap
    assert f_max < REL, f_max
    bad = {k: e for k, e in g_max.items() if e >= (1e-2 if k.startswith(PRE + "encoder.") else REL)}
    assert not bad, bad
    assert max(zero.values()) < 1e-2, zero
    _check_running(inp, ref, state, REL, shift)
