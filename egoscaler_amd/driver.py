"""Train / evaluate drivers on RCCL (SURVEY.md §8f rows N1 + N2).

Mirrors egoscaler/models/pointllm/train.py:39-310 and evaluate.py:70-170 without DeepSpeed / wandb:
  * same flags (argparse names of train.py:312-347), AdamW + linear warm-up over 1/5 of the steps
    (train.py:107-117), loss on the trajectory span (train.py:174-181), validation by generation +
    ADE/FDE (train.py:207-264), checkpoints `latest_model.pt` / `best_model_ade.pt` with the
    reference's dict keys (train.py:287-308), `--resume` (train.py:138-150),
    `{split}_gen_trajs.json` dump (evaluate.py:167-170)
  * one process per GPU, batch sharded by rank (the reference has no DistributedSampler,
    train.py:72-82), gradients all-reduced by dp.GradSync overlapped with backward.
The batch dict is the collate_fn contract of dataset.py:150-194 ('pcrgbs', 'prompts', 'prompt_masks',
'tokens', 'attention_masks', 'trajectories', 'trajectory_masks', 'max_abs', 'image_ids'), assembled on
the device (`build_batch`).  Data sources of the command line: EgoScaler files (`--root_dir/--data_dir`: data_io.EgoScalerFiles +
FileTrajData, descriptions through the HF tokenizer of `--model_name` with the reference's prompt template, dataset.py:16-19) or, without
them, the seeded synthetic samples of SURVEY.md §8d.  `--model_name DIR` goes through `build_model(args)` exactly as train.py:67 /
evaluate.py:79 do (config.json, weights and tokenizer of the directory; trajectory tokens appended, builder.py:33-46).
"""
import argparse
import json
import os
import types

import numpy as np
import torch
import torch.distributed as dist

from . import ops, synth, traj as T
from .dp import GradSync, shard_range, ragged_shard_range
from .optim import EgoAdamW, linear_warmup_lr


def collate(dims, image_ids, pcrgbs, desc_tokens, desc_masks, traj_tokens, traj_masks, gt_trajs, max_abs, sep_ids=()):
    """`CustomDataset.collate_fn` (dataset.py:150-194) on device tensors that are already stacked:
    tokens = desc | <sep> ids | traj ; masks likewise (the <sep> ids are always attended) ; prompts run up to and including
    the first <tsep> of SAMPLE 0 (dataset.py:180-182) ; 'trajectory_masks' is the token-level trajectory mask."""
    dev = pcrgbs.device
    B = desc_tokens.shape[0]
    sep = torch.as_tensor(list(sep_ids), dtype=torch.int64, device=dev).reshape(1, -1).expand(B, -1)
    tokens = torch.cat((desc_tokens, sep, traj_tokens), dim=-1)
    masks = torch.cat((desc_masks.bool(), torch.ones_like(sep), traj_masks.bool()), dim=-1)      # bool ++ int64 -> int64 0/1, as in the reference
    hit = (tokens[0] == dims.tok.tsep).nonzero()
    if hit.numel() == 0:
        raise IndexError("no <tsep> in the first sample")                  # the reference's [1][0] raises IndexError here too
    pos = int(hit[0, 0])
    return {"image_ids": image_ids, "pcrgbs": pcrgbs, "prompts": tokens[:, :pos + 1], "prompt_masks": masks[:, :pos + 1],
            "tokens": tokens, "attention_masks": masks, "trajectories": gt_trajs, "trajectory_masks": traj_masks.bool(),
            "max_abs": max_abs}


def build_batch(dims, desc_ids, trajs, pcrgbs, max_traj_token=160, image_ids=None, steps=None, desc_mask=None, max_abs=None,
                sep_ids=(), gt_trajs=None):
    """The per-sample half the release lacks (`CustomDataset.__getitem__`) + collate, on the device.
    desc_ids i64 [B,Ld] (description tokens, padded), desc_mask bool [B,Ld] (False on padding; None = all real),
    trajs f32 [B,T,6] in [-1,1] (already normalised), pcrgbs f32 [B,N,6].
    Description part: [bos] desc_a <point_start> <point_patch>xP <point_end> desc_b; trajectory part:
    <ts> (p*6 <tsep>)*T <te> eos pad...  Padding positions of the description carry mask False into `attention_masks`
    and `prompt_masks` exactly like the tokenizer's `desc_masks` do in the reference (dataset.py:161-177)."""
    tok, P = dims.tok, dims.pb.point_token_len
    dev = pcrgbs.device
    B, Ld = desc_ids.shape
    dm = torch.ones(B, Ld, dtype=torch.bool, device=dev) if desc_mask is None else desc_mask.to(dev).bool()
    h = Ld // 2
    col = lambda v: torch.full((B, 1), v, dtype=torch.int64, device=dev)
    one = torch.ones(B, 1, dtype=torch.bool, device=dev)
    head = torch.cat([col(tok.bos), desc_ids[:, :h], col(tok.point_start), torch.full((B, P), tok.point_patch, dtype=torch.int64, device=dev),
                      col(tok.point_end), desc_ids[:, h:]], 1)
    head_mask = torch.cat([one, dm[:, :h], one, torch.ones(B, P, dtype=torch.bool, device=dev), one, dm[:, h:]], 1)
    tt, tm = T.tokenize_batch(trajs, tok, max_traj_token, steps=steps)
    return collate(dims, image_ids if image_ids is not None else torch.arange(B, device=dev), pcrgbs, head, head_mask, tt, tm,
                   trajs if gt_trajs is None else gt_trajs, torch.ones(B, 6, device=dev) if max_abs is None else max_abs, sep_ids)


class SyntheticTrajData:
    """Seeded synthetic samples: RGB-D clip -> un-projection -> 8192-point cloud (A1, A2 on the device), uniform description
    ids of varying length (padded to `max_desc_token` with mask False when that is set), smooth random trajectories in
    workspace metres / rotation vectors that go through `norm` (traj.TargetNorm: --do_norm / --do_standard / neither)."""

    def __init__(self, dims, n_samples, frames=2, size=64, text_len=16, num_steps=20, seed=42, norm=None, max_desc_token=None,
                 ragged_text=False):
        self.dims, self.n, self.frames, self.size, self.text_len, self.num_steps, self.seed = dims, n_samples, frames, size, text_len, num_steps, seed
        self.norm = norm if norm is not None else T.TargetNorm()
        self.max_desc, self.ragged = max_desc_token, ragged_text

    def __len__(self):
        return self.n

    def raw_traj(self, i):
        """[num_steps, 6]: in [-1,1] for mode 'none', else workspace metres + rotation vectors (radians)."""
        g = synth._rng(self.seed + int(i), 0xDA7A)
        desc = g.integers(3, min(self.dims.tok.point_patch, self.dims.lm.vocab_size), size=self.text_len)
        base = g.uniform(-0.6, 0.6, size=(1, 6))
        walk = np.clip(base + np.cumsum(g.normal(0, 0.03, size=(self.num_steps, 6)), 0), -1, 1)
        n_real = int(g.integers(max(2, self.text_len // 2), self.text_len + 1)) if self.ragged else self.text_len
        return desc, n_real, (walk if self.norm.mode == "none" else T.denorm(walk[None])[0])

    def fit_norm(self, save_dir=None):
        """train split with --do_standard: compute_mean_std + norm_param.json (dataset.py:58-66,80-111)."""
        self.norm.fit([self.raw_traj(i)[2] for i in range(self.n)], self.num_steps)
        if save_dir is not None:
            self.norm.save(save_dir)
        return self.norm

    def batch(self, idx, device, max_traj_token=160):
        dims, H = self.dims, self.size
        clips = [synth.synth_clip(int(i), self.frames, H, H, self.seed) for i in idx]
        rgb = torch.from_numpy(np.stack([c[0] for c in clips])).to(device)
        depth = torch.from_numpy(np.stack([c[1] for c in clips])).to(device)
        f, pp = synth.clip_intrinsics(H)
        pts, col, cnt = ops.unproject_gather(rgb, depth, pp, f, f, synth.DEPTH_THRESHOLD, n_out=dims.pb.npoints)
        if int(cnt.min()) < dims.pb.npoints:
            raise ValueError("clip has fewer valid pixels than npoints")
        pc = ops.pc_norm(pts, col)
        Ld = self.text_len if self.max_desc is None else int(self.max_desc)
        Ld += Ld % 2
        desc = np.full((len(idx), Ld), dims.tok.pad, dtype=np.int64)
        dmask = np.zeros((len(idx), Ld), dtype=bool)
        trs, gts, mabs = [], [], []
        for j, i in enumerate(idx):
            d, n_real, raw = self.raw_traj(i)
            n_real = min(n_real, Ld)                                   # --max_desc_token truncates (dataset.py:48)
            desc[j, :n_real], dmask[j, :n_real] = d[:n_real], True
            v, m = self.norm.normalize(raw)
            trs.append(np.clip(v, -1, 1))
            gts.append(raw)
            mabs.append(m)
        to = lambda a, dt: torch.from_numpy(np.stack(a).astype(dt)).to(device)
        return build_batch(dims, torch.from_numpy(desc).to(device), to(trs, np.float32), pc, max_traj_token,
                           image_ids=torch.as_tensor([int(i) for i in idx], device=device), desc_mask=torch.from_numpy(dmask).to(device),
                           max_abs=to(mabs, np.float32), gt_trajs=to(gts, np.float32))


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def micro_batch_per_rank(bs, grad_accum_steps, world):
    """DeepSpeed arithmetic of train.py:92-96: train_batch_size = bs = micro * grad_accum_steps * world."""
    return max(1, -(-int(bs) // (max(1, int(grad_accum_steps)) * max(1, int(world)))))


def check_val_options(K, num_beams, sample, select, rescore, M, radius, soft, decoding_rules=True, full=False, constrain=False):
    """The rules of --num_samples / --select / --rescore / --num_modes / --mode_radius / --soft_decode on their resolved values, one text
    per rule; raises ValueError.  run_validation applies all of them; parse_args applies the first four (decoding_rules=False) and exits
    on them: the last four stay errors of the run itself (main() raises ValueError there, and tests pin that).  --full_metrics goes with
    every decoding mode: `full` has no rule."""
    if constrain and num_beams != 1:
        raise ValueError("--constrain_traj masks the logits row of every sample: it needs num_beams == 1 (beams share one prefill row)")
    if soft and num_beams != 1:
        raise ValueError("--soft_decode reads the per-step distribution of sampled or greedy decoding: it needs num_beams == 1")
    if M < 0 or (M > 0 and not (K > 1 and M <= K <= 64)):
        raise ValueError(f"--num_modes M picks M of K samples: it needs --num_samples K > 1 and 1 <= M <= K <= 64, not M = {M}, K = {K}")
    if radius != radius or radius < 0 or (radius > 0 and M == 0):
        raise ValueError(f"--mode_radius is a distance >= 0 and needs --num_modes M > 0, not {radius} with M = {M}")
    if rescore and not (K > 1 and select == "logprob"):
        raise ValueError("--rescore re-ranks sampled trajectories by log-prob: it needs --num_samples K > 1 and --select logprob")
    if not decoding_rules:
        return
    if K < 1:
        raise ValueError(f"num_samples has to be a strictly positive integer, but is {K}")
    if K > 1 and (num_beams != 1 or not sample):
        raise ValueError("num_samples > 1 draws samples: it cannot be combined with --val_greedy or --num_beams > 1")
    if select not in ("none", "logprob", "medoid"):
        raise ValueError(f"select must be none, logprob or medoid, not {select!r}")
    if select != "none" and K < 2:
        raise ValueError("--select chooses among samples: it needs --num_samples K > 1")


def val_options(args, num_beams=1, num_samples=None, select=None, num_modes=None, mode_radius=None, soft_decode=None, full_metrics=None,
                constrain_traj=None):
    """run_validation's options, each resolved as: the explicit keyword, else `args`, else its default; checked (check_val_options)."""
    pick = lambda explicit, name, default: explicit if explicit is not None else (getattr(args, name, default) or default)
    o = types.SimpleNamespace(K=int(pick(num_samples, "num_samples", 1)), num_beams=num_beams, sample=bool(getattr(args, "val_sample", True)),
                              select=str(pick(select, "select", "none")), rescore=bool(getattr(args, "rescore", False)),
                              M=int(pick(num_modes, "num_modes", 0)), radius=float(pick(mode_radius, "mode_radius", 0.0)),
                              soft=bool(pick(soft_decode, "soft_decode", False)), full=bool(pick(full_metrics, "full_metrics", False)),
                              constrain=bool(pick(constrain_traj, "constrain_traj", False)))
    check_val_options(**vars(o))
    return o


# what run_validation sums over the parsed clips of every rank, by name and in the order of the all-reduced tensor
BASE_SUMS = ("ADE", "FDE", "ADE_as_called", "GD", "n")
BEST_SUMS = ("minADE", "minFDE", "n_min")
SEL_SUMS = ("ADE_sel", "FDE_sel", "n_sel")
MODE_SUMS = ("minADE_M", "minFDE_M", "brierADE_M", "n_M", "modes", "clips_M")      # n_M: clips with a mode; modes over clips_M clips
LIMIT_SUMS = ("n_limit_viol", "lmass_min", "n_lmass")                             # violating bin tokens (all rows); per clip the smallest limits mass
GRAMMAR_SUMS = ("gmass_mean", "gmass_min", "n_gmass")                             # per clip: mean and smallest per-step mass of the allowed set
SOFT_SUMS = ("ADE_soft", "FDE_soft", "n_soft", "std", "n_std", "mass_min")        # std over n_std coordinates; the smallest masses
FULL_SUMS = ("IDE", "DTW", "GD_dev", "n_full", "minIDE", "minGD", "minDTW", "n_fmin", "GD_sel", "DTW_sel", "n_fsel", "minGD_M", "minDTW_M", "n_fM")


def _add(sums, **terms):
    for name, v in terms.items():
        sums[name] += float(v)                               # float64, whatever the term's own type


def _mean(sums, name, count):
    """sums[name] / sums[count] as a plain float (the records go into checkpoints read with weights_only=True), NaN without a count."""
    return float(sums[name] / sums[count]) if sums[count] else float("nan")


def reduce_sums(sums, device):
    """The sums of all ranks: one float64 tensor in the mapping's order, all-reduced and read back by name."""
    t = torch.tensor(list(sums.values()), dtype=torch.float64).to(device)
    dist.all_reduce(t)
    return dict(zip(sums, t.cpu().tolist()))


def pad_last_step(vals, n):
    """Rows of vals [R, Tn, ...] (numpy, in place) with 0 < n[r] < Tn parsed steps repeat step n[r] - 1 from n[r] on (train.py:252-256)."""
    for r in range(len(vals)):
        if 0 < n[r] < vals.shape[1]:
            vals[r, n[r]:] = vals[r, n[r] - 1]
    return vals


def parse_trajectories(ids, tok, num_steps, Tn, norm, max_abs, device):
    """Token ids (the prompt's last seven tokens, which hold step 0 + <tsep>, then the generated ones) [R, L] -> the de-normalised
    trajectories: de-tokenise, clamp to the Tn ground-truth steps, pad with the last parsed step, norm.denorm with max_abs [R, 6] (numpy).
    -> (numpy [R, Tn, 6], its fp32 device copy, parsed steps per row numpy [R]; 0 = detokenize_traj returned None, train.py:249-250)."""
    vals, n = T.detokenize_batch(ids, tok, num_steps + 4)
    n_h = torch.clamp(n, max=Tn).cpu().numpy()
    gen = norm.denorm(pad_last_step(vals[:, :Tn].cpu().numpy(), n_h), max_abs)
    return gen, torch.from_numpy(np.ascontiguousarray(gen, dtype=np.float32)).to(device), n_h


def _six(text, name, n=6):
    """`a,b,...` -> n floats; an empty field or `none` = no limit there (NaN)."""
    parts = [v.strip() for v in str(text).split(",")]
    if len(parts) != n:
        raise ValueError(f"{name} takes {n} comma-separated numbers, not {text!r}")
    try:
        return [float("nan") if v.lower() in ("", "none") else float(v) for v in parts]
    except ValueError:
        raise ValueError(f"{name} takes {n} comma-separated numbers, not {text!r}") from None


def traj_limit_options(args, constrain):
    """--traj_workspace / --traj_max_step resolved: None with both off, else (lo [6], hi [6], max_step [6]) in the units of the
    de-normalised trajectories, NaN = no limit (the workspace bounds x, y, z only).  Both need --constrain_traj; raises ValueError."""
    ws, ms = getattr(args, "traj_workspace", None), getattr(args, "traj_max_step", None)
    if ws is None and ms is None:
        return None
    if not constrain:
        raise ValueError("--traj_workspace / --traj_max_step narrow the bin window of constrained decoding: they need --constrain_traj")
    nan = float("nan")
    lo, hi, step = [nan] * 6, [nan] * 6, [nan] * 6
    if ws is not None:
        w = _six(ws, "--traj_workspace")
        lo[:3], hi[:3] = w[0::2], w[1::2]
        if any(a > b for a, b in zip(lo[:3], hi[:3])):
            raise ValueError(f"--traj_workspace is x0,x1,y0,y1,z0,z1 with x0 <= x1, y0 <= y1, z0 <= z1, not {ws!r}")
    if ms is not None:
        step = _six(ms, "--traj_max_step")
        if any(v < 0 for v in step):
            raise ValueError(f"--traj_max_step is six distances >= 0, not {ms!r}")
    return lo, hi, step


def generate_kwargs(o, args, tok):
    """generate()'s keyword arguments for the decoding mode: K samples on a shared prompt, beams, or neither; the bin statistics."""
    kw = {"output_bin_stats": True, "bin_token_ids": (tok.p0, tok.num_bins)} if o.soft else {}
    if o.constrain:                                          # the prompt holds the first step: it counts among the num_steps
        kw["traj_grammar"] = T.grammar_spec(tok, args.num_steps, args.num_steps)
    if o.K > 1:
        kw.update(num_return_sequences=o.K, share_prompt=True, **({"output_logprobs": True} if o.select == "logprob" else {}))
    elif o.num_beams != 1:
        kw.update(num_beams=o.num_beams, kv_cache_layout=getattr(args, "kv_cache_layout", None))
    return kw


def generate_batch(model, data, args, device, o, idx, norm):
    """One batch of the pass: generate() for the clips idx, and all its K * len(idx) rows parsed (row b * K + j = sample j of clip b)."""
    tok = model.dims.tok
    batch = data.batch(idx, device, args.max_traj_token)
    prompts, gt = batch["prompts"], batch["trajectories"]
    fps0 = torch.zeros(len(idx), dtype=torch.int32, device=device)
    lim = None
    if o.limits is not None:                                 # physical limits -> bins, per clip (its own max_abs under --do_standard)
        lim = T.motion_limits(tok, norm, *o.limits, max_abs=batch["max_abs"].cpu().numpy())
    out = model.generate(input_ids=prompts, attention_mask=batch["prompt_masks"], point_clouds=batch["pcrgbs"],
                         max_length=batch["tokens"].shape[1] - prompts.shape[1], do_sample=o.sample, fps_start=fps0,
                         kv_cache_dtype=getattr(args, "kv_cache_dtype", None),
                         decode_weight_dtype=getattr(args, "decode_weight_dtype", None), **generate_kwargs(o, args, tok),
                         **({} if lim is None else {"traj_limits": lim}))
    all_ids = out.sequences[:, prompts.shape[1]:]
    head = prompts[:, -7:]                                   # the prompt holds the first step; with its <tsep> it is parsed like the rest
    mabs = batch["max_abs"].cpu().numpy()
    gen, gen_d, n_h = parse_trajectories(torch.cat([head.repeat_interleave(o.K, 0), all_ids], 1), tok, args.num_steps, gt.shape[1], norm,
                                         np.repeat(mabs, o.K, axis=0), device)
    return types.SimpleNamespace(batch=batch, prompts=prompts, head=head, gt=gt, gt_h=gt.cpu().numpy(), mabs=mabs, fps0=fps0, out=out,
                                 all_ids=all_ids, ids_h=batch["image_ids"].cpu().numpy(), gen=gen, gen_d=gen_d, n_h=n_h, lim=lim,
                                 gen_k=gen_d.view(len(idx), o.K, gt.shape[1], -1),
                                 n_k=torch.from_numpy((n_h > 0).astype(np.int32) * gt.shape[1]).to(device).view(len(idx), o.K))


# -- the parts: each adds one batch to the sums and the dump, and turns its sums into its record keys -----------------------------------
def base_batch(o, b, sums, dump):
    """Sample 0 of every clip (K = 1: every row): ADE / FDE / ADE_as_called / GD over the parsed ones; the dump's trajectory."""
    gen, n_h = b.gen[::o.K], b.n_h[::o.K]
    ade, fde = (t.cpu().numpy() for t in T.metrics_batch(b.gen_d[::o.K], None, b.gt))
    for j in range(len(gen)):
        if n_h[j] <= 0:
            continue
        _add(sums, ADE=ade[j], FDE=fde[j], ADE_as_called=T.average_displacement_error(gen[j][None], b.gt_h[j][None]),
             GD=T.anglar_distance(gen[j][:, 3:6].astype(np.float64), b.gt_h[j][:, 3:6].astype(np.float64)), n=1)
        dump[int(b.ids_h[j])] = gen[j].tolist()              # evaluate.py:150: keyed by image_id.item(), not by the dataset index


def base_record(o, sums):
    return {"ADE": _mean(sums, "ADE", "n"), "FDE": _mean(sums, "FDE", "n"), "ADE_as_called": _mean(sums, "ADE_as_called", "n"),
            "GD": _mean(sums, "GD", "n"), "n": int(sums["n"])}


def best_of_batch(o, b, sums, dump):
    """All K samples of every clip: minADE / minFDE; the dump keeps the K trajectories (None for an unparsed one)."""
    made, mfde, best = (t.cpu().numpy() for t in T.metrics_best_of(b.gen_k, b.n_k, b.gt))
    for j in range(len(best)):
        if best[j] >= 0:
            _add(sums, minADE=made[j], minFDE=mfde[j], n_min=1)
        dump[int(b.ids_h[j])] = [b.gen[j * o.K + i].tolist() if b.n_h[j * o.K + i] > 0 else None for i in range(o.K)]


def best_of_record(o, sums):
    return {"minADE": _mean(sums, "minADE", "n_min"), "minFDE": _mean(sums, "minFDE", "n_min"), "n_min": int(sums["n_min"]), "K": o.K}


def sample_ranking(model, o, b):
    """What ranks the K samples of select "logprob" (and orders the modes): generate()'s own log-probs, with o.rescore model.score() on
    the same samples (the model's own weights); None for any other select."""
    if o.select != "logprob":
        return None
    if not o.rescore:
        return b.out
    return model.score(b.prompts, b.batch["prompt_masks"], b.batch["pcrgbs"], b.all_ids.reshape(len(b.ids_h), o.K, -1), fps_start=b.fps0)


def select_batch(o, b, ranked, sums, picked):
    """The one of K a user without the ground truth would keep: its ADE / FDE; picked[image id] = its index."""
    pick = ranked.rank[:, 0].contiguous() if o.select == "logprob" else T.select_medoid(b.gen_k, b.n_k)[0]
    sade, sfde, pick = (t.cpu().numpy() for t in (*T.metrics_selected(b.gen_k, b.n_k, b.gt, None, pick), pick))
    for j in range(len(pick)):
        picked[int(b.ids_h[j])] = int(pick[j])
        if not np.isnan(sade[j]):
            _add(sums, ADE_sel=sade[j], FDE_sel=sfde[j], n_sel=1)


def select_record(o, sums):
    return {"ADE_sel": _mean(sums, "ADE_sel", "n_sel"), "FDE_sel": _mean(sums, "FDE_sel", "n_sel"), "n_sel": int(sums["n_sel"]),
            "select": o.select}


def modes_batch(o, b, ranked, sums, mode_dump):
    """M different ones of the K, ordered by the ranking's scores or by centrality: their best-of metrics; indices and probabilities."""
    md, cf, _, nmd, _ = T.select_modes(b.gen_k, b.n_k, None if ranked is None else ranked.sample_scores, o.M, o.radius)
    oade, ofde, slot, brier = (t.cpu().numpy() for t in T.metrics_modes(b.gen_k, b.n_k, b.gt, None, md, cf))
    md, cf, nmd = md.cpu().numpy(), cf.cpu().numpy(), nmd.cpu().numpy()
    for j in range(len(nmd)):
        mode_dump[int(b.ids_h[j])] = {"index": md[j, :nmd[j]].tolist(), "conf": cf[j, :nmd[j]].tolist()}
        _add(sums, modes=nmd[j], clips_M=1)
        if slot[j] >= 0:
            _add(sums, minADE_M=oade[j], minFDE_M=ofde[j], brierADE_M=brier[j], n_M=1)


def modes_record(o, sums):
    return {"minADE_M": _mean(sums, "minADE_M", "n_M"), "minFDE_M": _mean(sums, "minFDE_M", "n_M"),
            "brierADE_M": _mean(sums, "brierADE_M", "n_M"), "n_modes": _mean(sums, "modes", "clips_M"), "M": o.M, "mode_radius": o.radius}


def grammar_batch(o, b, tok, sums):
    """Sample 0 of every clip: the mean and the smallest raw probability its steps gave the ids the grammar allowed, up to its eos."""
    from .decode import candidate_lengths
    mass = b.out.grammar_mass[::o.K].double()
    lens = candidate_lengths(b.all_ids[::o.K], tok.eos).clamp(min=1)
    live = torch.arange(mass.shape[1], device=mass.device)[None, :] < lens[:, None]
    mean = (mass * live).sum(1) / lens
    low = mass.masked_fill(~live, float("inf")).min(1).values
    _add(sums, gmass_mean=mean.sum(), gmass_min=low.sum(), n_gmass=len(mean))


def limits_batch(o, b, tok, sums):
    """Every row: the bin tokens it generated outside their window (T.limits_violations, the host restatement of the kernel's rule; the
    prompt's own tokens only move the pose); sample 0 of every clip: the smallest raw probability a step left inside the limits."""
    from .decode import candidate_lengths
    S0 = b.prompts.shape[1]
    viol = T.limits_violations(b.out.sequences.cpu(), tok, b.lim.repeat_interleave(o.K, 0), start=S0)
    mass = b.out.limits_mass[::o.K].double()
    lens = candidate_lengths(b.all_ids[::o.K], tok.eos).clamp(min=1)
    live = torch.arange(mass.shape[1], device=mass.device)[None, :] < lens[:, None]
    low = mass.masked_fill(~live, float("inf")).min(1).values
    _add(sums, n_limit_viol=int(viol.sum()), lmass_min=low.sum(), n_lmass=len(low))


def limits_record(o, args, sums):
    return {"n_limit_viol": int(sums["n_limit_viol"]), "limits_mass_min": _mean(sums, "lmass_min", "n_lmass"),
            "traj_workspace": getattr(args, "traj_workspace", None), "traj_max_step": getattr(args, "traj_max_step", None)}


def grammar_record(o, sums):
    return {"grammar_mass_mean": _mean(sums, "gmass_mean", "n_gmass"), "grammar_mass_min": _mean(sums, "gmass_min", "n_gmass")}


def soft_batch(o, b, tok, num_steps, norm, sums, soft_dump):
    """Sample 0 of every clip again, from the distributions its tokens were drawn from: the soft trajectory and its std."""
    device, Tn = b.head.device, b.gt.shape[1]
    isbin = (b.head >= tok.p0) & (b.head < tok.p0 + tok.num_bins)   # the prompt's step: its bin centres, std 0, mass 1
    centre = T.bin_edges(tok.num_bins, device)[(b.head - tok.p0).clamp(0, tok.num_bins - 1)].float()
    zero = torch.zeros_like(centre)
    smean, sstd, smass, sn = T.detokenize_soft(torch.cat([b.head, b.all_ids[::o.K]], 1), tok, num_steps + 4,
                                               torch.cat([torch.where(isbin, centre, zero), b.out.bin_mean[::o.K]], 1),
                                               torch.cat([zero, b.out.bin_std[::o.K]], 1), torch.cat([zero + 1, b.out.bin_mass[::o.K]], 1))
    sn_h, smass_h = torch.clamp(sn, max=Tn).cpu().numpy(), smass[:, :Tn].cpu().numpy()
    sgen = norm.denorm(pad_last_step(smean[:, :Tn].cpu().numpy(), sn_h), b.mabs)
    sstd_h = pad_last_step(sstd[:, :Tn].cpu().numpy(), sn_h) * norm.denorm_scale(b.mabs)[:, None, :]
    sade, sfde = (t.cpu().numpy() for t in T.metrics_batch(torch.from_numpy(np.ascontiguousarray(sgen, dtype=np.float32)).to(device), None, b.gt))
    for j in range(len(sn_h)):
        if sn_h[j] <= 0:
            continue
        _add(sums, ADE_soft=sade[j], FDE_soft=sfde[j], n_soft=1, std=sstd_h[j, :sn_h[j], :3].sum(), n_std=3.0 * sn_h[j],
             mass_min=smass_h[j, :sn_h[j]].min())
        soft_dump[int(b.ids_h[j])] = {"mean": sgen[j].tolist(), "std": sstd_h[j].tolist()}


def soft_record(o, sums):
    return {"ADE_soft": _mean(sums, "ADE_soft", "n_soft"), "FDE_soft": _mean(sums, "FDE_soft", "n_soft"), "n_soft": int(sums["n_soft"]),
            "sigma_mean": _mean(sums, "std", "n_std"), "bin_mass_min": _mean(sums, "mass_min", "n_soft")}


def full_batch(o, b, sums, full_dump, picked, mode_dump):
    """All K samples of every clip once more, through the whole metric module (T.metrics_full, one launch): IDE / DTW / GD of sample 0, the
    per-clip minima, and the values at the pick (picked) and over the modes (mode_dump) that select_batch / modes_batch left for the clip.
    The rows carry their parsed step counts, 0 for an unparsed one: they are padded with their last step already, which ADE, FDE and GD
    would repeat anyway and DTW must not see."""
    n = torch.from_numpy(np.ascontiguousarray(b.n_h, dtype=np.int32)).to(b.gen_k.device).view(len(b.ids_h), o.K)
    m = T.metrics_full(b.gen_k, n, b.gt)
    vals = np.stack([t.cpu().numpy() for t in m[:len(T.FULL_METRICS)]], axis=-1)          # [clips, K, 5]
    mins, args = m.mins.cpu().numpy(), m.args.cpu().numpy()
    IDE, GD, DTW = (T.FULL_METRICS.index(c) for c in ("IDE", "GD", "DTW"))
    for j in range(len(b.ids_h)):
        iid = int(b.ids_h[j])
        full_dump[iid] = {name: [None if np.isnan(v) else float(v) for v in vals[j, :, c]] for c, name in enumerate(T.FULL_METRICS)}
        if b.n_h[j * o.K] > 0:
            _add(sums, IDE=vals[j, 0, IDE], DTW=vals[j, 0, DTW], GD_dev=vals[j, 0, GD], n_full=1)
        if o.K > 1 and args[j, 0] >= 0:
            _add(sums, minIDE=mins[j, IDE], minGD=mins[j, GD], minDTW=mins[j, DTW], n_fmin=1)
        if o.select != "none" and picked[iid] >= 0 and b.n_h[j * o.K + picked[iid]] > 0:
            _add(sums, GD_sel=vals[j, picked[iid], GD], DTW_sel=vals[j, picked[iid], DTW], n_fsel=1)
        if o.M and mode_dump[iid]["index"]:
            rows = vals[j, mode_dump[iid]["index"]]
            _add(sums, minGD_M=rows[:, GD].min(), minDTW_M=rows[:, DTW].min(), n_fM=1)


def full_record(o, sums):
    rec = {"IDE": _mean(sums, "IDE", "n_full"), "DTW": _mean(sums, "DTW", "n_full"), "GD_dev": _mean(sums, "GD_dev", "n_full"),
           "n_full": int(sums["n_full"])}
    if o.K > 1:
        rec.update({"min" + c: _mean(sums, "min" + c, "n_fmin") for c in ("IDE", "GD", "DTW")})
    if o.select != "none":
        rec.update(GD_sel=_mean(sums, "GD_sel", "n_fsel"), DTW_sel=_mean(sums, "DTW_sel", "n_fsel"))
    if o.M:
        rec.update(minGD_M=_mean(sums, "minGD_M", "n_fM"), minDTW_M=_mean(sums, "minDTW_M", "n_fM"))
    return rec


def rank_batches(n, per, rank, world, max_batches=None):
    """The clips of this rank, batch by batch.  The reference's val / test DataLoader (train.py:79-82, evaluate.py:93-100: batch_size=bs,
    shuffle=False, NO drop_last) keeps the short last batch: every sample is generated for and lands in the dump.  A batch is dealt over
    the ranks; the short one is split raggedly and a rank whose share is empty skips it (the only collective of the pass is the
    all-reduce of the sums)."""
    gb = per * world
    nb = -(-n // gb)
    for bi in range(nb if max_batches is None else min(nb, max_batches)):
        n_here = min(gb, n - bi * gb)
        lo, hi = shard_range(gb, rank, world) if n_here == gb else ragged_shard_range(n_here, rank, world)
        if hi > lo:
            yield list(range(bi * gb + lo, bi * gb + hi))


@torch.no_grad()
def run_validation(model, data, args, device, max_batches=None, num_beams=1, num_samples=None, select=None, num_modes=None, mode_radius=None,
                   soft_decode=None, full_metrics=None, constrain_traj=None):
    """Generation + metrics on the rank's shard (train.py:207-264, evaluate.py:104-154): prompts up to the first <tsep>,
    `generate` of the remaining positions (sampling with the reference's defaults top_k 50 / top_p 0.95 / T 1.0 unless
    args.val_sample is False -> greedy), cut at eos, de-tokenise, de-normalise (dataset.denorm), pad with the last step,
    ADE / FDE / GD; sums are all-reduced over ranks so that every rank (and the best-checkpoint choice) sees the same means.

    Metrics: 'ADE'/'FDE' use the documented [T,D] form of metrics.py:38-55,7-27; 'ADE_as_called' is what the reference's
    drivers log (they pass [1,T,6], so the norm runs over TIME: SURVEY.md §0.1); 'GD' is metrics.py:61-87 on the rotation
    vectors [T,3] (the reference's own call passes [1,T,6] and raises inside scipy).

    num_beams > 1 (eval only): beam search (or beam sampling with the sampling flags) with one returned hypothesis per sample, the best.

    num_samples = K > 1 (default: args.num_samples, else 1): K sampled trajectories per clip from ONE prefill and one cached prompt per clip
    (generate(num_return_sequences=K, share_prompt=True)); sampling only, not with num_beams > 1.  'ADE' / 'FDE' / 'ADE_as_called' / 'GD' /
    'n' are those of sample 0 of every clip, computed as with K = 1; the record gains 'minADE' / 'minFDE' (best-of-K, T.metrics_best_of;
    means over the 'n_min' clips with at least one parsed sample) and 'K', and the dump holds the K trajectories per image id (None for
    an unparsed one).  K = 1 is the single-draw path unchanged.

    select (default: args.select, else "none") with K > 1: which of the K a user without the ground truth would keep, chosen on the device.
    "logprob" = the sample the model finds most probable (generate(output_logprobs=True).rank[:, 0]: highest mean token log-prob under the
    raw logits); "medoid" = the most central sample (T.select_medoid: smallest mean ADE to the other parsed samples).  The record gains
    'ADE_sel' / 'FDE_sel' (T.metrics_selected; means over the 'n_sel' clips whose pick parsed) and 'select'; the dump gains one key,
    "selected": {image id: picked sample index}.  "none" leaves the record and the dump as they are.
    args.rescore with select "logprob": the rank comes from model.score() on the generated samples (the exact model's teacher-forced
    log-probs; one more pass over the K suffixes of every clip) instead of the sampling run's own log-probs.

    num_modes = M > 0 (default: args.num_modes, else 0 = off) with 1 <= M <= K <= 64 and K > 1: a short list of M mutually different samples
    per clip, each with a probability (T.select_modes on the de-normalised trajectories, all D dimensions; mode_radius, default
    args.mode_radius, else 0, is in their units).  The order is that of the scores select "logprob" ranks by (with args.rescore those of
    model.score()), otherwise centrality.  The record gains 'minADE_M' / 'minFDE_M' / 'brierADE_M' (T.metrics_modes; means over the clips
    with a mode), 'n_modes' (mean number of modes per clip), 'M' and 'mode_radius'; the dump gains one key,
    "modes": {image id: {"index": [sample indices in pick order], "conf": [their probabilities]}}.  0 leaves both as they are.

    soft_decode (default: args.soft_decode, else False; num_beams == 1): generate(output_bin_stats=True) and, for sample 0 of every clip, the
    soft trajectory beside the hard one: every coordinate is the conditional mean over the bins of the distribution its token was drawn
    from (T.detokenize_soft; the step held by the prompt takes its bin centres, std 0, mass 1) instead of the drawn bin's centre.  It goes
    through the same norm.denorm; the std is scaled by |its linear factor| (TargetNorm.denorm_scale: denorm is affine per dimension in every
    mode).  The record gains 'ADE_soft' / 'FDE_soft' / 'n_soft' (T.metrics_batch, means over the parsed rows exactly as 'ADE' / 'FDE' / 'n'),
    'sigma_mean' (the mean std over the parsed waypoints' x, y, z, in denorm's units) and 'bin_mass_min' (the mean over the parsed clips of
    the smallest per-step bin mass); the dump gains one key, "soft": {image id: {"mean": [[6] per step], "std": [[6] per step]}}.

    full_metrics (default: args.full_metrics, else False; every decoding mode): the reference's whole metric module for all K samples of
    every clip in one launch per batch (T.metrics_full on the parsed step counts; DTW sees no padding).  The record gains 'IDE' / 'DTW' /
    'GD_dev' / 'n_full' (sample 0, means over the parsed rows as 'ADE' / 'n'; 'GD_dev' is the device's value of the host-computed 'GD',
    which stays), with K > 1 'minIDE' / 'minGD' / 'minDTW' (means over the clips with a parsed sample), with select 'GD_sel' / 'DTW_sel'
    (the pick's values) and with num_modes 'minGD_M' / 'minDTW_M' (minima over the chosen samples); the dump gains one key,
    "full": {image id: {"ADE": [K values], "FDE": ..., "IDE": ..., "GD": ..., "DTW": ...}} with None for an unparsed sample.  Off, the
    record and the dump are what they are without it.

    constrain_traj (default: args.constrain_traj, else False; num_beams == 1): generate(traj_grammar=T.grammar_spec(tok, num_steps, num_steps)):
    every generated row is a well-formed trajectory of exactly args.num_steps steps, the prompt's first step included (the state is read
    from the prompt).  The record gains 'grammar_mass_mean' and 'grammar_mass_min': the mean over the clips (sample 0) of the mean, and of
    the smallest, raw probability that a step gave the ids the grammar allowed -- how much of the model's own mass the constraint kept.
    Off, every record, dump and bit is what it is without it.

    args.traj_workspace "x0,x1,y0,y1,z0,z1" / args.traj_max_step "dx,dy,dz,rx,ry,rz" (both optional, both need constrain_traj; units of the
    de-normalised trajectories; an empty field = no limit there): generate(traj_limits=T.motion_limits(...)), the limits converted to bins
    per clip with conservative rounding and enforced on the device at every bin token.  The record gains 'n_limit_viol' (bin tokens outside
    their window over all rows, counted by T.limits_violations on the host: it must be 0), 'limits_mass_min' (as 'grammar_mass_min', of the
    probability the limits left allowed) and the two settings.  Off, every record, dump, launch and bit is what it is without them."""
    o = val_options(args, num_beams, num_samples, select, num_modes, mode_radius, soft_decode, full_metrics, constrain_traj)
    o.limits = traj_limit_options(args, o.constrain)
    rank, world = _rank_world()
    norm = getattr(data, "norm", None) or T.TargetNorm()
    sums = dict.fromkeys(BASE_SUMS + BEST_SUMS + SEL_SUMS + MODE_SUMS + SOFT_SUMS + FULL_SUMS + GRAMMAR_SUMS + LIMIT_SUMS, 0.0)
    dump, picked, mode_dump, soft_dump, full_dump = {}, {}, {}, {}, {}
    model.eval()
    for idx in rank_batches(len(data), micro_batch_per_rank(args.bs, 1, world), rank, world, max_batches):
        b = generate_batch(model, data, args, device, o, idx, norm)
        base_batch(o, b, sums, dump)
        if o.constrain:
            grammar_batch(o, b, model.dims.tok, sums)
        if o.limits is not None:
            limits_batch(o, b, model.dims.tok, sums)
        if o.soft:
            soft_batch(o, b, model.dims.tok, args.num_steps, norm, sums, soft_dump)
        if o.K > 1:
            best_of_batch(o, b, sums, dump)
        ranked = sample_ranking(model, o, b)
        if o.select != "none":
            select_batch(o, b, ranked, sums, picked)
        if o.M:
            modes_batch(o, b, ranked, sums, mode_dump)
        if o.full:
            full_batch(o, b, sums, full_dump, picked, mode_dump)
    if world > 1:
        sums = reduce_sums(sums, device)
    model.train()
    rec = base_record(o, sums)
    if o.K > 1:
        rec.update(best_of_record(o, sums))
    if o.select != "none":
        rec.update(select_record(o, sums))
        dump["selected"] = picked
    if o.M:
        rec.update(modes_record(o, sums))
        dump["modes"] = mode_dump
    if o.soft:
        rec.update(soft_record(o, sums))
        dump["soft"] = soft_dump
    if o.full:
        rec.update(full_record(o, sums))
        dump["full"] = full_dump
    if o.constrain:
        rec.update(grammar_record(o, sums))
    if o.limits is not None:
        rec.update(limits_record(o, args, sums))
    return rec, dump


def train(args, model, train_data, val_data=None, device="cuda", log=print, step_log=None):
    """train.py:129-310.  Returns the list of per-epoch records.  step_log (optional): called once per optimizer step with
    {"epoch", "step", "learning_rate", "loss"} — the reference's per-step wandb.log (train.py:186-193; reading the loss syncs, as its
    `loss.item()` does).

    Batch arithmetic (train.py:92-96): `--bs` is the optimizer batch of the whole job; each rank runs
    `--grad_accum_steps` micro-batches of ceil(bs / accum / world) samples per optimizer step, gradients accumulate in the
    fp32 main_grad buffers, ONE gradient sync + ONE AdamW step follow the last micro-batch (grad scale 1/(accum*world)).
    LR: HF linear schedule with warm-up over int(total/5) steps then decay to 0 (train.py:113-116), advanced once per
    optimizer step, `total` = optimizer steps of the run.  DEVIATION for --grad_accum_steps > 1: the reference sizes the
    schedule in LOADER iterations (num_training_steps = epochs * len(train_dataloader), train.py:114-116) while DeepSpeed advances it
    once per accumulation boundary, so there the warm-up lasts accum x longer and the rate never decays to zero (it ends at
    1 - 1/accum of the way down).  Here the schedule always spans the optimizer steps actually taken; with accum == 1 (the
    reference's default) the two agree step by step (tests/test_host_glue.py pins both statements against HF's scheduler)."""
    rank, world = _rank_world()
    accum = max(1, int(getattr(args, "grad_accum_steps", 1) or 1))
    micro = micro_batch_per_rank(args.bs, accum, world)
    clip = float(getattr(args, "max_grad_norm", 0) or 0)                              # 0: no clipping, nothing below changes
    opt = EgoAdamW(model, lr=float(args.lr_llm), max_grad_norm=clip) if clip > 0 else EgoAdamW(model, lr=float(args.lr_llm))
    sync = GradSync(wire_dtype=torch.bfloat16 if model.engine.dtype == torch.bfloat16 else None, resident=True) if world > 1 else None     # EgoAdamW reads the wire
    if sync is None and model.engine.dtype == torch.bfloat16 and model.engine.any_layer_trainable and model.engine.device.type == "cuda":
        sync = GradSync(wire_dtype=torch.bfloat16, resident=True, local=True)      # one rank, --unfreeze_language_model: bf16 weight gradients in per-layer wire buffers (dp.py), nothing exchanged
    bin_sigma = float(getattr(args, "bin_sigma", 0) or 0)                             # 0: the reference's one-hot loss, nothing below changes
    soft = T.soft_target_spec(model.dims.tok, bin_sigma, getattr(args, "bin_radius", None)) if bin_sigma > 0 else None
    start_epoch, global_step, best_ade = 0, 0, float("inf")
    os.makedirs(args.out_dir, exist_ok=True)
    latest = os.path.join(args.out_dir, "latest_model.pt")
    if getattr(args, "resume", False) and os.path.exists(latest):                      # train.py:138-150
        ck = torch.load(latest, map_location="cpu", weights_only=True)
        model.load_state_dict(ck["model_state_dict"])
        opt.load_state_dict(ck["optimizer_state_dict"])
        start_epoch, global_step, best_ade = ck["epoch"] + 1, ck["global_step"], ck.get("best_ade", best_ade)
        opt.resync_masters()
    if getattr(train_data, "norm", None) is not None and train_data.norm.mode == "standard":     # dataset.py:58-66
        if train_data.norm.mean is None:
            train_data.fit_norm(args.out_dir if rank == 0 else None)
        if val_data is not None and getattr(val_data, "norm", None) is not train_data.norm:
            val_data.norm = train_data.norm
    per_step = micro * accum * world                                                   # samples per optimizer step (== bs when divisible)
    # the reference's train DataLoader (train.py:72-77: batch_size=bs, shuffle=True, NO drop_last) keeps the short last batch of an epoch:
    # len(train_dataloader) = ceil(n / bs) iterations, which is also what sizes its LR schedule (train.py:114-116)
    steps_per_epoch = -(-len(train_data) // per_step)
    total_steps = steps_per_epoch * args.epochs
    history = []
    model.train()
    for epoch in range(start_epoch, args.epochs):
        g = np.random.Generator(np.random.Philox(key=np.array([1234, epoch], dtype=np.uint64)))   # same order on every rank
        order = g.permutation(len(train_data))
        run = torch.zeros((), device=device)
        run_nll = torch.zeros((), device=device) if soft is not None else None
        for it in range(steps_per_epoch):
            # the epoch's last optimizer step may be short (no drop_last, see above).  Its samples are dealt over the micro-batches in the
            # usual order; a micro-batch that does not divide over the ranks is filled up by wrapping around to the start of the epoch's
            # permutation, which is what torch's DistributedSampler(drop_last=False) does, so every rank always runs the SAME number of
            # micro-batches with at least one sample each and joins the same collectives (with one rank nothing is ever padded: the short
            # batch is exactly the reference's)
            n_step = min(per_step, len(train_data) - it * per_step)
            n_mb = min(accum, -(-n_step // (micro * world)))
            for a in range(n_mb):
                base = it * per_step + a * micro * world
                n_micro = min(micro * world, n_step - a * micro * world)
                mb = order[base: base + n_micro]
                if n_micro % world:
                    mb = np.concatenate([mb, order[: world - n_micro % world]])
                lo, hi = shard_range(len(mb), rank, world)
                idx = mb[lo:hi]
                batch = train_data.batch(idx, device, args.max_traj_token)
                last = a == n_mb - 1
                model.accumulate_grads = a > 0                                      # first micro-batch overwrites (optimizer.zero_grad(), train.py:159)
                model.engine.grad_sync = sync if last else None                     # reduce once, after the last micro-batch
                if last and (sync is None or sync.local):                           # one rank: trainable decoder layers are updated under this backward pass
                    opt.arm(grad_scale=1.0 / (n_mb * world), lr=linear_warmup_lr(float(args.lr_llm), global_step, total_steps))
                loss = model.loss_and_backward(batch["tokens"], batch["attention_masks"], batch["pcrgbs"], batch["prompts"].shape[1],
                                               model.dims.tok.pad, fps_start=torch.zeros(len(idx), dtype=torch.int32, device=device),
                                               **({} if soft is None else {"bin_soft": soft}))
                run += loss / n_mb
                if soft is not None:
                    run_nll += model.last_nll / n_mb
            model.accumulate_grads = False
            if sync is not None:
                sync.finish()
            lr_now = linear_warmup_lr(float(args.lr_llm), global_step, total_steps)
            opt.step(grad_scale=1.0 / (n_mb * world), lr=lr_now, overlap=model.engine.any_layer_trainable)    # --unfreeze_language_model: on a side stream,
                                                                                                              # under the next step's forward pass (optim.py)
            if step_log is not None:
                entry = {"epoch": epoch, "step": global_step, "learning_rate": lr_now, "loss": float(loss) if n_mb == 1 else None}
                if clip > 0:
                    entry["grad_norm"] = float(opt.last_grad_norm)
                if soft is not None:                                                    # "loss" is the soft loss, "nll" the hard one of the same rows
                    entry["nll"] = float(model.last_nll) if n_mb == 1 else None
                step_log(entry)
            global_step += 1
        rec = {"epoch": epoch, "train_loss": float(run) / max(1, steps_per_epoch), "global_step": global_step,
               "learning_rate": linear_warmup_lr(float(args.lr_llm), global_step, total_steps)}
        if soft is not None:                                                           # train_loss is the soft loss; train_nll stays comparable with the reference's
            rec.update({"train_nll": float(run_nll) / max(1, steps_per_epoch), "bin_sigma": soft.sigma, "bin_radius": soft.radius})
        if clip > 0:                                                                   # one read of the device-side statistics per epoch
            gs = opt.grad_stats(reset=True)
            rec.update({k: gs[k] for k in ("grad_norm_mean", "grad_norm_max", "clipped_steps", "nonfinite_steps")})
            if gs["nonfinite_steps"]:                                                  # before the checkpoint: a poisoned state must not replace a good file
                raise FloatingPointError(f"epoch {epoch}: the gradient norm was not finite in {gs['nonfinite_steps']} of {gs['steps']} optimizer "
                                         f"steps; masters and moments are poisoned, no checkpoint written")
        if val_data is not None:
            m, _ = run_validation(model, val_data, args, device, max_batches=getattr(args, "val_batches", None))
            rec.update(m)
        if world > 1:
            t = torch.tensor([rec["train_loss"]] + ([rec["train_nll"]] if soft is not None else []), device=device)
            dist.all_reduce(t)
            rec["train_loss"] = float(t[0]) / world
            if soft is not None:
                rec["train_nll"] = float(t[1]) / world
        history.append(rec)
        if rank == 0:
            log(json.dumps(rec))
            ck = {"epoch": epoch, "model_state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                  "optimizer_state_dict": opt.state_dict_cpu(), "scheduler_state_dict": {"last_step": global_step}, "global_step": global_step}
            torch.save(ck, latest)                                                      # train.py:287-296
            if val_data is not None and rec.get("ADE", float("inf")) < best_ade:        # metrics are all-reduced: same choice on any rank
                best_ade = rec["ADE"]
                ck["best_ade"] = best_ade
                torch.save(ck, os.path.join(args.out_dir, "best_model_ade.pt"))         # train.py:298-308
    model.engine.grad_sync = None
    return history


def check_adapter_keys(model, sd, path):
    """The LoRA adapters of a checkpoint must be the ones the --lora_* flags built: same keys, same shapes."""
    from . import lora
    own = {k: tuple(v.shape) for k, v in model.state_dict().items() if lora.is_adapter(k)}
    got = {k: tuple(v.shape) for k, v in sd.items() if lora.is_adapter(k)}
    if own == got:
        return
    if got and not own:
        raise ValueError(f"{path} holds LoRA adapters ({len(got)} tensors): pass the --lora_r / --lora_alpha / --lora_target_modules it was trained with")
    if own and not got:
        raise ValueError(f"{path} holds no LoRA adapters: drop --lora_r (or pass the checkpoint of a LoRA run)")
    diff = sorted(set(own) ^ set(got)) or sorted(k for k in own if own[k] != got[k])
    raise ValueError(f"{path}: its LoRA adapters do not match --lora_r {model.lora_cfg.r} / --lora_target_modules "
                     f"{','.join(model.lora_cfg.targets)} (first difference: {diff[0]})")


def merge_dumps(parts):
    """One dump of the ranks' dumps, in rank order: a top-level value that is a dict is a per-image-id sub-dump (--select / --num_modes /
    --soft_decode / --full_metrics) and is merged with the other ranks' of its key; anything else is a trajectory entry.  Trajectories come
    first."""
    dump = {k: v for p in parts for k, v in p.items() if not isinstance(v, dict)}
    for p in parts:
        for key, sub in p.items():
            if isinstance(sub, dict):
                dump.setdefault(key, {}).update(sub)
    return dump


def evaluate(args, model, data, split="test", device="cuda"):
    """evaluate.py:70-170: load best_model_ade.pt, generate on the split, dump {split}_gen_trajs.json
    ({image_id: [[x,y,z,rx,ry,rz], ...]}, evaluate.py:150,167-170); --do_standard statistics come from
    `{checkpoint_dir}/norm_param.json` (evaluate.py:91 hands checkpoint_dir to the dataset as save_dir)."""
    best = os.path.join(args.checkpoint_dir, "best_model_ade.pt")
    if os.path.exists(best):
        sd = torch.load(best, map_location="cpu", weights_only=True)["model_state_dict"]
        check_adapter_keys(model, sd, best)
        model.load_state_dict(sd)
    norm = getattr(data, "norm", None)
    if norm is not None and norm.mode == "standard" and norm.mean is None:
        norm.load(args.checkpoint_dir)
    metrics, dump = run_validation(model, data, args, device, num_beams=int(getattr(args, "num_beams", 1)),
                                   num_samples=int(getattr(args, "num_samples", 1) or 1), select=getattr(args, "select", "none"))
    rank, world = _rank_world()
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, dump)
        dump = merge_dumps(parts)
    if rank == 0:
        with open(os.path.join(args.checkpoint_dir, f"{split}_gen_trajs.json"), "w") as f:
            json.dump(dump, f)
    return metrics


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="EgoScaler trajectory generator on MI355X (flags of train.py:312-347)")
    ap.add_argument("mode", choices=["train", "eval"])
    ap.add_argument("--model_name", default=None, help="local HF directory; omit for seeded synthetic weights")
    ap.add_argument("--max_traj_token", type=int, default=160)
    ap.add_argument("--max_desc_token", type=int, default=20)
    ap.add_argument("--num_steps", type=int, default=20)
    ap.add_argument("--do_norm", action="store_true")
    ap.add_argument("--do_standard", action="store_true")
    ap.add_argument("--unfreeze_pc_encoder", action="store_true")
    ap.add_argument("--unfreeze_language_model", action="store_true")
    ap.add_argument("--lora_r", type=int, default=0, help="LoRA adapters of this rank on the decoder projections (0: none); base weights stay frozen")
    ap.add_argument("--lora_alpha", type=float, default=16.0, help="LoRA scaling s = lora_alpha / lora_r")
    ap.add_argument("--lora_target_modules", default="q_proj,v_proj",
                    help="comma list of q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--grad_accum_steps", type=int, default=1)
    ap.add_argument("--lr_llm", type=float, default=2e-5)
    ap.add_argument("--max_grad_norm", type=float, default=0.0,
                    help="train: clip the global gradient norm of every optimizer step to this value on the device (HF Trainer's "
                         "max_grad_norm / DeepSpeed's gradient_clipping); 'inf' only measures it; adds grad_norm_mean / grad_norm_max / "
                         "clipped_steps / nonfinite_steps to the epoch record and grad_norm to the step log (0: off, the reference does not clip)")
    ap.add_argument("--bin_sigma", type=float, default=0.0,
                    help="train with the bin-aware loss: a target that is a bin token becomes a discrete Gaussian of this width (in bins, at most 16) "
                         "over the neighbouring bins, renormalised at the ends of the bin range; train_loss is then the soft loss and the epoch "
                         "record gains train_nll (the reference's hard loss), bin_sigma and bin_radius, the step log nll (0: off, the reference's loss)")
    ap.add_argument("--bin_radius", type=int, default=None,
                    help="with --bin_sigma: cut the Gaussian this many bins from the target, 1 .. 32 (default min(32, ceil(3 * bin_sigma)))")
    ap.add_argument("--num_bins", type=int, default=256)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))
    ap.add_argument("--out_dir", default="runs/egoscaler_amd")
    ap.add_argument("--checkpoint_dir", default=None)
    ap.add_argument("--tiny", action="store_true", help="small synthetic model (smoke runs)")
    ap.add_argument("--n_train", type=int, default=64)
    ap.add_argument("--n_val", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--val_greedy", dest="val_sample", action="store_false",
                    help="validate with greedy decoding instead of the reference's sampling defaults (model_arch.py:82-88)")
    ap.add_argument("--num_beams", type=int, default=1,
                    help="eval mode: beam search with N beams (beam sampling unless --val_greedy); the dump keeps the best hypothesis per image")
    ap.add_argument("--kv_cache_layout", default="dense", choices=["dense", "split"],
                    help="KV cache of beam search (--num_beams > 1) in validation / eval: one full-length row per beam (dense), or one "
                         "prompt row per clip plus one suffix row per beam (split)")
    ap.add_argument("--num_samples", type=int, default=1,
                    help="validation / eval: K sampled trajectories per clip from one prefill and one cached prompt per clip; adds best-of-K "
                         "minADE / minFDE to the record and keeps all K in the dump (not with --val_greedy or --num_beams > 1)")
    ap.add_argument("--select", default="none", choices=["none", "logprob", "medoid"],
                    help="validation / eval with --num_samples K > 1: also pick one of the K without the ground truth, on the device (logprob: "
                         "highest mean token log-prob under the raw logits; medoid: smallest mean ADE to the other samples); adds ADE_sel / "
                         "FDE_sel to the record and the picked index per image id to the dump")
    ap.add_argument("--kv_cache_dtype", default="auto", choices=["auto", "fp8"],
                    help="KV cache of every generate() call in validation / eval: the model's dtype (auto) or e4m3fn codes with per-(token, head) scales")
    ap.add_argument("--decode_weight_dtype", default="auto", choices=["auto", "fp8", "int4"],
                    help="weights of the decode-step projections of every generate() call in validation / eval: the model's (auto), "
                         "e4m3fn codes with per-output-row scales (fp8) or 4-bit codes with per-row scales over 128-column groups (int4); "
                         "bf16 models, prefill stays bf16")
    ap.add_argument("--root_dir", default=None, help="EgoScaler data root (pcrgbs/, trajs/ ...: dataset.py:36, dataset_base.py:68-103)")
    ap.add_argument("--data_dir", default=None, help="directory of the split files {train,val,test}.json (dataset.py:37)")
    ap.add_argument("--smooth_traj", action="store_true", help="smoothing_traj on the resampled tracks (dataset.py:39 reads this attribute)")
    ap.add_argument("--split", default="test", help="eval mode: the split to generate for (evaluate.py:89-100 uses 'test')")
    ap.add_argument("--rescore", action="store_true",
                    help="validation / eval with --num_samples K > 1 --select logprob: rank the K samples by model.score() (teacher-forced "
                         "log-probs on the model's own weights, one suffix pass on the shared prompt) instead of the sampling run's own "
                         "log-probs, which are those of the quantized decoder under --decode_weight_dtype fp8 / int4")
    ap.add_argument("--num_modes", type=int, default=0,
                    help="validation / eval with --num_samples K > 1: also pick M <= K mutually different samples per clip, each with a "
                         "probability, on the device (ordered by the --select logprob scores when given, else by centrality); adds minADE_M / "
                         "minFDE_M / brierADE_M / n_modes to the record and the indices and probabilities per image id to the dump (0: off)")
    ap.add_argument("--mode_radius", type=float, default=0.0,
                    help="with --num_modes: a sample within this distance (mean displacement over all 6 dimensions, units of the de-normalised "
                         "trajectories) of an earlier mode is not a mode of its own; 0 suppresses exact duplicates only")
    ap.add_argument("--soft_decode", action="store_true",
                    help="validation / eval with --num_beams 1: also decode sample 0 of every clip softly, every coordinate as the mean over the "
                         "bins of the distribution its token was drawn from; adds ADE_soft / FDE_soft / n_soft, sigma_mean (mean std of x, y, z) "
                         "and bin_mass_min to the record and the soft trajectory with its std per image id to the dump")
    ap.add_argument("--full_metrics", action="store_true",
                    help="validation / eval, every decoding mode: all five measures of the reference's metric module (ADE, FDE, IDE, GD, DTW) "
                         "for every sample on the device, one launch per batch; adds IDE / DTW / GD_dev / n_full (with --num_samples K > 1 "
                         "minIDE / minGD / minDTW, with --select GD_sel / DTW_sel, with --num_modes minGD_M / minDTW_M) to the record and the "
                         "per-sample values per image id to the dump")
    ap.add_argument("--constrain_traj", action="store_true",
                    help="validation / eval with --num_beams 1: constrained decoding, every generated row is a well-formed trajectory of exactly "
                         "--num_steps steps (the prompt's first step included), by one grammar launch per step on the device; adds "
                         "grammar_mass_mean / grammar_mass_min (the raw probability the model gave the allowed ids) to the record")
    ap.add_argument("--traj_workspace", default=None, metavar="x0,x1,y0,y1,z0,z1",
                    help="with --constrain_traj: every generated waypoint stays inside this box (units of the de-normalised trajectories; an "
                         "empty field = no bound; write --traj_workspace=-2,2,... when it starts with a minus sign), enforced on the device at "
                         "every bin token; adds n_limit_viol (must be 0) and limits_mass_min to the record")
    ap.add_argument("--traj_max_step", default=None, metavar="dx,dy,dz,rx,ry,rz",
                    help="with --constrain_traj: no waypoint moves farther than this from the one before it, per dimension (same units; an "
                         "empty field = no cap), the prompt's step included; record keys as --traj_workspace")
    a = ap.parse_args(argv)
    try:
        traj_limit_options(a, a.constrain_traj)
    except ValueError as e:
        ap.error(str(e))
    if not a.max_grad_norm >= 0:
        ap.error("--max_grad_norm must be >= 0 (0: off)")
    if not 0 <= a.bin_sigma <= 16:                                       # (refuses NaN and inf as well)
        ap.error("--bin_sigma must be a finite width in bins, 0 <= bin_sigma <= 16 (0: off)")
    if a.bin_radius is not None and not 1 <= a.bin_radius <= 32:
        ap.error("--bin_radius must be between 1 and 32")
    if a.bin_radius is not None and not a.bin_sigma > 0:
        ap.error("--bin_radius goes with --bin_sigma")
    try:
        check_val_options(int(a.num_samples or 1), a.num_beams, a.val_sample, a.select, a.rescore, a.num_modes, a.mode_radius, a.soft_decode,
                          decoding_rules=False, constrain=a.constrain_traj)
    except ValueError as e:
        ap.error(str(e))
    return a


DESC2TRAJ = {"desc": "Action description: {desc}"}                      # dataset.py:16-19


def make_data(a, dims, tokenizer, split, norm, n_synth, seed):
    """The split's data source: files when --root_dir/--data_dir are given (they need the tokenizer of --model_name), else synthetic."""
    if a.root_dir and a.data_dir:
        if tokenizer is None:
            raise ValueError("--root_dir/--data_dir need --model_name DIR (descriptions are tokenised with its tokenizer)")
        from .data_io import EgoScalerFiles, FileTrajData
        from .pointllm.constant import SEP_TOKEN
        encode = lambda text: tokenizer(DESC2TRAJ["desc"].format(desc=text), add_special_tokens=False).input_ids
        sep = tokenizer(SEP_TOKEN, add_special_tokens=False).input_ids              # dataset.py:54
        return FileTrajData(dims, EgoScalerFiles(a.root_dir, a.data_dir, split), encode, num_steps=a.num_steps, max_desc_token=a.max_desc_token,
                            smooth=a.smooth_traj, norm=norm, sep_ids=tuple(int(t) for t in sep))
    return SyntheticTrajData(dims, n_synth, num_steps=a.num_steps, seed=seed, norm=norm, max_desc_token=a.max_desc_token, ragged_text=True)


def main(argv=None):
    from .config import dims_7b, dims_tiny
    from .pointllm import TrajPointLLMForCausalLM
    a = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(a.local_rank)
    dev = torch.device("cuda", a.local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    tokenizer = None
    if a.model_name is not None:                                        # train.py:67 / evaluate.py:79: everything comes from the directory
        from .pointllm import build_model
        margs = types.SimpleNamespace(**{**vars(a), "dtype": dtype, "device": dev})
        model, tokenizer, _, _ = build_model(margs)
        dims = model.dims
    else:
        dims = dims_tiny() if a.tiny else dims_7b()
        model = TrajPointLLMForCausalLM(a, dims, None, device=dev, dtype=dtype)
        sd = synth.synth_state_dict(dims, 0)
        model.load_state_dict({k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()},
                              strict=model.lora_cfg is None)         # (fresh LoRA adapters keep their initialisation)
    a.checkpoint_dir = a.checkpoint_dir or a.out_dir
    norm = T.TargetNorm(a.do_norm, a.do_standard)
    if a.mode == "train":
        val = make_data(a, dims, tokenizer, "val", norm, a.n_val, 977)
        train(a, model, make_data(a, dims, tokenizer, "train", norm, a.n_train, 42), val, dev)
    else:
        print(json.dumps(evaluate(a, model, make_data(a, dims, tokenizer, a.split, norm, a.n_val, 977), a.split, dev)))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
