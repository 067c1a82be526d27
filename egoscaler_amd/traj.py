"""Trajectory (de)tokenisation, re-sampling, scaling and metrics.

Two layers, mirroring where the reference does this work:
  * batch-level integer work on the device (egomi_traj_tokenize / _detokenize / _metrics):
    what CustomDataset.__getitem__/collate_fn and detokenize_traj do per sample on the host
    (models/pointllm/dataset.py:150-194; the per-sample methods are missing from the release,
    SURVEY.md §0.1, so the contract is built from models/pointllm/utils/utils.py:13-104);
  * small host helpers with the reference's names and semantics for single trajectories / strings
    (utils.py, models/utils/traj_utils.py, models/utils/metrics.py), numpy like the reference.
Nothing here imports oracle/.
"""
import collections
import re

import numpy as np
import torch

from ._lib import call
from .ops import S

# Aria pin-hole camera and workspace constants (egoscaler/configs/camera.py:7-9, configs/dataset.py:1-7)
PINHOLE_IMAGE_SIZE = 1408
FOCAL_LEN = 605.343
PRINCIPAL_POINT = 703.5
WORKSPACE = {"min_x": -2.0, "max_x": 2.0, "min_y": -2.0, "max_y": 2.0, "min_z": 0.0, "max_z": 2.5}


# ------------------------------------------------------------------------------------------ device
def bin_edges(num_bins: int, device) -> torch.Tensor:
    return torch.from_numpy(np.linspace(-1, 1, num_bins)).to(device)            # float64, numpy's own values


def tokenize_batch(traj: torch.Tensor, tok, seq_len: int, steps=None):
    """traj f32 [B,T,6] in [-1,1] -> (ids i64 [B,seq_len], mask bool [B,seq_len]).
    Layout <ts> (p*6 <tsep>)*T <te> eos pad...; raises ValueError if seq_len is too short."""
    traj = traj.to(torch.float32).contiguous()
    B, T, _ = traj.shape
    dev = traj.device
    ids = torch.empty(B, seq_len, dtype=torch.int64, device=dev)
    mask = torch.empty(B, seq_len, dtype=torch.uint8, device=dev)
    err = torch.empty(B, dtype=torch.int32, device=dev)
    st = None if steps is None else torch.as_tensor(steps, dtype=torch.int32, device=dev).contiguous()
    call("egomi_traj_tokenize", traj, st, B, T, bin_edges(tok.num_bins, dev), tok.num_bins, tok.p0, tok.ts, tok.tsep, tok.te, tok.eos, tok.pad,
         seq_len, ids, mask, err, S())
    if int(err.max()) != 0:
        raise ValueError("trajectory tokens exceed max_traj_token")
    return ids, mask.bool()


def detokenize_batch(ids: torch.Tensor, tok, max_steps: int):
    """ids i64 [B,L] (generated span) -> (values f32 [B,max_steps,6] in [-1,1], n_steps i32 [B])."""
    ids = ids.to(torch.int64).contiguous()
    B, L = ids.shape
    dev = ids.device
    out = torch.zeros(B, max_steps, 6, dtype=torch.float32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    call("egomi_traj_detokenize", ids, B, L, bin_edges(tok.num_bins, dev), tok.num_bins, tok.p0, tok.tsep, tok.eos, max_steps, out, n, S())
    return out, n


GrammarSpec = collections.namedtuple("GrammarSpec", "p0 nb ts tsep te eos min_steps max_steps")


def grammar_spec(tok, min_steps: int, max_steps: int) -> GrammarSpec:
    """The trajectory grammar of generate(traj_grammar=...) for the tokenizer ids `tok` (the object tokenize_batch takes):
    <ts> (bin x 6 <tsep>) x n <te> eos with min_steps <= n <= max_steps, bins = the ids tok.p0 .. tok.p0 + tok.num_bins - 1.  n counts the
    steps from the sequence's last <ts>, the prompt's included: a prompt that already holds the first step needs min_steps >= 1 to mean
    anything.  The table itself is csrc/grammar.hip's."""
    mn, mx = int(min_steps), int(max_steps)
    if not 0 <= mn <= mx:
        raise ValueError(f"grammar_spec: 0 <= min_steps <= max_steps does not hold for ({min_steps}, {max_steps})")
    return GrammarSpec(int(tok.p0), int(tok.num_bins), int(tok.ts), int(tok.tsep), int(tok.te), int(tok.eos), mn, mx)


def motion_limits_bins(lo=None, hi=None, dmax=None, nb=256, rows=1):
    """The motion-limits table of generate(traj_limits=...) from limits already in bins: lo, hi, dmax are None (full range: 0, nb - 1, no
    cap = nb - 1), one integer, six of them (one per trajectory dimension x, y, z, rx, ry, rz) or [rows, 6] -> int32 [rows, 18] =
    lo | hi | dmax.  lo[d] <= bin <= hi[d] is the box, inclusive; dmax[d] the largest |bin_t[d] - bin_(t-1)[d]|.  Ranges are checked as
    decode.traj_limits_check checks them."""
    from .decode import traj_limits_check
    nb, rows = int(nb), int(rows)
    cols = []
    for v, full in ((lo, 0), (hi, nb - 1), (dmax, nb - 1)):
        a = np.full((rows, 6), full, dtype=np.int64) if v is None else np.asarray(v)
        if a.dtype.kind not in "iu":
            raise ValueError(f"motion_limits_bins: limits in bins are integers, not {a.dtype}")
        cols.append(np.broadcast_to(a.astype(np.int64), (rows, 6)))
    return traj_limits_check(np.concatenate(cols, axis=1), nb, rows)


def motion_limits(tok, norm, lo=None, hi=None, max_step=None, max_abs=None):
    """The motion-limits table of generate(traj_limits=...) from limits in the data's physical units (what TargetNorm.denorm returns:
    metres and rotation vectors): lo / hi [6] or [B, 6] = the box per dimension, max_step [6] or [B, 6] = the largest move per step and
    dimension, each None (or NaN / +-inf entries) for no limit; max_abs [B, 6] = the per-sample scale of `--do_standard` (None: one row
    with max_abs = 1).  -> int32 [B, 18] = lo | hi | dmax in bins, one row per sample.
    Bin i has the normalised value c_i = linspace(-1, 1, nb)[i] (bin_edges) and de-normalises through TargetNorm.denorm, which is affine per
    dimension: v -> offset + scale * c with scale = norm.denorm_scale(max_abs) > 0.  Rounding is conservative: lo rounds up to the first
    bin whose centre de-normalises >= lo, hi down to the last whose centre de-normalises <= hi, dmax down to the largest count of bins
    whose centres lie no farther apart than max_step -- each verified with denorm itself on the neighbouring bins, not trusted to the
    division.  A box that holds no bin centre raises ValueError."""
    nb = int(tok.num_bins)
    m = np.ones((1, 6)) if max_abs is None else np.asarray(max_abs, dtype=np.float64).reshape(-1, 6)
    B = m.shape[0]
    c = np.linspace(-1, 1, nb)
    phys = norm.denorm(np.broadcast_to(c[None, :, None], (B, nb, 6)), m)            # [B, nb, 6]: every bin centre de-normalised
    if bool((np.diff(phys, axis=1) <= 0).any()):
        raise ValueError("motion_limits: the de-normalisation must increase with the bin in every dimension (std and max_abs > 0)")

    def rows(v, fill):
        a = np.full((B, 6), fill) if v is None else np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (B, 6)))
        return np.where(np.isnan(a), fill, a)
    plo, phi, pst = rows(lo, -np.inf), rows(hi, np.inf), rows(max_step, np.inf)
    if bool((pst < 0).any()):
        raise ValueError("motion_limits: max_step is a distance, >= 0")
    blo = (phys < plo[:, None, :]).sum(1)                                           # the first bin with phys >= lo
    bhi = nb - 1 - (phys > phi[:, None, :]).sum(1)                                  # the last bin with phys <= hi
    if bool((blo > bhi).any()):
        raise ValueError("motion_limits: no bin centre de-normalises inside [lo, hi] in some dimension")
    dmax = np.zeros((B, 6), dtype=np.int64)
    for k in range(1, nb):                                                          # the largest k with every pair of centres k apart <= max_step
        ok = (phys[:, k:, :] - phys[:, :-k, :]).max(1) <= pst
        dmax = np.where(ok & (dmax == k - 1), k, dmax)
    from .decode import traj_limits_check
    return traj_limits_check(np.concatenate([blo, bhi, dmax], axis=1), nb, B)


def limits_window(lo, hi, dmax, q):
    """The one window rule of the motion limits (csrc/grammar.hip gr_window) on the host: the inclusive window (a, b) of bin indices for a
    dimension with limits (lo, hi, dmax) whose last closed step chose bin q (q < 0: unknown)."""
    if q < 0:
        return lo, hi
    a, b = max(lo, q - dmax), min(hi, q + dmax)
    if a > b:                                                                       # q lies farther than dmax outside the box: the cap wins
        a = b = min(max(lo if q < lo else hi, q - dmax), q + dmax)
    return a, b


def limits_violations(ids, tok, lim, start=0):
    """The validator of generate(traj_limits=...): ids [R, L] (whole sequences, prompt included: the last pose of the prompt limits the first
    generated step), lim [R, 18] -> int64 numpy [R], the number of bin tokens per row that lie outside their window.  It walks every row
    with the grammar's pose rule on the host in numpy: from the row's last <ts> (none: nothing is counted), a bin in a run of at most six
    after <ts> / <tsep> is dimension = its place in the run and is held against limits_window(lo, hi, dmax, prev[dimension]); <tsep> after
    six bins makes them prev, after fewer makes prev unknown; any other token ends the run.  Tokens after the first eos are not read.
    start: only bin tokens at columns >= start are counted (the prompt length: what the prompt holds was not the decoder's choice); the
    pose is followed from the row's beginning either way."""
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64)
    lim = np.asarray(lim.cpu() if isinstance(lim, torch.Tensor) else lim).astype(np.int64)
    if ids.ndim != 2 or lim.shape != (ids.shape[0], 18):
        raise ValueError(f"limits_violations: ids [R, L] and lim [R, 18], not {ids.shape} and {lim.shape}")
    p0, nb = int(tok.p0), int(tok.num_bins)
    out = np.zeros(ids.shape[0], dtype=np.int64)
    for r, row in enumerate(ids.tolist()):
        last = max((j for j, t in enumerate(row) if t == tok.ts), default=None)
        if last is None:
            continue
        prev, cur, run = [-1] * 6, [-1] * 6, 0
        for j, t in enumerate(row[last + 1:], last + 1):
            if t == tok.eos:
                break
            if p0 <= t < p0 + nb:
                if run < 6:
                    a, b = limits_window(int(lim[r, run]), int(lim[r, 6 + run]), int(lim[r, 12 + run]), prev[run])
                    out[r] += j >= start and not a <= t - p0 <= b
                    cur[run] = t - p0
                    run += 1
                continue
            if t == tok.tsep:
                prev = list(cur) if run == 6 else [-1] * 6
            run = 0
    return out


SoftTargetSpec = collections.namedtuple("SoftTargetSpec", "p0 nb sigma radius")


def soft_target_spec(tok, sigma: float, radius=None) -> SoftTargetSpec:
    """The bin-aware training target of loss_and_backward(bin_soft=...) for the tokenizer ids `tok`: a row whose target is one of the bin ids
    tok.p0 .. tok.p0 + tok.num_bins - 1 is scored against a discrete Gaussian of width `sigma` (in bins, 0 < sigma <= 16) around that bin,
    cut at `radius` bins (1 .. 32; default min(32, ceil(3 sigma))) and at the ends of the bin window and renormalised there; every other
    target keeps its one-hot (include/egomi.h, egomi_ce_soft_fwd_bwd)."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"soft_target_spec: sigma must be a number, not {sigma!r}") from None
    if not 0.0 < s <= 16.0:                                                          # (refuses NaN as well)
        raise ValueError(f"soft_target_spec: 0 < sigma <= 16 (bins) does not hold for {sigma!r}")
    if radius is None:
        w = min(32, int(np.ceil(3.0 * s)))
    else:
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
            raise ValueError(f"soft_target_spec: radius must be an integer, not {radius!r}")
        w = int(radius)
    if not 1 <= w <= 32:
        raise ValueError(f"soft_target_spec: 1 <= radius <= 32 does not hold for {radius!r}")
    return SoftTargetSpec(int(tok.p0), int(tok.num_bins), s, w)


def detokenize_soft(ids: torch.Tensor, tok, max_steps: int, bin_mean, bin_std, bin_mass=None):
    """detokenize_batch with the per-token statistics of generate(output_bin_stats=True) / egomi_bin_stats in place of the bin centres
    (egomi_traj_detokenize_soft): the same scan of the same ids, and a step parsed from ids hit .. hit+5 takes
    mean[b, n, c] = bin_mean[b, hit + c], std[b, n, c] = bin_std[b, hit + c], mass[b, n] = min over c of bin_mass[b, hit + c];
    a copied-forward step repeats all three.  -> (mean f32 [B,max_steps,6], std f32 [B,max_steps,6], mass f32 [B,max_steps] or None without
    bin_mass, n_steps i32 [B] = detokenize_batch's); steps >= n_steps are 0.
    ids i64 [B,L] and the statistics [B, >= L] share their column numbering: pass the GENERATED part only (out.sequences[:, S0:] beside
    out.bin_mean), or prepend the same number of columns to both."""
    ids = ids.to(torch.int64).contiguous()
    B, L = ids.shape
    dev = ids.device
    stats = [None if s is None else s.to(device=dev, dtype=torch.float32) for s in (bin_mean, bin_std, bin_mass)]
    for s in stats:
        if s is not None and (s.dim() != 2 or s.shape[0] != B or s.shape[1] < L):
            raise ValueError(f"the bin statistics must be [B, >= L] = [{B}, >= {L}] like ids, not {tuple(s.shape)}")
    bm, bsd, bms = (None if s is None else s[:, :L].contiguous() for s in stats)
    mean = torch.zeros(B, max_steps, 6, dtype=torch.float32, device=dev)
    std = torch.zeros(B, max_steps, 6, dtype=torch.float32, device=dev)
    mass = None if bms is None else torch.zeros(B, max_steps, dtype=torch.float32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    call("egomi_traj_detokenize_soft", ids, B, L, tok.num_bins, tok.p0, tok.tsep, tok.eos, bm, bsd, bms, L, max_steps, mean, std, mass, n, S())
    return mean, std, mass, n


def _lens(n, dev, shape=None):
    """A step-count argument as the kernels read it: None (every sample is full length), or int32, contiguous, on `dev`; of `shape`
    [B,K] where one is given.  A count beyond the buffer's T steps counts as T (csrc/traj_disp.h: traj_len)."""
    if n is None:
        return None
    if shape is not None and tuple(n.shape) != shape:
        raise ValueError("n_gen must be [B,K]")
    return n.to(device=dev, dtype=torch.int32).contiguous()


def metrics_batch(gen, n_gen, gt, n_gt=None):
    """ADE / FDE per sample (float64), generated trajectories padded with their last step or cut to
    the ground-truth length (models/utils/metrics.py:40-52)."""
    gen, gt = gen.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    B, T, D = gt.shape
    if gen.shape != gt.shape:
        raise ValueError("gen and gt must share [B,T,D]")
    dev = gt.device
    ade = torch.empty(B, dtype=torch.float64, device=dev)
    fde = torch.empty(B, dtype=torch.float64, device=dev)
    call("egomi_traj_metrics", gen, _lens(n_gen, dev), gt, _lens(n_gt, dev), B, T, D, ade, fde, S())
    return ade, fde


def metrics_best_of(gen, n_gen, gt, n_gt=None):
    """Best-of-K metrics per clip (float64, on the device): gen [B, K, T, D], n_gen [B, K] or None, gt [B, T, D], n_gt [B] or None ->
    (min_ade [B], min_fde [B], best [B] int32).  Every sample is scored as metrics_batch scores it; a sample with n_gen <= 0 (nothing
    parsed) takes no part.  best = arg-min of ADE over the others (lowest index on ties), -1 with NaN metrics when none is left;
    min_fde is the minimum FDE over the samples, not the FDE of `best`."""
    gen, gt = gen.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    B, T, D = gt.shape
    if gen.dim() != 4 or gen.shape[0] != B or tuple(gen.shape[2:]) != (T, D):
        raise ValueError("gen must be [B,K,T,D] for gt [B,T,D]")
    K = gen.shape[1]
    if K < 1:
        raise ValueError("gen holds no sample")
    dev = gt.device
    ng, nt = _lens(n_gen, dev, (B, K)), _lens(n_gt, dev)
    min_ade = torch.empty(B, dtype=torch.float64, device=dev)
    min_fde = torch.empty(B, dtype=torch.float64, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    call("egomi_traj_metrics_min", gen, ng, gt, nt, B, K, T, D, min_ade, min_fde, best, S())
    return min_ade, min_fde, best


FULL_METRICS = ("ADE", "FDE", "IDE", "GD", "DTW")                              # the columns of metrics_full's mins / args
FULL_MAX_STEPS = 256
FullMetrics = collections.namedtuple("FullMetrics", ("ade", "fde", "ide", "gd", "dtw", "mins", "args"))


def metrics_full(gen, n_gen, gt, n_gt=None, rot0=3):
    """All five measures of the reference's metric module per sample, on the device in one launch (egomi_traj_metrics_full):
    gen [B, K, T, D] (or [B, T, D] for K = 1), n_gen [B, K] ([B]) or None, gt [B, T, D], n_gt [B] or None, T <= 256 ->
    FullMetrics(ade, fde, ide, gd, dtw, mins, args): the first five float64 and shaped like gen's leading dimensions (views of the one
    [B, K, 5] result), mins float64 [B, 5] and args int32 [B, 5] the per-clip minimum of every column over the samples whose value is not
    NaN and that sample's index (lowest index on ties; NaN and -1 when there is none), columns in the order of FULL_METRICS.
    ade / fde are metrics_batch's, bit for bit, and mins[:, :2], args[:, 0] metrics_best_of's.  ide = ||gt[0] - gen[0]||; gd = the
    reference's angular distance on the rotation vectors in columns rot0 .. rot0 + 2 of the padded rows (NaN everywhere when they do not
    exist: rot0 = -1 with gen[..., :3]); dtw = dynamic_time_warping on gen[:n_gen] and gt[:n_gt], which sees no padding: pass the parsed
    step counts.  A sample with n_gen <= 0 (or a clip with n_gt <= 0) is NaN in all five."""
    gen, gt = gen.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    B, T, D = gt.shape
    single = gen.dim() == 3
    if single:
        gen = gen[:, None]
        n_gen = None if n_gen is None else n_gen.reshape(-1, 1)
    if gen.dim() != 4 or gen.shape[0] != B or tuple(gen.shape[2:]) != (T, D):
        raise ValueError("gen must be [B,K,T,D] for gt [B,T,D]")
    K = gen.shape[1]
    if K < 1:
        raise ValueError("gen holds no sample")
    dev = gt.device
    ng, nt = _lens(n_gen, dev, (B, K)), _lens(n_gt, dev)
    if T > FULL_MAX_STEPS:
        raise ValueError(f"metrics_full serves T <= {FULL_MAX_STEPS} steps, not {T}")
    out = torch.empty(B, K, len(FULL_METRICS), dtype=torch.float64, device=dev)
    mins = torch.empty(B, len(FULL_METRICS), dtype=torch.float64, device=dev)
    args = torch.empty(B, len(FULL_METRICS), dtype=torch.int32, device=dev)
    call("egomi_traj_metrics_full", gen, ng, gt, nt, B, K, T, D, int(rot0), out, mins, args, S())
    cols = out[:, 0] if single else out
    return FullMetrics(*(cols[..., m] for m in range(len(FULL_METRICS))), mins, args)


def select_medoid(gen, n_gen=None):
    """The most central of K samples per clip, on the device (egomi_traj_medoid): gen [B, K, T, D], n_gen [B, K] or None ->
    (pick [B] int32, cost [B, K] float64).  cost[b, j] = mean over the other parsed samples i of the mean displacement between samples j
    and i (each padded with its own last step, as metrics_batch pads); a sample with n_gen <= 0 takes no part (cost NaN); pick = arg-min
    of cost (lowest index on ties), -1 when no sample is left; a single parsed sample is picked at cost 0.  Needs neither the ground
    truth nor model scores, so it also serves trajectories that did not come from generate()."""
    gen = gen.to(torch.float32).contiguous()
    if gen.dim() != 4 or gen.shape[1] < 1:
        raise ValueError("gen must be [B,K,T,D] with K >= 1")
    B, K, Tn, D = gen.shape
    dev = gen.device
    ng = _lens(n_gen, dev, (B, K))
    cost = torch.empty(B, K, dtype=torch.float64, device=dev)
    pick = torch.empty(B, dtype=torch.int32, device=dev)
    call("egomi_traj_medoid", gen, ng, B, K, Tn, D, cost, pick, S())
    return pick, cost


def metrics_selected(gen, n_gen, gt, n_gt, pick):
    """ADE / FDE (float64 [B]) of the sample pick[b] of every clip: metrics_batch on the gathered rows gen[b, pick[b]] (bit-equal to it);
    pick[b] < 0 (nothing to pick) gives NaN.  gen [B, K, T, D], n_gen [B, K] or None, gt [B, T, D], n_gt [B] or None, pick [B]."""
    B, K = gen.shape[:2]
    pick = pick.to(gen.device).long()
    ok = pick >= 0
    idx = torch.arange(B, device=gen.device), pick.clamp(min=0)
    g = gen[idx]
    ng = None if n_gen is None else n_gen[idx]
    ade, fde = metrics_batch(g, ng, gt, n_gt)
    nan = torch.full_like(ade, float("nan"))
    return torch.where(ok, ade, nan), torch.where(ok, fde, nan)


def select_modes(gen, n_gen=None, scores=None, num_modes=6, radius=0.0, return_dist=False):
    """M mutually different of K samples per clip, each with a probability, on the device (egomi_traj_modes): gen [B, K, T, D] with K <= 64,
    n_gen [B, K] or None, scores [B, K] or None, 1 <= num_modes = M <= 64 -> (modes int32 [B, M], conf float64 [B, M], assign int32 [B, K],
    n_modes int32 [B], n_nms int32 [B]), and dist float64 [B, K, K] with return_dist.
    The distance between two samples is select_medoid's: the mean displacement with each sample padded by its own last step, over ALL D
    dimensions, as ADE runs everywhere in this package; for position-only modes pass gen[..., :3].  A sample with n_gen <= 0 takes no part.
    Order: descending scores (seq_rank's rules: ties to the lower index, NaN as -inf), or with scores=None ascending select_medoid cost.
    A sample of the order becomes a mode when it is farther than `radius` from every mode picked before it (n_nms of them); free slots are
    then filled with the sample farthest from the picked modes while that distance is > 0 (n_modes in all; modes[b, n_modes:] = -1).
    assign = slot of the nearest mode (-1 for an unparsed sample), conf[b, m] = share of the clip's parsed samples assigned to slot m."""
    gen = gen.to(torch.float32).contiguous()
    if gen.dim() != 4 or gen.shape[1] < 1:
        raise ValueError("gen must be [B,K,T,D] with K >= 1")
    B, K, Tn, D = gen.shape
    M = int(num_modes)
    if K > 64:
        raise ValueError(f"select_modes serves K <= 64 samples per clip, not {K}")
    if not 1 <= M <= 64:
        raise ValueError(f"num_modes must be in 1 .. 64, not {num_modes}")
    ng = _lens(n_gen, gen.device, (B, K))
    if scores is not None and tuple(scores.shape) != (B, K):
        raise ValueError("scores must be [B,K]")
    radius = float(radius)
    if radius != radius or radius < 0:
        raise ValueError(f"radius must be a number >= 0, not {radius}")
    dev = gen.device
    modes = torch.empty(B, M, dtype=torch.int32, device=dev)
    conf = torch.empty(B, M, dtype=torch.float64, device=dev)
    assign = torch.empty(B, K, dtype=torch.int32, device=dev)
    n_modes = torch.empty(B, dtype=torch.int32, device=dev)
    n_nms = torch.empty(B, dtype=torch.int32, device=dev)
    dist = torch.empty(B, K, K, dtype=torch.float64, device=dev) if return_dist else None
    sc = None if scores is None else scores.to(device=dev, dtype=torch.float32).contiguous()
    call("egomi_traj_modes", gen, ng, sc, B, K, Tn, D, M, radius, dist, modes, conf, assign, n_modes, n_nms, S())
    out = (modes, conf, assign, n_modes, n_nms)
    return out + (dist,) if return_dist else out


def metrics_modes(gen, n_gen, gt, n_gt, modes, conf):
    """Metrics of the chosen set: metrics_best_of on the gathered rows gen[b, modes[b, m]] (bit-equal to it; an unused slot, modes < 0,
    takes no part: its n_gen is forced to 0) -> (min_ade [B], min_fde [B], best_slot int32 [B], brier_ade [B]), float64.
    brier_ade = min_ade + (1 - conf[b, best_slot]) ** 2; NaN with best_slot -1 when nothing is left.
    gen [B, K, T, D], n_gen [B, K] or None, gt [B, T, D], n_gt [B] or None, modes [B, M] int32, conf [B, M] float64."""
    B, K, Tn = gen.shape[:3]
    modes = modes.to(gen.device).long()
    used = modes >= 0
    rows = torch.arange(B, device=gen.device)[:, None], modes.clamp(min=0)
    ng = torch.full((B, K), Tn, dtype=torch.int32, device=gen.device) if n_gen is None else n_gen.to(gen.device).to(torch.int32)
    min_ade, min_fde, slot = metrics_best_of(gen[rows], torch.where(used, ng[rows], torch.zeros_like(ng[rows])), gt, n_gt)
    c = conf.to(gen.device).to(torch.float64).gather(1, slot.long().clamp(min=0)[:, None])[:, 0]
    brier = torch.where(slot >= 0, min_ade + (1.0 - c) ** 2, torch.full_like(min_ade, float("nan")))
    return min_ade, min_fde, slot, brier


# ------------------------------------------------------------------------------------------ host
def discretize_action(action_vector, num_bins=256):
    """utils/utils.py:13-16."""
    return (np.digitize(action_vector, np.linspace(-1, 1, num_bins)) - 1).tolist()


def token_to_action(tokens, num_bins=256):
    """utils/utils.py:18-21."""
    bins = np.linspace(-1, 1, num_bins)
    return [bins[v] for v in tokens]


def rt2_scaler(traj: np.ndarray, maxmin, split=None) -> np.ndarray:
    """utils/utils.py:23-34: rot*pi, z -> [d_min,d_max], xy pixel -> metric through the Aria intrinsics."""
    d_max, d_min = maxmin
    traj[:, [3, 4, 5]] = np.pi * traj[:, [3, 4, 5]]
    traj[:, 2] = (1.0 / 2) * traj[:, 2] + (1.0 / 2)
    traj[:, 2] = (d_max - d_min) * traj[:, 2] + d_min
    for c in (0, 1):
        traj[:, c] = (PINHOLE_IMAGE_SIZE / 2) * traj[:, c] + (PINHOLE_IMAGE_SIZE / 2)
        traj[:, c] = (traj[:, c] - PRINCIPAL_POINT) * traj[:, 2] / FOCAL_LEN
    return traj


def simple_scaler(traj: np.ndarray, maxmin) -> np.ndarray:
    """utils/utils.py:36-45: the <x..><y..><z..><rx..><ry..><rz..> format — rotations in percent of a turn, depth in percent of the
    [d_min, d_max] range, x / y already in pixels."""
    d_max, d_min = maxmin
    traj[:, [3, 4, 5]] = np.pi * (2 * (traj[:, [3, 4, 5]] / 100) - 1)
    traj[:, 2] = traj[:, 2] / 100
    traj[:, 2] = traj[:, 2] * (d_max - d_min) + d_min
    traj[:, 0] = (traj[:, 0] - PRINCIPAL_POINT) * traj[:, 2] / FOCAL_LEN
    traj[:, 1] = (traj[:, 1] - PRINCIPAL_POINT) * traj[:, 2] / FOCAL_LEN
    return traj


_PATTERNS = {                                                                  # utils/utils.py:49-61
    (True, "pos"): re.compile(r"<p(\d+)> <p(\d+)> <p(\d+)>"),
    (True, "xy"): re.compile(r"<p(\d+)> <p(\d+)>"),
    (True, "full"): re.compile(r"<p(\d+)> <p(\d+)> <p(\d+)> <p(\d+)> <p(\d+)> <p(\d+)>"),
    (False, "pos"): re.compile(r"<x(\d+)><y(\d+)><z(\d+)>"),
    (False, "full"): re.compile(r"<x(\d+)><y(\d+)><z(\d+)><rx(\d+)><ry(\d+)><rz(\d+)>"),
}


def str_to_float(s, maxmin, split=None, rt2=False, only_pos=False, only_xy=False, z_values=None, num_bins=256):
    """utils/utils.py:47-104, every format: `rt2` (<p*> bins; 6-DoF, `only_pos` = 3 bins with rotations at bin 0, `only_xy` = 2 bins with
    the depth taken from `z_values[i]`, the last one repeated) or the per-axis <x..><y..> form (`only_pos`: 3 integers; `only_xy` is ignored
    there, as in the reference).  One match per `<tsep>` segment, a segment without one repeats the previous step (only once one exists,
    :88-90); float32 array through rt2_scaler / simple_scaler, None when nothing parsed.  (The reference's default is rt2=False; the
    trajectory generator's drivers pass rt2=True.)"""
    kind = "pos" if only_pos else ("xy" if (only_xy and rt2) else "full")
    pattern = _PATTERNS[(bool(rt2), kind)]
    traj, last = [], None
    for i, seg in enumerate(s.split("<tsep>")):
        m = pattern.search(seg)
        if m:
            if rt2:
                g = [int(v) for v in m.groups()]
                x, y, z, rx, ry, rz = token_to_action(g + [0] * (6 - len(g)), num_bins=num_bins)
                if kind == "xy":
                    z = z_values[i] if i < len(z_values) else z_values[-1]
            elif only_pos:
                x, y, z = map(int, m.groups())
                rx, ry, rz = 0, 0, 0
            else:
                x, y, z, rx, ry, rz = map(float, m.groups())
            last = (x, y, z, rx, ry, rz)
            traj.append(last)
        elif last is not None:
            traj.append(last)
    if not traj:
        return None
    traj = np.array(traj).astype(np.float32)
    return rt2_scaler(traj, maxmin, split) if rt2 else simple_scaler(traj, maxmin)


def denorm(traj: np.ndarray) -> np.ndarray:
    """dataset.py:139-145 (do_norm): [-1,1] -> workspace metres, rotations * pi.  traj [B,T,6]."""
    t = np.array(traj, copy=True)
    t[:, :, [0, 1, 2]] = (t[:, :, [0, 1, 2]] + 1) / 2
    for c, k in enumerate("xyz"):
        t[:, :, c] = t[:, :, c] * (WORKSPACE["max_" + k] - WORKSPACE["min_" + k]) + WORKSPACE["min_" + k]
    t[:, :, [3, 4, 5]] *= np.pi
    return t


def preprocess_traj(traj: np.ndarray, num_steps: int, return_padding_mask: bool = False):
    """models/utils/traj_utils.py:3-39."""
    T = traj.shape[0]
    if T >= num_steps:
        out, pm = traj[np.linspace(0, T - 1, num_steps).astype(int)], np.ones(num_steps, dtype=int)
    else:
        out = np.vstack([traj, np.tile(traj[-1], (num_steps - T, 1))])
        pm = np.concatenate([np.ones(T, dtype=int), np.zeros(num_steps - T, dtype=int)])
    return (out, pm) if return_padding_mask else out


def smoothing_traj(traj: np.ndarray) -> np.ndarray:
    """models/utils/traj_utils.py:41-96 (5-tap box filter on xyz with the reference's edge rules)."""
    p, n, out = traj[:, :3], traj.shape[0], []
    for j in range(n):
        if j == 0:
            m = (3 * p[0] + p[1] + p[2]) / 5 if n >= 3 else ((3 * p[0] + p[1]) / 4 if n == 2 else p[0])
        elif j == 1:
            m = (2 * p[0] + p[1] + p[2] + p[3]) / 5 if n >= 4 else ((2 * p[0] + p[1] + p[2]) / 4 if n == 3 else p[1])
        elif j == n - 2:
            m = (p[j - 2] + p[j - 1] + p[j] + p[j + 1]) / 4 if n >= 4 else ((p[j - 1] + p[j] + p[j + 1]) / 3 if n == 3 else p[j])
        elif j == n - 1:
            m = (p[j - 2] + p[j - 1] + p[j]) / 3 if n >= 3 else ((p[j - 1] + p[j]) / 2 if n == 2 else p[j])
        else:
            m = (p[j - 2] + p[j - 1] + p[j] + p[j + 1] + p[j + 2]) / 5
        out.append(m)
    return np.concatenate([np.array(out), traj[:, 3:]], axis=-1)


def _pad_like(gen, gt):
    if gen.shape[0] > gt.shape[0]:
        return gen[:gt.shape[0]]
    if gen.shape[0] < gt.shape[0]:
        return np.vstack([gen, np.repeat(gen[-1].reshape(1, -1), gt.shape[0] - gen.shape[0], axis=0)])
    return gen


def average_displacement_error(gen_traj, gt_traj) -> float:
    """models/utils/metrics.py:38-55 (axis=1 norm, as written; hand it [T,D], or [1,T,D] to get the
    value the reference drivers actually log)."""
    return np.linalg.norm(gt_traj - _pad_like(gen_traj, gt_traj), ord=2, axis=1).mean()


def final_displacement_error(gen_traj, gt_traj) -> float:
    """models/utils/metrics.py:7-27."""
    return np.linalg.norm(gt_traj[-1] - _pad_like(gen_traj, gt_traj)[-1], ord=2)


def initial_displacement_error(gen_traj, gt_traj) -> float:
    """models/utils/metrics.py:29-36."""
    return np.linalg.norm(gt_traj[0] - gen_traj[0], ord=2)


def dynamic_time_warping(gen_traj, gt_traj) -> float:
    """models/utils/metrics.py:57-59 as the exact dynamic programme, float64: gen_traj [n, D] and gt_traj [m, D] as they are (no padding,
    no cut), local cost c(i, k) = ||gen_i - gt_k||_2 over all D dims, Dp(i, k) = c(i, k) + min(Dp(i-1, k), Dp(i, k-1), Dp(i-1, k-1)),
    Dp(0, 0) = c(0, 0); the value is Dp(n-1, m-1), not normalised by the path length.
    Relation to the reference, which calls fastdtw(gen, gt, dist=euclidean)[0] at its default radius=1: fastdtw is exact when either
    sequence has fewer than radius + 2 = 3 steps (it then runs this very programme); on longer sequences it searches a window of the same
    table, so its value is an upper bound of this one.  fastdtw is not installed beside this package: how far the two lie apart on longer
    sequences is NOT measured."""
    x, y = np.asarray(gen_traj, dtype=np.float64), np.asarray(gt_traj, dtype=np.float64)
    n, m = len(x), len(y)
    cost = np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))
    dp = np.full((n, m), np.inf)
    for i in range(n):
        for k in range(m):
            if i == 0 and k == 0:
                dp[i, k] = cost[i, k]
                continue
            best = min(dp[i - 1, k] if i else np.inf, dp[i, k - 1] if k else np.inf, dp[i - 1, k - 1] if i and k else np.inf)
            dp[i, k] = cost[i, k] + best
    return float(dp[n - 1, m - 1])


def anglar_distance(gen_rot, gt_rot) -> float:
    """models/utils/metrics.py:61-87 (name as in the reference): mean 2*acos(|<q1,q2>| clipped) over steps."""
    from scipy.spatial.transform import Rotation as R
    g = _pad_like(gen_rot, gt_rot)
    ad = []
    for a, b in zip(g, gt_rot):
        d = np.dot(R.from_rotvec(a).as_quat(), R.from_rotvec(b).as_quat())
        ad.append(2 * np.arccos(np.clip(d, -1.0, 1.0)))
    return sum(ad) / len(ad)


class TargetNorm:
    """Target normalisation of CustomDataset (models/pointllm/dataset.py:41-148): `--do_norm` (workspace bounds,
    rotations / pi) or `--do_standard` (dataset mean / std, then a per-sample max-abs scale so values land in [-1, 1]),
    with the statistics side file `norm_param.json` {"mean", "std"} (dataset.py:104-124).

    `denorm` is the reference's (dataset.py:126-148).  The forward direction lives in the reference's missing
    `__getitem__`; it is restated here as the exact inverse of `denorm`:
      do_norm     : x,y,z -> 2*(v - min)/(max - min) - 1 ; rotvec -> r / pi ;            max_abs = 1
      do_standard : z = (v - mean) / std ; max_abs[d] = max_t |z[t,d]| ; v_norm = z / max_abs
    mode "none" (neither flag; the reference's denorm then returns None): values are taken as already normalised."""

    def __init__(self, do_norm=False, do_standard=False, mean=None, std=None):
        assert not (do_norm and do_standard), "Cannot enable both normalization methods."            # dataset.py:44
        self.mode = "norm" if do_norm else ("standard" if do_standard else "none")
        self.mean = None if mean is None else np.asarray(mean, dtype=np.float64)
        self.std = None if std is None else np.asarray(std, dtype=np.float64)

    # -- statistics (dataset.py:80-124)
    def fit(self, trajs, num_steps, smooth=False):
        """compute_mean_std (dataset.py:80-102): every trajectory resampled to num_steps (optionally smoothed), mean and
        std over (sample, step), std + 1e-8."""
        allt = []
        for t in trajs:
            t = preprocess_traj(np.asarray(t), num_steps)
            if smooth:
                t = smoothing_traj(t)
            allt.append(t)
        allt = np.array(allt)
        self.mean, self.std = allt.mean(axis=(0, 1)), allt.std(axis=(0, 1)) + 1e-8
        return self.mean, self.std

    def save(self, save_dir):
        import json
        import os
        with open(os.path.join(save_dir, "norm_param.json"), "w") as f:
            json.dump({"mean": self.mean.tolist(), "std": self.std.tolist()}, f)

    def load(self, save_dir):
        import json
        import os
        with open(os.path.join(save_dir, "norm_param.json")) as f:
            p = json.load(f)
        self.mean, self.std = np.array(p["mean"]), np.array(p["std"])
        return self

    # -- per sample
    def normalize(self, traj):
        """traj [T,6] (metres, rotation vectors) -> (values in [-1,1] [T,6] float64, max_abs [6])."""
        t = np.array(traj, dtype=np.float64, copy=True)
        if self.mode == "norm":
            for c, k in enumerate("xyz"):
                lo, hi = WORKSPACE["min_" + k], WORKSPACE["max_" + k]
                t[:, c] = 2.0 * (t[:, c] - lo) / (hi - lo) - 1.0
            t[:, 3:6] /= np.pi
            return t, np.ones(6)
        if self.mode == "standard":
            if self.mean is None:
                raise ValueError("do_standard needs statistics: fit() on the train split or load() norm_param.json")
            z = (t - self.mean) / self.std
            m = np.abs(z).max(axis=0)
            m = np.where(m > 0, m, 1.0)
            return z / m, m
        return t, np.ones(6)

    def denorm(self, traj, max_abs):
        """dataset.py:126-148.  traj [B,T,6] (numpy, copied), max_abs [B,6]."""
        t = np.array(traj, copy=True)
        if self.mode == "norm":
            return denorm(t)
        if self.mode == "standard":
            t = t * np.asarray(max_abs)[:, None, :]
            return t * self.std + self.mean
        return t

    def denorm_scale(self, max_abs):
        """|d denorm / d value| per sample and dimension, [B,6]: denorm is affine in every mode and every dimension (norm: v -> (v + 1) / 2 *
        (max - min) + min on x, y, z and v -> pi v on the rotations; standard: v -> v max_abs std + mean; none: the identity), so a
        standard deviation in normalised units becomes one in denorm's units by this factor."""
        m = np.asarray(max_abs, dtype=np.float64)
        if self.mode == "norm":
            f = [(WORKSPACE["max_" + k] - WORKSPACE["min_" + k]) / 2.0 for k in "xyz"] + [np.pi] * 3
            return np.broadcast_to(np.asarray(f), m.shape).copy()
        if self.mode == "standard":
            return np.abs(m * self.std)
        return np.ones_like(m)
