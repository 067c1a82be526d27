"""References for gradient-norm clipping (include/egomi.h, egomi_grad_sumsq / egomi_clip_scale / EgoAdamW(max_grad_norm=...)).

- a numpy float64 restatement: math.fsum of the float64 squares per segment (exactly rounded sums), then egomi_clip_scale's
  formulas written out;
- a torch-CPU arm: torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW.
Nothing here touches the GPU or the library."""
import math

import numpy as np
import torch


def f64(t):
    """A tensor's values (fp32 or bf16) as a flat float64 numpy array."""
    return t.detach().reshape(-1).to("cpu", torch.float64).numpy()


def seg_sumsq(t):
    x = f64(t)
    return math.fsum(x * x)                     # the squares of widened fp32 / bf16 values are exact in float64; fsum rounds once


def total_sumsq(segs):
    return math.fsum(segs)


def clip_scale(total, grad_scale, max_norm):
    """(total_norm fp32, coef fp32, scale_eff fp32) of egomi_clip_scale for a float64 total sum of squares."""
    gs = np.float32(grad_scale)
    with np.errstate(all="ignore"):
        norm = np.float64(gs) * np.sqrt(np.float64(total))
        coef = np.float64(np.float32(max_norm)) / (norm + np.float64(1e-6))
        if coef > 1.0:                           # a NaN stays a NaN
            coef = np.float64(1.0)
        eff = gs if coef >= 1.0 else np.float32(np.float64(gs) * coef)
        return np.float32(norm), np.float32(coef), np.float32(eff)


def stats_after(calls):
    """The stats block [steps, clipped, non-finite, sum of finite norms, max] after clip_scale calls (total, grad_scale, max_norm), from zero."""
    st = [0.0] * 5
    for total, gs, mx in calls:
        norm, coef, _ = clip_scale(total, gs, mx)
        st[0] += 1
        if np.isfinite(norm):
            st[1] += 1.0 if coef < 1.0 else 0.0
            st[3] += float(norm)
            st[4] = max(st[4], float(norm))
        else:
            st[2] += 1
    return st


def global_norm(grads, grad_scale):
    """grad_scale * sqrt(float64 sum of squares over all tensors)."""
    return float(np.float32(grad_scale)) * math.sqrt(total_sumsq([seg_sumsq(g) for g in grads]))


def torch_clip_adamw(params, grads_per_step, grad_scale, max_norm, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
    """The torch-CPU arm.  params {name: fp32 tensor}, grads_per_step [{name: tensor}] (unscaled, as the engine holds them):
    per step p.grad = g * grad_scale, clip_grad_norm_(max_norm), AdamW.step().  -> ({name: fp32 tensor}, [total norm per step])."""
    ps = {n: torch.nn.Parameter(p.detach().to("cpu", torch.float32).clone()) for n, p in params.items()}
    opt = torch.optim.AdamW(list(ps.values()), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    norms = []
    for grads in grads_per_step:
        for n, p in ps.items():
            p.grad = grads[n].detach().to("cpu", torch.float32).reshape(p.shape) * grad_scale
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(ps.values()), max_norm)))
        opt.step()
    return {n: p.detach() for n, p in ps.items()}, norms
