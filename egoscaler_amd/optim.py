"""AdamW over the engine's fp32 main_grad buffers (reference optimizer: train.py:107-117,
AdamW lr 2e-5 + linear warm-up over 1/5 of the steps; DeepSpeed keeps fp32 master weights for bf16
params, train.py:97-98 — same here, without ZeRO sharding: 288 GB holds everything replicated)."""
import torch

from . import ops


class EgoAdamW:
    def __init__(self, model, lr=2e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None):
        """max_grad_norm (None: no clipping, the step as it always was): a float clips the global gradient norm to it
        (torch.nn.utils.clip_grad_norm_ semantics), float("inf") only measures it.  See _clip."""
        self.model, self.lr, self.betas, self.eps, self.wd = model, lr, betas, eps, weight_decay
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"EgoAdamW: max_grad_norm must be > 0 (or None), got {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip_table = self._clip_names = self._clip_out = self._clip_stats = self._clip_scale = None
        self.t = 0
        self.state = {}
        for n, p in model.named_parameters():
            if p.requires_grad:
                master = p.data if p.dtype == torch.float32 else p.data.float()
                self.state[n] = {"p": p, "master": master, "m": torch.zeros_like(master), "v": torch.zeros_like(master)}

    def arm(self, grad_scale=1.0, lr=None):
        """Call right before the LAST backward pass of an optimizer step (one rank, the step about to follow with step(overlap=True) and the same
        grad_scale / lr): every decoder layer is then updated as soon as ITS gradients are final (Engine._notify_layer), on the side stream, under the
        backward pass of the layers below it — the update is HBM-bound and gets the chip whenever the compute stream runs something that leaves
        registers free (attention, norms, RoPE; the 8-phase GEMM does not), instead of queueing all 38 ms of it behind the backward pass.  step()
        then handles what is left (projector / point backbone, embedding, final norm, lm_head).  Values are the same as the plain step's.
        Returns False (and arms nothing) where that is not possible: an exchange is attached (gradients are not final until it has run), no CUDA
        device, or resident W^T copies of trainable weights that a later product of this backward could still read — or max_grad_norm is set:
        the global norm needs every gradient of the step, so no layer can be updated under the backward pass of the layers below it."""
        eng = self.model.engine
        self._armed = None
        eng.layer_final_hook = None
        if self.max_grad_norm is not None:
            return False
        if (eng.grad_sync is not None and not getattr(eng.grad_sync, "local", False)) or eng.device.type != "cuda" or not eng.any_layer_trainable:
            return False
        if any(nm in eng.trainable for nm in getattr(eng, "wT", {})):      # (EGOMI_GEMM_TN=0 route; before the first forward pass the hook looks again)
            return False
        groups = {}
        for n in self.state:
            groups.setdefault(eng.param_group_of(n), []).append(n)
        self._armed = {"lr": self.lr if lr is None else lr, "grad_scale": grad_scale, "done": set(), "groups": groups}
        eng.layer_final_hook = self._early_layer
        return True

    def _early_layer(self, l):
        a, eng = self._armed, self.model.engine
        names = a["groups"].get(l)
        if not names or any(nm in eng.trainable for nm in eng.wT):
            return
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream()
        self._side.wait_stream(torch.cuda.current_stream())       # the layer's gradients are final; every reader of its old weights has been queued
        with torch.cuda.stream(self._side):
            for n in names:
                self._update(n, self.state[n], eng, a["lr"], a["grad_scale"], t=self.t + 1)
            ev = torch.cuda.Event()
            ev.record(self._side)
            eng.param_events[l] = ev
        a["done"].add(l)

    def _update(self, n, st, eng, lr, grad_scale, t=None):
        g = eng.reduced_grad.get(n)                        # resident exchange (dp.GradSync(resident=True)): the rank-summed bf16 gradient, read
        if g is None:                                      # in place from the layer's wire buffer
            g = eng.main_grad.get(n)
        if g is None:
            return
        p = st["p"]
        copy = None if p.dtype == torch.float32 else p.data
        if self.max_grad_norm is not None:                 # clipping: the scale (grad_scale x coefficient) is on the device, _clip put it there
            ops.adamw(st["master"], copy, g, st["m"], st["v"], lr, self.betas[0], self.betas[1], self.eps, self.wd, self.t if t is None else t,
                      grad_scale_dev=self._clip_scale)
            return
        ops.adamw(st["master"], copy, g, st["m"], st["v"], lr, self.betas[0], self.betas[1], self.eps, self.wd, self.t if t is None else t, grad_scale)

    def _clip_prepare(self, eng):
        """The segment table over exactly the buffers _update will read (reduced_grad, else main_grad; entries without a gradient left out):
        device-resident, rebuilt only when an address, size or dtype changed.  False when no entry has a gradient: the step then updates
        nothing, as without clipping."""
        names, grads = [], []
        for n in self.state:
            g = eng.reduced_grad.get(n)
            if g is None:
                g = eng.main_grad.get(n)
            if g is not None:
                names.append(n)
                grads.append(g)
        if not grads:
            return False
        if self._clip_table is None or self._clip_table.key != ops.GradTable.key_of(grads):
            self._clip_table, self._clip_names = ops.GradTable(grads), names
        if self._clip_out is None:
            self._clip_out = torch.zeros(3, dtype=torch.float32, device=eng.device)
            self._clip_stats = torch.zeros(5, dtype=torch.float64, device=eng.device)
            self._clip_scale = self._clip_out[2:3]
        return True

    def _clip(self, grad_scale):
        """On the stream the updates run on, before the first of them: the float64 sum of squares of every gradient of the step (two
        launches), then total norm, coefficient and effective scale (one launch).  Nothing here waits for the device.  Under data
        parallelism this runs after the exchange, on the rank-summed values every rank holds bit-identically: every rank gets the same
        coefficient and no collective is added."""
        _, total = ops.grad_sumsq(self._clip_table)
        ops.clip_scale(total, grad_scale, self.max_grad_norm, self._clip_out, self._clip_stats)
        self._clip_event = torch.cuda.Event()
        self._clip_event.record()

    @property
    def last_grad_norm(self):
        """Device fp32 scalar: the global norm of the latest step's gradient as the update saw it (grad_scale folded in), before clipping.
        The current stream is made to wait for the kernel that wrote it (it may have run on the side stream); the host is not."""
        if self._clip_out is None:
            raise RuntimeError("EgoAdamW.last_grad_norm: no step with max_grad_norm set has run")
        torch.cuda.current_stream().wait_event(self._clip_event)
        return self._clip_out[0]

    def per_tensor_grad_norms(self):
        """name -> grad_scale * sqrt(sum of squares) of the latest step, for diagnostics.  Waits for the device."""
        if self._clip_table is None:
            raise RuntimeError("EgoAdamW.per_tensor_grad_norms: no step with max_grad_norm set has run")
        self.model.engine.wait_param_updates()
        seg = self._clip_table.seg_sumsq.cpu().tolist()
        return {n: self._last_grad_scale * s ** 0.5 for n, s in zip(self._clip_names, seg)}

    def grad_stats(self, reset=True):
        """{"steps", "clipped_steps", "nonfinite_steps", "grad_norm_mean", "grad_norm_max"} since the last reset.  Waits for the device."""
        if self.max_grad_norm is None:
            raise RuntimeError("EgoAdamW.grad_stats: max_grad_norm is not set")
        if self._clip_stats is None:
            return {"steps": 0, "clipped_steps": 0, "nonfinite_steps": 0, "grad_norm_mean": float("nan"), "grad_norm_max": 0.0}
        self.model.engine.wait_param_updates()
        steps, clipped, bad, total, peak = self._clip_stats.cpu().tolist()
        if reset:
            self._clip_stats.zero_()
        finite = steps - bad
        return {"steps": int(steps), "clipped_steps": int(clipped), "nonfinite_steps": int(bad),
                "grad_norm_mean": total / finite if finite else float("nan"), "grad_norm_max": peak}

    def step(self, grad_scale=1.0, lr=None, overlap=False):
        """overlap=True (training loops that go straight on to the next forward pass: bench.py, driver.train): the updates run on a side stream in
        the order the NEXT forward pass needs the tensors — projector / point backbone, embedding, decoder layers 0..L-1, final norm + lm_head — with
        one event per group, and the engine's forward waits for a group right before it first reads it (Engine.wait_params).  The pass is HBM-bound
        (30 B per parameter) and shares the CUs with the MFMA-bound forward products instead of running alone between two steps; values are the
        same.  Whoever reads parameters or optimizer state outside a forward pass calls engine.wait_param_updates() first (state_dict, generate,
        checkpoints and this class's own state accessors do)."""
        self.t += 1
        lr = self.lr if lr is None else lr
        eng = self.model.engine
        armed, self._armed = getattr(self, "_armed", None), None
        eng.layer_final_hook = None
        early = armed["done"] if armed is not None else set()       # decoder layers arm() has already updated under the backward pass
        if early and (armed["lr"] != lr or armed["grad_scale"] != grad_scale):
            raise RuntimeError("EgoAdamW.step: lr / grad_scale differ from the ones given to arm()")
        clip = self.max_grad_norm is not None and self._clip_prepare(eng)
        if clip:
            self._last_grad_scale = float(grad_scale)
        if not (overlap and eng.device.type == "cuda" and not any(nm in eng.trainable for nm in eng.wT)):
            eng.wait_param_updates()
            if clip:
                self._clip(grad_scale)
            for n, st in self.state.items():
                if eng.param_group_of(n) not in early:
                    self._update(n, st, eng, lr, grad_scale)
            eng.after_weights_update()
            return
        groups = {}
        for n in self.state:
            groups.setdefault(eng.param_group_of(n), []).append(n)
        L = eng.dims.lm.num_hidden_layers
        order = ["pre", "embed"] + list(range(L)) + ["post"]
        cur = torch.cuda.current_stream()
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream()
        self._side.wait_stream(cur)                        # gradients final (and exchanged); every reader of the old weights has been queued
        with torch.cuda.stream(self._side):
            if clip:
                self._clip(grad_scale)
            for key in order:
                names = groups.get(key)
                if not names or key in early:
                    continue
                for n in names:
                    self._update(n, self.state[n], eng, lr, grad_scale)
                ev = torch.cuda.Event()
                ev.record(self._side)
                eng.param_events[key] = ev
        eng.after_weights_update()

    def zero_grad(self):
        self.model.engine.zero_grad()
        for st in self.state.values():
            st["p"].grad = None

    def state_dict(self):
        self.model.engine.wait_param_updates()
        return {"t": self.t, "state": {n: {k: st[k] for k in ("master", "m", "v")} for n, st in self.state.items()}}

    def state_dict_cpu(self):
        self.model.engine.wait_param_updates()
        return {"t": self.t, "state": {n: {k: st[k].detach().cpu() for k in ("master", "m", "v")} for n, st in self.state.items()}}

    def resync_masters(self):
        """After loading a checkpoint: the low-precision model copies follow the fp32 masters again."""
        self.model.engine.wait_param_updates()
        for st in self.state.values():
            if st["p"].dtype != torch.float32:
                st["p"].data.copy_(st["master"])
        self.model.engine.after_weights_update()

    def load_state_dict(self, sd):
        self.model.engine.wait_param_updates()
        self.t = sd["t"]
        for n, s in sd["state"].items():
            for k in ("master", "m", "v"):
                self.state[n][k].copy_(s[k])


def linear_warmup_lr(base_lr, step, total_steps, warmup_steps=None):
    """HF `get_linear_schedule_with_warmup` as the reference sets it up (train.py:113-116): warm-up over
    int(total/5) steps starting from lr = 0 at step 0 (`step / warm`), then a linear decay that reaches 0 at
    `total_steps`.  `step` is the number of optimizer steps already taken (LambdaLR's epoch counter)."""
    warm = int(total_steps / 5) if warmup_steps is None else int(warmup_steps)
    if step < warm:
        return base_lr * float(step) / float(max(1, warm))
    return base_lr * max(0.0, float(total_steps - step) / float(max(1, total_steps - warm)))
