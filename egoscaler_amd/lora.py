"""LoRA adapters on the decoder projections: configuration, parameter names, initialisation and PEFT's on-disk format (host side).

Semantics are PEFT's lora.Linear (peft/tuners/lora/layer.py): y = x W^T + s (x A^T) B^T with s = lora_alpha / r, A [r, in], B [out, r],
A ~ kaiming_uniform_(a=sqrt(5)) = U(+-1/sqrt(in)), B = 0; no dropout, no adapter bias, no rsLoRA / DoRA.  The products run in
csrc/lora.hip (engine.Engine._lora_fwd / _lora_bwd); the base decoder weights stay frozen.
"""
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, Tuple

import torch

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
DEFAULT_TARGETS = ("q_proj", "v_proj")                 # PEFT's default for LLaMA
# adapters that share one input are computed together: (group, input, targets in the order of the stacked product's output columns)
GROUPS = (("qkv", ("q_proj", "k_proj", "v_proj")), ("o", ("o_proj",)), ("gu", ("gate_proj", "up_proj")), ("down", ("down_proj",)))
PEFT_PREFIX = "base_model.model."


def module_of(target):
    return ("self_attn." if target in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp.") + target


def base_name(l, target):
    return f"model.layers.{l}.{module_of(target)}.weight"


def adapter_names(l, target) -> Tuple[str, str]:
    p = f"model.layers.{l}.{module_of(target)}."
    return p + "lora_A.weight", p + "lora_B.weight"


def is_adapter(name):
    return ".lora_A." in name or ".lora_B." in name


@dataclass(frozen=True)
class LoraConfig:
    r: int
    alpha: float
    targets: Tuple[str, ...]

    @property
    def scale(self):
        return self.alpha / self.r

    def groups(self):
        """[(group, [targets of the group that are adapted])] for the groups with at least one adapter."""
        return [(g, [t for t in ts if t in self.targets]) for g, ts in GROUPS if any(t in self.targets for t in ts)]


def parse_targets(v):
    if v is None:
        return DEFAULT_TARGETS
    items = [s.strip() for s in v.split(",")] if isinstance(v, str) else [str(s).strip() for s in v]
    items = [s for s in items if s]
    if not items:
        raise ValueError("lora_target_modules is empty")
    bad = [s for s in items if s not in TARGETS]
    if bad:
        raise ValueError(f"unknown LoRA target module(s) {bad}: choose from {', '.join(TARGETS)} "
                         "(adapters on lm_head, the embeddings or the point backbone are not built)")
    return tuple(t for t in TARGETS if t in items)


def config_from_args(args, dtype=None):
    """LoraConfig from args.lora_r / lora_alpha / lora_target_modules, or None when lora_r is absent or 0.  Raises ValueError on what is
    not built."""
    r = getattr(args, "lora_r", None)
    if r is None or int(r) == 0:
        return None
    if int(r) != r or not (8 <= int(r) <= 64) or int(r) % 8:
        raise ValueError(f"lora_r must be a multiple of 8 in [8, 64] (or 0 for no adapters), not {r}")
    if getattr(args, "unfreeze_language_model", False):
        raise ValueError("lora_r > 0 together with unfreeze_language_model is not supported: LoRA trains adapters on a frozen LLM")
    if float(getattr(args, "lora_dropout", 0.0) or 0.0) != 0.0:
        raise ValueError("LoRA dropout > 0 is not built")
    alpha = getattr(args, "lora_alpha", None)
    alpha = 16.0 if alpha is None else float(alpha)
    if not alpha > 0:
        raise ValueError(f"lora_alpha must be > 0, not {alpha}")
    if dtype is not None and dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"LoRA needs a bf16 or fp32 model, not {dtype}")
    return LoraConfig(r=int(r), alpha=alpha, targets=parse_targets(getattr(args, "lora_target_modules", None)))


def init_A(shape, seed, l, target):
    """PEFT's kaiming_uniform_(a=sqrt(5)) = U(-1/sqrt(in), 1/sqrt(in)), drawn from a generator seeded by (seed, layer, target): every rank
    of a data-parallel job starts from the same adapters."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + l * 16 + TARGETS.index(target)) & 0x7FFFFFFFFFFFFFFF)
    bound = 1.0 / math.sqrt(shape[1])
    return torch.empty(shape, dtype=torch.float32).uniform_(-bound, bound, generator=g)


def adapter_config(cfg: LoraConfig, base_model_name_or_path=None):
    return {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": cfg.r, "lora_alpha": cfg.alpha, "target_modules": list(cfg.targets),
            "lora_dropout": 0.0, "bias": "none", "fan_in_fan_out": False, "use_rslora": False, "use_dora": False,
            "inference_mode": False, "base_model_name_or_path": base_model_name_or_path}


def save_dir(path, cfg: LoraConfig, tensors: Dict[str, torch.Tensor], base_model_name_or_path=None):
    """PEFT's save_pretrained layout: adapter_config.json + adapter_model.safetensors keyed base_model.model.<our name>."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(adapter_config(cfg, base_model_name_or_path), f, indent=2)
    save_file({PEFT_PREFIX + k: v.detach().cpu().contiguous() for k, v in tensors.items()}, os.path.join(path, "adapter_model.safetensors"))


def load_dir(path):
    """-> (LoraConfig, {our name: tensor}) from a PEFT adapter directory."""
    from safetensors.torch import load_file
    with open(os.path.join(path, "adapter_config.json")) as f:
        c = json.load(f)
    if c.get("peft_type", "LORA") != "LORA":
        raise ValueError(f"not a LoRA adapter: peft_type {c.get('peft_type')!r}")
    if float(c.get("lora_dropout", 0.0) or 0.0) != 0.0 or c.get("bias", "none") != "none" or c.get("use_dora") or c.get("use_rslora"):
        raise ValueError("adapter uses dropout, a bias, DoRA or rsLoRA: not built")
    cfg = LoraConfig(r=int(c["r"]), alpha=float(c["lora_alpha"]), targets=parse_targets(c["target_modules"]))
    sd = load_file(os.path.join(path, "adapter_model.safetensors"))
    out = {}
    for k, v in sd.items():
        if not k.startswith(PEFT_PREFIX):
            raise ValueError(f"unexpected key {k!r} in the adapter file")
        k = k[len(PEFT_PREFIX):]
        k = k.replace(".lora_A.default.weight", ".lora_A.weight").replace(".lora_B.default.weight", ".lora_B.weight")
        out[k] = v
    return cfg, out
