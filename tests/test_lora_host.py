"""CPU: LoRA configuration, initialisation and PEFT's on-disk format (egoscaler_amd/lora.py)."""
import json
import math
import types

import pytest
import torch

from egoscaler_amd import lora


def _args(**kw):
    return types.SimpleNamespace(**kw)


def test_off_when_absent_or_zero():
    assert lora.config_from_args(_args()) is None
    assert lora.config_from_args(_args(lora_r=0)) is None


def test_defaults_and_scale():
    c = lora.config_from_args(_args(lora_r=16))
    assert c.alpha == 16.0 and c.targets == ("q_proj", "v_proj") and c.scale == 1.0
    c = lora.config_from_args(_args(lora_r=8, lora_alpha=32, lora_target_modules="down_proj, q_proj"))
    assert c.scale == 4.0 and c.targets == ("q_proj", "down_proj")
    c = lora.config_from_args(_args(lora_r=64, lora_alpha=16, lora_target_modules=list(lora.TARGETS)))
    assert c.scale == 0.25 and c.targets == lora.TARGETS
    assert [g for g, _ in c.groups()] == ["qkv", "o", "gu", "down"]
    assert lora.config_from_args(_args(lora_r=16, lora_target_modules="v_proj,up_proj")).groups() == [("qkv", ["v_proj"]), ("gu", ["up_proj"])]


@pytest.mark.parametrize("r", [4, 12, 72, -8, 8.5])
def test_bad_rank(r):
    with pytest.raises(ValueError, match="multiple of 8"):
        lora.config_from_args(_args(lora_r=r))


def test_bad_configurations():
    with pytest.raises(ValueError, match="unknown LoRA target"):
        lora.config_from_args(_args(lora_r=8, lora_target_modules="q_proj,lm_head"))
    with pytest.raises(ValueError, match="empty"):
        lora.config_from_args(_args(lora_r=8, lora_target_modules=" , "))
    with pytest.raises(ValueError, match="unfreeze_language_model"):
        lora.config_from_args(_args(lora_r=8, unfreeze_language_model=True))
    with pytest.raises(ValueError, match="bf16 or fp32"):
        lora.config_from_args(_args(lora_r=8), dtype=torch.float16)
    with pytest.raises(ValueError, match="dropout"):
        lora.config_from_args(_args(lora_r=8, lora_dropout=0.1))
    with pytest.raises(ValueError, match="lora_alpha"):
        lora.config_from_args(_args(lora_r=8, lora_alpha=0))


def test_init_bounds_and_seeding():
    a = lora.init_A((16, 4096), 0, 3, "q_proj")
    b = 1 / math.sqrt(4096)
    assert float(a.abs().max()) <= b and float(a.abs().max()) > 0.9 * b
    assert abs(float(a.mean())) < 0.05 * b
    assert torch.equal(a, lora.init_A((16, 4096), 0, 3, "q_proj"))         # every rank draws the same adapters
    assert not torch.equal(a, lora.init_A((16, 4096), 0, 3, "v_proj"))
    assert not torch.equal(a, lora.init_A((16, 4096), 1, 3, "q_proj"))


def test_names():
    assert lora.adapter_names(5, "q_proj") == ("model.layers.5.self_attn.q_proj.lora_A.weight", "model.layers.5.self_attn.q_proj.lora_B.weight")
    assert lora.adapter_names(0, "gate_proj")[1] == "model.layers.0.mlp.gate_proj.lora_B.weight"
    assert lora.base_name(2, "down_proj") == "model.layers.2.mlp.down_proj.weight"
    assert lora.is_adapter("model.layers.0.mlp.up_proj.lora_A.weight") and not lora.is_adapter("model.layers.0.mlp.up_proj.weight")


def test_peft_format_round_trip(tmp_path):
    cfg = lora.LoraConfig(r=8, alpha=16.0, targets=("q_proj", "v_proj", "down_proj"))
    g = torch.Generator().manual_seed(0)
    t = {}
    for l in range(2):
        for tg, (n_out, n_in) in (("q_proj", (32, 32)), ("v_proj", (32, 32)), ("down_proj", (32, 64))):
            a, b = lora.adapter_names(l, tg)
            t[a] = torch.randn(8, n_in, generator=g)
            t[b] = torch.randn(n_out, 8, generator=g)
    lora.save_dir(str(tmp_path), cfg, t, "some/base")
    c = json.load(open(tmp_path / "adapter_config.json"))
    assert c["peft_type"] == "LORA" and c["task_type"] == "CAUSAL_LM" and c["r"] == 8 and c["lora_alpha"] == 16.0
    assert c["target_modules"] == ["q_proj", "v_proj", "down_proj"] and c["lora_dropout"] == 0.0 and c["bias"] == "none"
    from safetensors.torch import load_file
    raw = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert sorted(raw) == sorted("base_model.model." + k for k in t)
    assert "base_model.model.model.layers.1.mlp.down_proj.lora_A.weight" in raw
    assert tuple(raw["base_model.model.model.layers.1.mlp.down_proj.lora_A.weight"].shape) == (8, 64)
    cfg2, t2 = lora.load_dir(str(tmp_path))
    assert cfg2 == cfg and sorted(t2) == sorted(t)
    assert all(torch.equal(t[k], t2[k]) for k in t)


def test_load_rejects_unsupported(tmp_path):
    cfg = lora.LoraConfig(r=8, alpha=16.0, targets=("q_proj",))
    lora.save_dir(str(tmp_path), cfg, {lora.adapter_names(0, "q_proj")[0]: torch.zeros(8, 4)})
    c = json.load(open(tmp_path / "adapter_config.json"))
    c["use_dora"] = True
    json.dump(c, open(tmp_path / "adapter_config.json", "w"))
    with pytest.raises(ValueError, match="DoRA"):
        lora.load_dir(str(tmp_path))


def test_driver_flags():
    from egoscaler_amd import driver
    a = driver.parse_args(["train", "--lora_r", "16", "--lora_target_modules", "q_proj,k_proj"])
    assert a.lora_r == 16 and a.lora_alpha == 16.0 and lora.config_from_args(a).targets == ("q_proj", "k_proj")
    assert lora.config_from_args(driver.parse_args(["eval"])) is None
