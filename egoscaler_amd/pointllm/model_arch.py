"""TrajPointLLMForCausalLM on MI355X.

Mirrors egoscaler/models/pointllm/model_arch.py:8-124 (class, constructor arguments, freeze logic,
narrow forward, generate wrapper, train(mode) override) and the parts of
pointllm/model/pointllm.py it inherits (point_backbone_config :49-59,288-300; resize of the token
embeddings used by builder.py:44).  State-dict keys and shapes are the reference's,
so checkpoints round-trip.  All arithmetic runs in egoscaler_amd.engine on libegomi.so.
"""
import json
import os
import types
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from ..config import EgoDims, LlamaDims, PointBertDims, SpecialTokens
from ..engine import Engine
from .. import lora, ops, synth


class PointLLMConfig:
    """Duck-typed stand-in for the HF config the reference passes around (PointLLMConfig,
    pointllm.py:23-24): plain attributes, readable from / writable to a HF-style config.json."""
    model_type = "pointllm"

    def __init__(self, **kw):
        self.hidden_size = 4096
        self.intermediate_size = 11008
        self.num_hidden_layers = 32
        self.num_attention_heads = 32
        self.vocab_size = 32003
        self.rms_norm_eps = 1e-6
        self.rope_theta = 10000.0
        self.max_position_embeddings = 2048
        self.pad_token_id = 0
        self.bos_token_id = 1
        self.eos_token_id = 2
        self.point_backbone = "PointBERT"
        self.point_backbone_config_name = "PointTransformer_8192point_2layer"
        self.use_color = True
        self.mm_use_point_start_end = True
        self.DEFAULT_POINT_PATCH_TOKEN = "<point_patch>"
        self.DEFAULT_POINT_START_TOKEN = "<point_start>"
        self.DEFAULT_POINT_END_TOKEN = "<point_end>"
        self.point_bert = None            # optional dict overriding the PointBERT YAML values
        self.__dict__.update(kw)

    # PointBERT shapes by `point_backbone_config_name` (pointllm.py:38-41 resolves the name to a YAML next to its own sources; the numbers
    # of the two YAMLs the reference ships: pointbert/PointTransformer_8192point_2layer.yaml:1-16, PointTransformer_base_8192point.yaml:1-13)
    POINTBERT_BY_NAME = {
        "PointTransformer_8192point_2layer": dict(trans_dim=384, depth=12, num_heads=6, group_size=32, num_group=512, encoder_dims=256,
                                                  projection_hidden_dim=[1024, 2048], npoints=8192, drop_path_rate=0.1),
        "PointTransformer_base_8192point": dict(trans_dim=1152, depth=12, num_heads=12, group_size=48, num_group=512, encoder_dims=512,
                                                projection_hidden_dim=[], npoints=8192, drop_path_rate=0.1),
    }

    @classmethod
    def from_pretrained(cls, path, **overrides):
        """Reads the config.json of an HF directory — written by this class OR by the reference's own `save_pretrained` (HF PretrainedConfig:
        extra fields such as `architectures`, `dtype`, `transformers_version`, `head_dim`, `hidden_act` are kept as plain attributes;
        transformers >= 5 nests rope_theta under `rope_parameters`, 4.x wrote it at top level).  `point_backbone_config_name` selects the
        PointBERT shapes like the reference's YAML lookup (pointllm.py:38-41); a `<name>.yaml` inside the directory, or `point_bert=...`
        here / in the JSON, overrides the two names the reference ships."""
        with open(os.path.join(path, "config.json")) as f:
            kw = json.load(f)
        rp = kw.get("rope_parameters")
        if isinstance(rp, dict) and "rope_theta" in rp and "rope_theta" not in kw:
            kw["rope_theta"] = float(rp["rope_theta"])
            if rp.get("rope_type", "default") != "default":
                raise NotImplementedError(f"rope_type {rp.get('rope_type')!r}: only the default rotary embedding is built")
        if kw.get("rope_scaling"):
            raise NotImplementedError("rope_scaling is not built (the reference's checkpoints do not use it)")
        nkv = kw.get("num_key_value_heads")
        if nkv is not None and nkv != kw.get("num_attention_heads", nkv):
            raise NotImplementedError("grouped-query attention (num_key_value_heads != num_attention_heads) is not built")
        if kw.get("hidden_act", "silu") != "silu" or kw.get("attention_bias") or kw.get("mlp_bias") or kw.get("tie_word_embeddings"):
            raise NotImplementedError("config asks for a LLaMA variant this build does not have (hidden_act / biases / tied embeddings)")
        kw.update(overrides)
        cfg = cls(**kw)
        if cfg.point_bert is None:
            name = cfg.point_backbone_config_name
            yml = os.path.join(path, f"{name}.yaml")
            if os.path.exists(yml):
                import yaml
                with open(yml) as f:
                    y = yaml.safe_load(f)
                mdl = y.get("model", {})
                keys = ("trans_dim", "depth", "num_heads", "group_size", "num_group", "encoder_dims", "drop_path_rate")
                cfg.point_bert = {k: mdl[k] for k in keys if k in mdl}
                cfg.point_bert["projection_hidden_dim"] = list(mdl.get("projection_hidden_dim", [])) if mdl.get("projection_hidden_layer", 0) else []
                if "npoints" in y:
                    cfg.point_bert["npoints"] = y["npoints"]
            elif name in cls.POINTBERT_BY_NAME:
                cfg.point_bert = dict(cls.POINTBERT_BY_NAME[name])
            else:
                raise ValueError(f"unknown point_backbone_config_name {name!r}: put {name}.yaml into {path} or pass point_bert=dict(...)")
        return cfg

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump({k: v for k, v in self.__dict__.items()}, f, indent=1)

    @classmethod
    def from_dims(cls, dims: EgoDims):
        pb = dims.pb
        return cls(hidden_size=dims.lm.hidden_size, intermediate_size=dims.lm.intermediate_size,
                   num_hidden_layers=dims.lm.num_hidden_layers, num_attention_heads=dims.lm.num_attention_heads,
                   vocab_size=dims.lm.vocab_size, rms_norm_eps=dims.lm.rms_norm_eps, rope_theta=dims.lm.rope_theta,
                   max_position_embeddings=dims.lm.max_position_embeddings, pad_token_id=dims.tok.pad,
                   bos_token_id=dims.tok.bos, eos_token_id=dims.tok.eos,
                   point_bert=dict(trans_dim=pb.trans_dim, depth=pb.depth, num_heads=pb.num_heads, group_size=pb.group_size,
                                   num_group=pb.num_group, encoder_dims=pb.encoder_dims,
                                   projection_hidden_dim=list(pb.projection_hidden_dim), npoints=pb.npoints))

    def to_dims(self) -> EgoDims:
        pbk = dict(self.point_bert or {})
        pb = PointBertDims(point_dims=6 if self.use_color else 3, **pbk)
        lm = LlamaDims(hidden_size=self.hidden_size, intermediate_size=self.intermediate_size,
                       num_hidden_layers=self.num_hidden_layers, num_attention_heads=self.num_attention_heads,
                       vocab_size=self.vocab_size, rms_norm_eps=self.rms_norm_eps,
                       rope_theta=getattr(self, "rope_theta", 10000.0), max_position_embeddings=self.max_position_embeddings)
        return EgoDims(pb=pb, lm=lm, tok=SpecialTokens(pad=self.pad_token_id or 0, bos=self.bos_token_id, eos=self.eos_token_id))


@dataclass
class CausalLMOutput:
    """Same fields the reference reads from CausalLMOutputWithPast (train.py:174, evaluate.py)."""
    logits: torch.Tensor
    loss: Optional[torch.Tensor] = None
    past_key_values: Optional[object] = None
    hidden_states: Optional[object] = None
    attentions: Optional[object] = None

    def __getitem__(self, i):
        return (self.logits,)[i]


@dataclass
class GenerateOutput:
    sequences: torch.Tensor
    scores: Tuple[torch.Tensor, ...]
    # generate(output_logprobs=True) only (None otherwise)
    token_logprobs: Optional[torch.Tensor] = None       # fp32 [rows, T']: log-prob of every generated token under the raw logits, 0 after a row finished
    sequences_logprobs: Optional[torch.Tensor] = None   # fp32 [rows]: their sum per row
    sequences_lengths: Optional[torch.Tensor] = None    # int32 [rows]: tokens counted (the eos included, the pads after it not)
    sample_scores: Optional[torch.Tensor] = None        # num_return_sequences = K > 1: fp32 [B, K], sum / length ** rank_length_penalty
    rank: Optional[torch.Tensor] = None                 # int32 [B, K]: the clip's sample indices by descending sample_scores
    # generate(output_bin_stats=True) only: fp32 [rows, T'], column t = the raw distribution token t was drawn from, over the bin tokens; 0 after a row's eos
    bin_mass: Optional[torch.Tensor] = None             # probability that the token is a bin token at all
    bin_mean: Optional[torch.Tensor] = None             # E[value | bin token]
    bin_std: Optional[torch.Tensor] = None              # the standard deviation of that conditional distribution
    bin_entropy: Optional[torch.Tensor] = None          # its entropy in nats
    # generate(traj_grammar=spec) only: fp32 [rows, T'], column t = the raw probability of the ids the grammar allowed at step t; 0 after a row's eos
    grammar_mass: Optional[torch.Tensor] = None
    # generate(traj_limits=table) only: fp32 [rows, T'], column t = the raw probability of the ids allowed under the motion limits at step t; 0 after a row's eos
    limits_mass: Optional[torch.Tensor] = None


@dataclass
class GenerateBeamOutput:
    """HF GenerateBeamDecoderOnlyOutput's fields as generate(num_beams > 1, output_scores=True) fills them."""
    sequences: torch.Tensor
    sequences_scores: torch.Tensor
    scores: Tuple[torch.Tensor, ...]
    beam_indices: torch.Tensor


def _install(root: nn.Module, dotted: str, tensor: torch.Tensor, buffer: bool):
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if not hasattr(m, p):
            m.add_module(p, nn.Module())
        m = getattr(m, p)
    if buffer:
        m.register_buffer(parts[-1], tensor)
    else:
        m.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


_BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked")


class _LogitsFn(torch.autograd.Function):
    """Bridges the engine into torch.autograd so `loss.backward()` of the reference's training loop
    (train.py:176-183) drives the hand-written backward."""

    @staticmethod
    def forward(ctx, anchor, model, input_ids, attention_mask, point_clouds, fps_start, save):
        eng = model.engine
        hn = eng.forward_hidden(input_ids, attention_mask, point_clouds, fps_start, save=save)
        logits = eng.logits(hn)
        ctx.model, ctx.hn, ctx.saved = model, hn, save
        B, S = input_ids.shape
        return logits.view(B, S, -1)

    @staticmethod
    def backward(ctx, d_logits):
        model = ctx.model
        if not ctx.saved:
            raise RuntimeError("backward through a forward that ran without grad")
        eng = model.engine
        model._begin_backward()
        dl = d_logits.reshape(-1, d_logits.shape[-1])
        if dl.dtype != eng.dtype or not dl.is_contiguous():
            dl = dl.to(eng.dtype).contiguous()
        d_hn = eng.backward_logits(dl, ctx.hn)
        eng.backward_hidden(d_hn)
        model._publish_grads()
        return (torch.zeros_like(model._anchor), None, None, None, None, None, None)


def _fill_logprobs(out, dec, cols, rank, rank_length_penalty):
    """The log-prob fields of a GenerateOutput from the decoder's static buffers, as copies: token_logprobs [rows, cols], sequences_logprobs
    and sequences_lengths [rows]; rank = (B, K): also sample_scores and rank [B, K] (egomi_seq_rank); None: they stay None."""
    out.token_logprobs = dec.lp_tok[:, :cols].clone()
    out.sequences_logprobs, out.sequences_lengths = dec.lp_sum.clone(), dec.lp_n.clone()
    if rank is not None:
        from ..decode import seq_rank
        out.sample_scores, out.rank = seq_rank(out.sequences_logprobs, out.sequences_lengths, *rank, float(rank_length_penalty))


def _fill_bin_stats(out, dec, cols, past=None, shape=None):
    """The four bin_* fields of a GenerateOutput from the decoder's static buffers, as copies of their first `cols` columns: [rows, cols],
    zero where the bool mask `past` [rows, cols] is set; shape: reshaped to it."""
    for field, buf in (("bin_mass", dec.bs_mass), ("bin_mean", dec.bs_mean), ("bin_std", dec.bs_std), ("bin_entropy", dec.bs_ent)):
        t = buf[:, :cols].clone() if past is None else buf[:, :cols].masked_fill(past, 0.0)
        setattr(out, field, t if shape is None else t.reshape(shape))


class TrajPointLLMForCausalLM(nn.Module):
    def __init__(self, args, config, model_name: Optional[str] = None, device=None, dtype=torch.float32):
        super().__init__()
        self.args, self.config, self.model_name = args, config, model_name
        self.dims = config.to_dims() if not isinstance(config, EgoDims) else config
        dev = torch.device(device or "cuda")
        self.lora_cfg = lora.config_from_args(args, dtype)     # LoRA adapters on the decoder projections (None: off); validated before any allocation
        if dev.type != "cuda":
            raise RuntimeError("TrajPointLLMForCausalLM (egoscaler_amd) runs on an MI355X only; there is no CPU path")
        # q|k|v and gate|up of a decoder layer live side by side in ONE allocation each: every Parameter keeps its own name, shape and
        # contiguous rows (state_dict / load_state_dict / optimizers see the reference's tensors), and the engine reads [Wq;Wk;Wv] and
        # [Wgate;Wup] as stacked operands without holding copies that would have to follow each optimizer step
        shapes = dict(synth.param_shapes(self.dims))
        shared = {}
        for l in range(self.dims.lm.num_hidden_layers):
            for grp in (tuple(f"model.layers.{l}.self_attn.{n}_proj.weight" for n in "qkv"),
                        tuple(f"model.layers.{l}.mlp.{n}_proj.weight" for n in ("gate", "up"))):
                if all(g in shapes and len(shapes[g]) == 2 and shapes[g][1] == shapes[grp[0]][1] for g in grp):
                    block = torch.zeros(sum(shapes[g][0] for g in grp), shapes[grp[0]][1], dtype=dtype, device=dev)
                    r = 0
                    for g in grp:
                        shared[g] = block[r:r + shapes[g][0]]
                        r += shapes[g][0]
        for k, shape in synth.param_shapes(self.dims):
            leaf = k.rsplit(".", 1)[-1]
            is_buf = leaf in _BUFFER_LEAVES
            t = shared[k] if k in shared else torch.zeros(shape, dtype=torch.long if leaf == "num_batches_tracked" else dtype, device=dev)
            _install(self, k, t, is_buf)
        if self.lora_cfg is not None:
            self._install_lora(shapes, dtype, dev)
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        self.training_graph = True
        self.accumulate_grads = False
        self._tensors = None
        self.engine = None
        self.point_backbone_config = None
        self._build_engine()
        if model_name is not None and os.path.isdir(model_name):
            self.load_pretrained_weights()
        self._configure_trainable_parameters()

    # -- LoRA ------------------------------------------------------------------------------------------
    def _install_lora(self, shapes, dtype, dev):
        """PEFT lora.Linear adapters: lora_A.weight [r, in] ~ U(+-1/sqrt(in)) (kaiming_uniform_(a=sqrt(5))), lora_B.weight [out, r] = 0.  The
        A's of adapters that share an input (q|k|v, gate|up) lie back to back in one allocation: the engine reads them as one stacked operand."""
        cfg, seed = self.lora_cfg, int(getattr(self.args, "seed", 0) or 0)
        for l in range(self.dims.lm.num_hidden_layers):
            for _, targets in cfg.groups():
                n_in = shapes[lora.base_name(l, targets[0])][1]
                block = torch.empty(len(targets) * cfg.r, n_in, dtype=dtype, device=dev)
                for i, t in enumerate(targets):
                    a_name, b_name = lora.adapter_names(l, t)
                    A = block[i * cfg.r:(i + 1) * cfg.r]
                    A.copy_(lora.init_A(A.shape, seed, l, t))
                    _install(self, a_name, A, False)
                    _install(self, b_name, torch.zeros(shapes[lora.base_name(l, t)][0], cfg.r, dtype=dtype, device=dev), False)

    def lora_state_dict(self):
        """{name: tensor} of the adapters (empty without LoRA)."""
        self.engine.wait_param_updates()
        return {n: p.detach() for n, p in self.named_parameters() if lora.is_adapter(n)}

    def _adapters_changed(self):
        self.engine.lora_version += 1
        self.engine.w8 = self.engine.w4 = None

    def save_lora(self, path):
        """The adapters in PEFT's save_pretrained layout: adapter_config.json and adapter_model.safetensors (keys
        base_model.model.model.layers.{l}.<module>.lora_{A,B}.weight)."""
        if self.lora_cfg is None:
            raise ValueError("save_lora: the model has no LoRA adapters")
        lora.save_dir(path, self.lora_cfg, self.lora_state_dict(), self.model_name)

    def load_lora(self, path):
        """Adapters from a PEFT adapter directory; r, lora_alpha and target_modules must match this model's."""
        if self.lora_cfg is None:
            raise ValueError("load_lora: the model has no LoRA adapters (build it with lora_r > 0)")
        cfg, sd = lora.load_dir(path)
        if (cfg.r, cfg.alpha, cfg.targets) != (self.lora_cfg.r, self.lora_cfg.alpha, self.lora_cfg.targets):
            raise ValueError(f"adapter {path}: r={cfg.r}, lora_alpha={cfg.alpha}, targets={list(cfg.targets)} do not match the model's "
                             f"r={self.lora_cfg.r}, lora_alpha={self.lora_cfg.alpha}, targets={list(self.lora_cfg.targets)}")
        own = self.lora_state_dict()
        if set(sd) != set(own):
            raise ValueError(f"adapter {path}: keys differ from the model's (missing {sorted(set(own) - set(sd))[:4]}, "
                             f"unexpected {sorted(set(sd) - set(own))[:4]})")
        with torch.no_grad():
            for k, v in sd.items():
                own[k].copy_(v)
        self._adapters_changed()

    @torch.no_grad()
    def merge_lora(self):
        """Folds s B A into the base weights (W + s B A in fp32, rounded once to the model dtype), removes the adapters and turns LoRA off:
        state_dict() then has exactly the reference's keys."""
        if self.lora_cfg is None:
            raise ValueError("merge_lora: the model has no LoRA adapters")
        eng = self.engine
        eng.wait_param_updates()
        params = dict(self.named_parameters())
        for l in range(self.dims.lm.num_hidden_layers):
            for t in self.lora_cfg.targets:
                W = params[lora.base_name(l, t)].data
                W.copy_(eng.lora_merged(l, t))
        for l in range(self.dims.lm.num_hidden_layers):
            for t in self.lora_cfg.targets:
                mod = self
                for q in lora.adapter_names(l, t)[0].split(".")[:-2]:
                    mod = getattr(mod, q)
                del mod.lora_A, mod.lora_B
        self.lora_cfg = None
        if hasattr(self.args, "lora_r"):
            self.args.lora_r = 0
        tr = [n for n in eng.trainable if not lora.is_adapter(n)]
        self.engine = None
        self._build_engine()
        self.engine.set_trainable(tr)
        return self

    # -- plumbing ---------------------------------------------------------------------------------
    def _build_engine(self):
        tensors = {k: v for k, v in self.named_parameters()}
        tensors.update({k: v for k, v in self.named_buffers()})
        dtype = self.model.embed_tokens.weight.dtype
        dev = self.model.embed_tokens.weight.device
        old = self.engine
        self.__dict__.pop("_decoders", None)                # decoders hold stacked copies of the old engine's weights
        self.__dict__.pop("_scorers", None)
        self.engine = Engine(self.dims, {k: v.data for k, v in tensors.items()}, dev, dtype)
        self.engine.param_ref = dict(self.named_parameters())
        self.engine.lora = self.lora_cfg
        if old is not None:
            self.engine.trainable = old.trainable
        pb = self.dims.pb
        cfg = self.point_backbone_config or {}
        cfg.update({"point_cloud_dim": pb.point_dims, "backbone_output_dim": pb.trans_dim,
                    "project_output_dim": self.dims.lm.hidden_size, "point_token_len": pb.point_token_len,
                    "mm_use_point_start_end": True, "projection_hidden_layer": len(pb.projection_hidden_dim),
                    "projection_hidden_dim": list(pb.projection_hidden_dim), "use_max_pool": False})     # pointllm.py:49-59
        self.point_backbone_config = cfg
        self.model.point_backbone_config = cfg
        self.model.load_point_backbone_checkpoint = self.load_point_backbone_checkpoint     # the reference calls it on get_model() (pointllm.py:86)

    def get_model(self):
        return self.model

    def state_dict(self, *a, **k):
        if getattr(self, "engine", None) is not None:
            self.engine.wait_param_updates()                # an overlapped optimizer step (EgoAdamW.step(overlap=True)) may still be writing parameters
        return super().state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        if getattr(self, "engine", None) is not None:
            self.engine.wait_param_updates()
        r = super()._apply(fn, *a, **k)
        if getattr(self, "engine", None) is not None:
            self._build_engine()
        return r

    def load_state_dict(self, sd, strict=True, **kw):
        self.engine.wait_param_updates()
        r = super().load_state_dict(sd, strict=strict, **kw)
        self.engine.prepared = False
        self.engine.lm_wT_stale = True          # the padded lm_head transpose follows the loaded values
        self.engine.lora_version += 1           # ... and merged decode copies the loaded adapters
        return r

    def load_pretrained_weights(self):
        """HF directory: *.safetensors shards or pytorch_model*.bin (model_arch.py:25-31)."""
        files = sorted(f for f in os.listdir(self.model_name) if f.endswith(".safetensors"))
        sd = {}
        if files:
            from safetensors.torch import load_file
            for f in files:
                sd.update(load_file(os.path.join(self.model_name, f)))
        else:
            for f in sorted(f for f in os.listdir(self.model_name) if f.startswith("pytorch_model") and f.endswith(".bin")):
                sd.update(torch.load(os.path.join(self.model_name, f), map_location="cpu", weights_only=True))
        if sd:
            self.load_state_dict(sd, strict=False)

    def load_point_backbone_checkpoint(self, checkpoint_path=None):
        """pointllm.py:86-87 -> PointTransformer.load_checkpoint (point_encoder.py:144-166): a PointBERT pre-training checkpoint, `torch.save`d as
        {'state_dict': {...}}; the keys prefixed `module.point_encoder.` are the encoder's own state dict and are loaded non-strictly, every
        other key of the file (classification heads, the dVAE) is ignored.  Returns the (missing_keys, unexpected_keys) the reference prints.
        The file is read with weights_only=True: nothing in it can execute."""
        path = checkpoint_path if checkpoint_path is not None else getattr(self.config, "point_backbone_ckpt", None)
        if path is None:
            raise ValueError("no checkpoint path: pass one or set config.point_backbone_ckpt")
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        pre, dst = "module.point_encoder.", "model.point_backbone."
        src = {k[len(pre):]: v for k, v in ckpt["state_dict"].items() if k.startswith(pre)}
        own = {k[len(dst):]: v for k, v in super().state_dict().items() if k.startswith(dst)}
        self.engine.wait_param_updates()
        with torch.no_grad():
            for k, v in src.items():
                if k in own:
                    if own[k].shape != v.shape:
                        raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(v.shape)} from checkpoint, "
                                           f"the shape in current model is {tuple(own[k].shape)}.")      # load_state_dict raises on shapes even when not strict
                    own[k].copy_(v)
        missing = [k for k in own if k not in src]
        unexpected = [k for k in src if k not in own]
        self.engine.prepared = False                        # BatchNorm fold / stacked copies follow the loaded values
        if not missing and not unexpected:
            print(f"PointBERT's weights are successfully loaded from {path}")
        else:
            print("missing_keys", missing, "unexpected_keys", unexpected)
        return types.SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def save_pretrained(self, path):
        from safetensors.torch import save_file
        if isinstance(self.config, PointLLMConfig):
            self.config.save_pretrained(path)
        os.makedirs(path, exist_ok=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}, os.path.join(path, "model.safetensors"))

    def _configure_trainable_parameters(self):
        """model_arch.py:33-51: point backbone frozen unless --unfreeze_pc_encoder; model.layers
        frozen unless --unfreeze_language_model; embed_tokens always trainable; everything else
        (point_proj, model.norm, lm_head) keeps requires_grad=True."""
        unfreeze_pc = bool(getattr(self.args, "unfreeze_pc_encoder", False))
        unfreeze_llm = bool(getattr(self.args, "unfreeze_language_model", False))
        names = []
        for n, p in self.named_parameters():
            if n.startswith("model.point_backbone."):
                p.requires_grad = unfreeze_pc
            elif lora.is_adapter(n):
                p.requires_grad = True                     # LoRA: the adapters train, their base weights stay frozen
            elif n.startswith("model.layers."):
                p.requires_grad = unfreeze_llm
            else:
                p.requires_grad = True
            if p.requires_grad:
                names.append(n)
        self.engine.set_trainable(names)

    def resize_token_embeddings(self, new_num_tokens, mean_resizing=False):
        """builder.py:44: grow embed_tokens / lm_head; new rows N(0, 0.02) like HF with
        mean_resizing=False (std = initializer_range)."""
        old = self.dims.lm.vocab_size
        if new_num_tokens == old:
            return
        for name in ("model.embed_tokens.weight", "lm_head.weight"):
            mod, leaf = self, name
            parts = name.split(".")
            for q in parts[:-1]:
                mod = getattr(mod, q)
            w = getattr(mod, parts[-1])
            nw = torch.empty(new_num_tokens, w.shape[1], dtype=w.dtype, device=w.device)
            n = min(old, new_num_tokens)
            nw[:n] = w.data[:n]
            if new_num_tokens > old:
                nw[old:].normal_(0.0, 0.02)
            mod.register_parameter(parts[-1], nn.Parameter(nw, requires_grad=w.requires_grad))
        self.dims.lm.vocab_size = new_num_tokens
        if hasattr(self.config, "vocab_size"):
            self.config.vocab_size = new_num_tokens
        tr = self.engine.trainable
        self.engine = None
        self._build_engine()
        self.engine.trainable = tr
        self.engine.main_grad, self.engine.layer_flat = {}, {}

    def initialize_tokenizer_point_backbone_config_wo_embedding(self, tokenizer):
        """pointllm.py:277-300."""
        cfg = self.point_backbone_config
        pp = getattr(self.config, "DEFAULT_POINT_PATCH_TOKEN", "<point_patch>")
        tokenizer.add_tokens([pp], special_tokens=True)
        cfg["default_point_patch_token"] = pp
        cfg["point_patch_token"] = tokenizer.convert_tokens_to_ids([pp])[0]
        ps = getattr(self.config, "DEFAULT_POINT_START_TOKEN", "<point_start>")
        pe = getattr(self.config, "DEFAULT_POINT_END_TOKEN", "<point_end>")
        tokenizer.add_tokens([ps, pe], special_tokens=True)
        cfg["default_point_start_token"], cfg["default_point_end_token"] = ps, pe
        cfg["point_start_token"] = tokenizer.convert_tokens_to_ids([ps])[0]
        cfg["point_end_token"] = tokenizer.convert_tokens_to_ids([pe])[0]
        self.set_point_token_ids(cfg["point_patch_token"], cfg["point_start_token"], cfg["point_end_token"])

    def set_point_token_ids(self, patch, start, end):
        t = self.dims.tok
        t.point_patch, t.point_start, t.point_end = int(patch), int(start), int(end)
        self.point_backbone_config.update(point_patch_token=int(patch), point_start_token=int(start), point_end_token=int(end))

    # -- gradients ----------------------------------------------------------------------------------
    def _begin_backward(self, explicit=False):
        """explicit=True (loss_and_backward): gradients are overwritten unless `accumulate_grads` is set, for both dtypes.
        explicit=False (torch autograd driving `_LogitsFn`): fp32 follows torch semantics (`p.grad is None` after
        `optimizer.zero_grad()` means fresh, otherwise accumulate); bf16 has no `.grad` and follows `accumulate_grads`."""
        eng = self.engine
        eng._xt_last.clear()                 # transposed-activation cache of engine._wgrad is valid within one backward only
        for n, p in self.named_parameters():
            if n in eng.trainable:
                g = eng.grad_buffer(n)
                fresh = (p.grad is None) if (p.dtype == torch.float32 and not explicit) else (not self.accumulate_grads)
                if fresh:
                    if eng.lazy_zero_ok(n):
                        eng.grad_fresh.add(n)          # overwritten by its first wgrad product (engine._wgrad)
                    else:
                        g.zero_()

    def _publish_grads(self):
        eng = self.engine
        eng.flush_fresh()
        for n, p in self.named_parameters():
            if n in eng.trainable:
                g = eng.reduced_grad.get(n, eng.main_grad[n])     # (resident exchange: the bf16 view the optimizer will read)
                p.main_grad = g
                if p.dtype == torch.float32:
                    p.grad = g

    # -- reference API --------------------------------------------------------------------------------
    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, inputs_embeds=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, point_clouds=None, return_dict=None,
                fps_start=None):
        """model_arch.py:53-75: only input_ids / attention_mask / point_clouds / return_dict are used."""
        dev = self.engine.device
        input_ids = input_ids.to(dev)
        if fps_start is None and point_clouds is not None:
            n = point_clouds[0].shape[0] if isinstance(point_clouds, (list, tuple)) else point_clouds.shape[1]
            b = len(point_clouds) if isinstance(point_clouds, (list, tuple)) else point_clouds.shape[0]
            fps_start = torch.randint(0, n, (b,), dtype=torch.long)            # misc.py:52 (global CPU RNG)
        save = torch.is_grad_enabled() and self.training_graph
        logits = _LogitsFn.apply(self._anchor, self, input_ids, attention_mask, point_clouds, fps_start, save)
        out = CausalLMOutput(logits=logits)
        return out if (return_dict is None or return_dict) else (logits,)

    last_nll = None           # loss_and_backward(bin_soft=spec): the mean hard loss of the step's rows, a device fp32 scalar

    def loss_and_backward(self, input_ids, attention_mask, point_clouds, prompt_len, pad_token_id, fps_start=None,
                          backward=True, grad_scale=1.0, bin_soft=None):
        """Fused training step of train.py:166-183: forward, lm_head restricted to the trajectory span
        [Lp-1, S-1), cross-entropy with ignore_index=pad (mean), and the full backward, without
        materialising [B,S,V] logits.  Returns the loss (fp32 scalar tensor).

        bin_soft=traj.soft_target_spec(tok, sigma, radius): the bin-aware loss.  Rows whose target is a bin token are scored against a
        truncated discrete Gaussian over the neighbouring bins instead of the one-hot (ops.cross_entropy_soft, egomi_ce_soft_fwd_bwd); the
        returned loss and the gradients are those of that soft loss, and self.last_nll holds the mean hard loss of the same rows (what the
        call without bin_soft returns for these logits) as a device fp32 scalar, without a host sync.  None: the reference's loss."""
        eng = self.engine
        dev = eng.device
        input_ids = input_ids.to(dev)
        B, S = input_ids.shape
        if fps_start is None and point_clouds is not None:
            fps_start = torch.randint(0, point_clouds.shape[1], (B,), dtype=torch.long)
        Lp = int(prompt_len)
        # the loss reads rows [Lp-1, S-1) only: where the engine can, its top decoder layer runs on the R = S - Lp + 1 rows from Lp-1 on
        # (a window that ends with the sequence, as the attention kernels' query window needs) and hn comes back compact [B*R, d]
        hn = eng.forward_hidden(input_ids, attention_mask, point_clouds, fps_start, save=backward, loss_from=Lp - 1 if backward else None)
        d = hn.shape[1]
        R = eng.ctx.get("top_rows", 0) if backward else 0
        if R:
            hs = hn.view(B, R, d)[:, :R - 1].reshape(-1, d)
        else:
            hs = hn.view(B, S, d)[:, Lp - 1:S - 1].reshape(-1, d)
        tg = input_ids[:, Lp:].reshape(-1).contiguous()
        lg = eng.logits(hs, padded=backward)
        if bin_soft is None:
            ls, cnt = ops.cross_entropy(lg, tg, pad_token_id, dlogits=lg if backward else None, grad_scale=grad_scale)
        else:
            ls, nll, cnt = ops.cross_entropy_soft(lg, tg, pad_token_id, bin_soft, dlogits=lg if backward else None, grad_scale=grad_scale)
            self.last_nll = (nll / cnt.float())[0]
        loss = ls / cnt.float()
        if backward:
            self._begin_backward(explicit=True)
            d_hs = eng.backward_logits(lg, hs)
            if R:
                eng.backward_hidden(eng.compact_loss_grad(d_hs))
            else:
                d_hn = eng.ws.get("d_hn_full", (B, S, d), eng.dtype, zero=True)
                d_hn[:, Lp - 1:S - 1] = d_hs.view(B, S - Lp, d)
                eng.backward_hidden(d_hn.view(B * S, d))
            self._publish_grads()
        return loss[0]

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, point_clouds=None, max_length=20, temperature=1.0, top_k=50,
                 top_p=0.95, repetition_penalty=1.0, do_sample=True, num_return_sequences=1, fps_start=None,
                 eos_token_id="config", pad_token_id=None, seed=None, num_beams=1, length_penalty=1.0, early_stopping=False, kv_cache_dtype=None,
                 decode_weight_dtype=None, share_prompt=False, kv_cache_layout=None, output_logprobs=False, rank_length_penalty=1.0, output_bin_stats=False,
                 bin_token_ids=None, traj_grammar=None, traj_limits=None, **kwargs):
        """model_arch.py:77-108: `max_length` means max_new_tokens; returns .sequences [B,S0+T'] and .scores (T' x [B,V], the PROCESSED
        scores, as HF returns them with output_scores=True).  Prefill runs encoder + splice and fills the KV cache; every later step
        feeds one token (the behaviour pointllm.py:112,255-275 intends; see DESIGN.md on the reference's cache bug).

        Every mode runs on the device under one hipGraph (decode.Decoder.sample -> egomi_sample_rows): repetition penalty, temperature,
        top-k, top-p in HF's order and with HF's tie rules (golden: tests/golden/sampling.npz, recorded from HF's own processors on the
        reference model's logits), a draw from the softmax (Gumbel-max on a counter-based generator seeded from torch's CPU generator —
        torch.multinomial's stream cannot be reproduced, so parity is on `.scores` and, with do_sample=False, on the ids), and HF's
        eos rule: `eos_token_id` defaults to the config's (GenerationConfig.from_model_config), finished rows emit `pad_token_id`, and
        the outputs are cut after the step at which every row has finished.  eos_token_id=None: fixed length, never stops.

        num_beams > 1: HF's beam search (do_sample=False) or beam sampling (do_sample=True), generation/utils.py _beam_search, on the
        device under one hipGraph (decode.Decoder.beam -> egomi_beam_rows / egomi_beam_update / egomi_attn_decode_rows; each prompt is
        prefilled once and shared by its beams).  Returns GenerateBeamOutput(sequences [B*nrs, S0+Lgen], sequences_scores [B*nrs], scores
        (one [B*num_beams, V] per iteration HF runs: processed log-probs), beam_indices [B*nrs, Lgen]).  Golden: tests/golden/beam_search.npz,
        recorded from HF's own generate.

        kv_cache_dtype: None or "auto" = a KV cache in the model's dtype; "fp8" = OCP e4m3fn codes with one fp32 scale per (layer, row,
        head, position) and tensor, s = amax / 448 (decode.Decoder(kv_dtype="fp8"), csrc/kv8.hip): half the cache bytes of bf16, and of what
        every decode step's attention streams.  Applies to every mode; the prefill logits (step 0) never read the cache.

        decode_weight_dtype: None or "auto" = the decode steps multiply the model's weights; "fp8" = the four projections of every decoder
        layer (q|k|v, o_proj, gate|up, down_proj) run on OCP e4m3fn codes with one fp32 scale per output row, s = amax / 448, W8A16
        (decode.Decoder(weight_dtype="fp8"), csrc/w8.hip): half the weight bytes every decode step streams.  lm_head, the embeddings and the
        norms keep the model's dtype.  Applies to every mode and either kv_cache_dtype; bf16 models with at most 512 decoder rows
        (batch x num_beams) only.  The prefill runs on the bf16 weights, so the prefill logits (step 0) are those of the bf16 run; only
        the later steps read the fp8 weights.  "int4" = the same four projections on symmetric 4-bit codes (-7 .. 7) with one fp32 scale per
        output row and 128-column group, s = amax / 7, W4A16 (decode.Decoder(weight_dtype="int4"), csrc/w4.hip): 0.53 of the fp8 form's
        weight bytes per step, with about 4.5 times its weight error (11.7 % against 2.6 % on Gaussian weights; the accuracy on a trained
        checkpoint is not measured).  Accepted wherever "fp8" is, under the same limits.

        share_prompt=True with num_return_sequences = K > 1 and num_beams == 1 (best-of-K sampling): same outputs, shapes and row order
        (row b * K + j = sample j of prompt b) as the default, but every prompt is prefilled ONCE and its K/V are kept once: the decoder holds
        a prompt cache [L, B, H, S0, hd] plus a suffix cache [L, B*K, H, max_length, hd], and every step's attention reads a prompt's K/V once
        for its K samples (decode.Decoder(samples_per_prompt=K), csrc/shared.hip).  The draws of row r are those of the default path (same
        seed, same row numbering), but the attention sums in another order, so logits differ in their last bits and a sampled token can
        differ at a near-tie; hence the default stays False.  1 <= K <= 32 (K = 1 is the default path); not with num_beams > 1, a list of
        ragged clouds or kv_cache_dtype="fp8"; decode_weight_dtype="fp8" and LoRA adapters work as in the default path.

        kv_cache_layout: None or "dense" = one cache row of S0 + max_length keys per beam (only the items' rows ever hold prompt keys);
        "split" with num_beams > 1 = the prompt / suffix layout of share_prompt for beam search: one prompt cache row per item
        [L, B, H, S0, hd] plus one suffix row of max_length keys per beam [L, B*num_beams, H, max_length, hd]
        (decode.Decoder(split_cache=True)), and every step's attention reads an item's prompt K/V once for all its beams and the suffix
        through the beam row table (egomi_attn_decode_shared_rows, csrc/shared.hip).  Same outputs, fields and shapes; the attention sums
        in another order, so scores differ in their last bits.  Not with num_beams == 1 (see share_prompt), kv_cache_dtype="fp8", a list
        of ragged clouds or more than 32 beams; decode_weight_dtype="fp8" and LoRA adapters work as in the dense layout.

        output_logprobs=True (num_beams == 1; HF: output_logits=True + compute_transition_scores): the output also carries the log-probability
        of every generated token under the RAW model distribution -- not under the processed `scores`, where top-k / top-p leave -inf holes --
        computed on the device inside the token loop (one egomi_token_logprob launch per step, csrc/logprob.hip; no raw logits are kept):
        token_logprobs fp32 [rows, T'] (T' = the columns `sequences` keeps; 0 after a row's eos), sequences_logprobs fp32 [rows] (their sum),
        sequences_lengths int32 [rows] (the eos counted, the pads not); with num_return_sequences = K > 1 also sample_scores fp32 [B, K] =
        sum / length ** rank_length_penalty (HF's beam convention: 1.0 = mean log-prob, 0.0 = the sum) and rank int32 [B, K], the clip's
        sample indices by descending score (egomi_seq_rank): rows[b * K + rank[b, 0]] is the sample the model finds most probable.  Every
        other field, the row order and the drawn tokens are those of the call without it; no row is dropped.  Works in every non-beam mode;
        num_beams > 1 raises ValueError (beams return sequences_scores).

        output_bin_stats=True with bin_token_ids=(p0, nb) (num_beams == 1): the per-waypoint view of the same raw distribution.  The nb
        contiguous token ids p0 .. p0 + nb - 1 stand for the values linspace(-1, 1, nb) (the tokenizer's first bin id and num_bins, as
        traj.tokenize_batch / detokenize_batch take them; the model does not know its tokenizer, so the tuple is required).  One
        egomi_bin_stats launch per step inside the token loop (csrc/logprob.hip; no raw logits are kept) fills four fp32 [rows, T'] fields,
        column t describing the distribution token t was drawn from: bin_mass (the probability that the token is a bin token at all),
        bin_mean (E[value | bin token]: a continuous estimate without the quantisation step 2 / (nb - 1)), bin_std and bin_entropy (nats) of
        that conditional distribution; 0 after a row's eos.  It reports and changes nothing: the fed-back token, every other field and the
        graphs of the calls without it are what they were; it combines with output_logprobs (two launches per step).  traj.detokenize_soft
        turns bin_mean / bin_std / bin_mass into trajectories.  num_beams > 1 raises ValueError.

        traj_grammar=traj.grammar_spec(tok, min_steps, max_steps) (num_beams == 1; HF: prefix_allowed_tokens_fn): constrained decoding.  Every
        returned row reads <ts> (bin x 6 <tsep>) x n <te> eos with min_steps <= n <= max_steps from the prompt's last <ts> on, whatever the
        weights: a ten-state machine per row on the device, one egomi_traj_grammar_step launch per step directly before the token kernel
        inside the token loop (csrc/grammar.hip), writes -inf over every id the row's state does not allow.  The state is read from the
        prompt (egomi_traj_grammar_init, before the prefill is queued), and a row that needs more than max_length tokens to close raises
        ValueError naming it.  The mask is in place on the logits, so with the option on `scores` are the processed scores of the
        CONSTRAINED distribution, and output_logprobs / output_bin_stats report on that same renormalised distribution -- the one the token
        was drawn from, a proper distribution over valid trajectories.  What the model itself thought of the grammar survives in
        grammar_mass fp32 [rows, T']: column t = the raw probability of the ids allowed at step t (0 after a row's eos).  eos_token_id must
        be the spec's eos.  Works with every cache and weight dtype, share_prompt and LoRA; num_beams > 1 raises ValueError.  None: every
        graph, launch and output is what it is without the option.

        traj_limits=table (with traj_grammar; traj.motion_limits / motion_limits_bins): per-prompt, per-dimension motion limits on the
        waypoints, enforced on the device at every bin token.  The table is [B, 18] CPU integers in bins, one row per prompt (expanded
        to the K rows of num_return_sequences, with or without share_prompt): lo[6] | hi[6] = the inclusive box of every trajectory
        dimension, dmax[6] = the largest allowed |bin_t - bin_(t-1)| between consecutive waypoints, the prompt's last complete step
        included (csrc/grammar.hip states the rule; a waypoint farther than dmax outside the box moves toward it by dmax per step).  The
        two grammar launches run in their *_limits form and nothing is added to the loop; when a trajectory may end does not change.
        limits_mass fp32 [rows, T'] holds, beside grammar_mass, the raw probability of what the limits left allowed:
        limits_mass / grammar_mass is how much the model wanted to break them.  The table lives in a device buffer the captured loop
        reads, so a call with another table replays the same graph.  Needs traj_grammar; num_beams > 1 raises ValueError.  None: every
        graph, launch and output is what generate(traj_grammar=...) gives without it."""
        if traj_limits is not None and traj_grammar is None:
            raise ValueError("traj_limits narrows the bin window of the trajectory grammar: it needs traj_grammar")
        if traj_limits is not None and int(num_beams) > 1:
            raise ValueError("traj_limits is for num_beams == 1, like traj_grammar")
        if traj_grammar is not None and int(num_beams) > 1:
            raise ValueError("traj_grammar is for num_beams == 1: the beams of an item share one prefill logits row at step 0")
        if output_logprobs and int(num_beams) > 1:
            raise ValueError("output_logprobs=True is for num_beams == 1; beam search returns `sequences_scores` (length-penalised sums of "
                             "the beams' log-probs)")
        if output_bin_stats and int(num_beams) > 1:
            raise ValueError("output_bin_stats=True is for num_beams == 1; beam search keeps no per-step distribution of its hypotheses")
        bins = self._bin_window(bin_token_ids) if output_bin_stats else None
        if kv_cache_layout not in (None, "dense", "split"):
            raise ValueError(f"`kv_cache_layout` must be None, 'dense' or 'split', but is {kv_cache_layout!r}")
        split = kv_cache_layout == "split"
        if split:
            if int(num_beams) == 1:
                raise ValueError("kv_cache_layout='split' needs num_beams > 1; for independent samples of one prompt use share_prompt=True")
            if kv_cache_dtype == "fp8":
                raise NotImplementedError("kv_cache_layout='split' with kv_cache_dtype='fp8' is not built")
            if isinstance(point_clouds, (list, tuple)):
                raise NotImplementedError("kv_cache_layout='split' with a list of ragged clouds is not built")
            if int(num_beams) > 32:
                raise ValueError(f"kv_cache_layout='split' supports at most 32 beams, not {num_beams}")
            if int(max_length) < 1:
                raise ValueError("kv_cache_layout='split' needs max_length >= 1")
        share = bool(share_prompt) and int(num_return_sequences) > 1
        if share_prompt:
            if int(num_beams) > 1:
                raise NotImplementedError("share_prompt=True with num_beams > 1 is not built (beam search already prefills each prompt once; "
                                          "kv_cache_layout='split' gives it the prompt / suffix cache)")
            if isinstance(point_clouds, (list, tuple)):
                raise NotImplementedError("share_prompt=True with a list of ragged clouds is not built")
            if kv_cache_dtype == "fp8":
                raise NotImplementedError("share_prompt=True with kv_cache_dtype='fp8' is not built")
            if int(num_return_sequences) > 32:
                raise ValueError(f"share_prompt=True supports at most 32 return sequences, not {num_return_sequences}")
        if kv_cache_dtype not in (None, "auto", "fp8"):
            raise ValueError(f"`kv_cache_dtype` must be None, 'auto' or 'fp8', but is {kv_cache_dtype!r}")
        kv = "fp8" if kv_cache_dtype == "fp8" else None
        if decode_weight_dtype not in (None, "auto", "fp8", "int4"):
            raise ValueError(f"`decode_weight_dtype` must be None, 'auto', 'fp8' or 'int4', but is {decode_weight_dtype!r}")
        wd = decode_weight_dtype if decode_weight_dtype in ("fp8", "int4") else None
        dev = self.engine.device
        ids, fps_start = self._decode_inputs(input_ids, point_clouds, fps_start)
        n_ret = int(num_return_sequences)
        limits = None
        if traj_limits is not None:                        # checked per prompt, then one row per decoder row (row b * K + j = sample j of prompt b)
            from ..decode import grammar_check, traj_limits_check
            limits = traj_limits_check(traj_limits, grammar_check(traj_grammar, self.dims.lm.vocab_size)[1], ids.shape[0])
            limits = limits.repeat_interleave(max(n_ret, 1), 0)
        nb = int(num_beams)
        if nb < 1:
            raise ValueError(f"`num_beams` has to be a strictly positive integer, but is {num_beams}")
        if early_stopping not in (True, False, "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping}.")
        if nb > 1:
            if n_ret > nb:                                 # configuration_utils.py:802
                raise ValueError("`num_return_sequences` has to be smaller or equal to `num_beams`.")
            if isinstance(point_clouds, (list, tuple)):
                raise NotImplementedError("num_beams > 1 with a list of ragged clouds is not built")
            return self._generate_beam(ids, attention_mask, point_clouds, fps_start, int(max_length), nb, n_ret, float(length_penalty),
                                       early_stopping, do_sample, temperature, top_k, top_p, repetition_penalty, eos_token_id, pad_token_id,
                                       seed, kwargs.get("use_graph", True), kv, wd, split)
        if n_ret > 1 and not share:                        # HF expands every input n times (generation/utils.py _expand_inputs_for_generation)
            if isinstance(point_clouds, (list, tuple)):
                raise NotImplementedError("num_return_sequences > 1 with a list of ragged clouds is not built")
            ids = ids.repeat_interleave(n_ret, 0)
            attention_mask = None if attention_mask is None else attention_mask.to(dev).repeat_interleave(n_ret, 0)
            point_clouds = None if point_clouds is None else point_clouds.to(dev).repeat_interleave(n_ret, 0)
            fps_start = None if fps_start is None else torch.as_tensor(fps_start).to(dev).repeat_interleave(n_ret, 0)
        B, S0 = ids.shape
        T = int(max_length)
        if share and T < 1:
            raise ValueError("share_prompt=True needs max_length >= 1")
        eos_token_id, pad_token_id = self._sampling_args(eos_token_id, pad_token_id, temperature, repetition_penalty, top_p)
        grammar = self._grammar_ready(traj_grammar, ids, attention_mask, eos_token_id, T) if traj_grammar is not None else None
        # one Decoder (static KV cache + captured token loops) per geometry, kept while the decoder layers it holds stacked copies of cannot
        # change: frozen-LLM mode, same prepared weights.  run_validation / evaluate (train.py:207-264, evaluate.py:104-154) call generate()
        # once per batch: without this every batch re-allocated the cache and re-captured a graph of (new tokens x ~300) kernels
        if share:                                          # B prompts, B * n_ret decoder rows: one prefill and one cached K/V per prompt
            dec = self._decoder(B * n_ret, S0 + T, kv=kv, wd=wd, share=(n_ret, T))
            self._prefill_prompts(dec, ids, attention_mask, point_clouds, fps_start, T)
            B = B * n_ret
        else:
            dec = self._decoder(B, S0 + T, kv=kv, wd=wd)
            dec.prefill(ids, attention_mask, point_clouds, fps_start, T)
        if not do_sample:                                  # HF applies the warpers (temperature / top-k / top-p) in sampling mode only
            temperature, top_k, top_p = 1.0, 0, 1.0
        seq, sc = dec.sample(T, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                             eos=eos_token_id, pad=pad_token_id, seed=seed, use_graph=kwargs.get("use_graph", True),
                             logprobs=bool(output_logprobs), bin_stats=bins, grammar=grammar, limits=limits)
        stop = T
        if eos_token_id is not None and T > 0:             # HF leaves the loop after the step at which the last unfinished row emitted eos
            hit = seq[:, S0:] == eos_token_id
            first = torch.where(hit.any(1), hit.int().argmax(1), torch.full((B,), T - 1, device=dev))
            stop = int(first.max()) + 1
        sc = sc[:stop].clone()                              # the decoder's buffers are static (and the decoder may be reused by the next call):
        out = GenerateOutput(sequences=seq[:, :S0 + stop].clone(), scores=tuple(sc[t] for t in range(stop)))     # hand out copies
        if output_logprobs:
            _fill_logprobs(out, dec, stop, (B // n_ret, n_ret) if n_ret > 1 else None, rank_length_penalty)
        if bins is not None or grammar is not None:
            from ..decode import candidate_lengths
            past = torch.arange(stop, device=dev)[None, :] >= candidate_lengths(out.sequences[:, S0:], eos_token_id)[:, None]
        if bins is not None:
            _fill_bin_stats(out, dec, stop, past=past)
        if grammar is not None:
            out.grammar_mass = dec.gr_mass[:, :stop].masked_fill(past, 0.0)
        if limits is not None:
            out.limits_mass = dec.gr_limits_mass[:, :stop].masked_fill(past, 0.0)
        return out

    def _grammar_ready(self, traj_grammar, ids, attention_mask, eos_token_id, T):
        """generate(traj_grammar=...) before its prefill: the checked spec, after one egomi_traj_grammar_init launch on the prompts whose
        `need` is read back: a prompt row that cannot close inside T new tokens raises ValueError."""
        from ..decode import grammar_check, traj_grammar_init
        spec = grammar_check(traj_grammar, self.dims.lm.vocab_size)
        if eos_token_id != spec[5]:
            raise ValueError(f"traj_grammar closes every row with eos = {spec[5]}: `eos_token_id` must be that id, not {eos_token_id}")
        dev, B = ids.device, ids.shape[0]
        mask = None if attention_mask is None else attention_mask.to(dev).to(torch.uint8).contiguous()
        state = torch.empty(B, 2, dtype=torch.int32, device=dev)
        need = torch.empty(B, dtype=torch.int32, device=dev)
        traj_grammar_init(ids.to(torch.int64).contiguous(), mask, spec, state, need)
        need = need.cpu()
        short = (need > T).nonzero()
        if short.numel():
            r = int(short[0, 0])
            raise ValueError(f"traj_grammar: prompt row {r} needs {int(need[r])} new tokens to close its trajectory, max_length is {T}"
                             + (" (the prompt already holds more steps than max_steps)" if int(need[r]) >= (1 << 30) else ""))
        return spec

    def _decode_inputs(self, input_ids, point_clouds, fps_start):
        """The start of generate() and score(): pending parameter updates are waited for (the decoder reads the weights outside the engine's
        forward pass); -> (the ids on the device, fps_start or its default draw from torch's CPU generator, misc.py:52)."""
        eng = self.engine
        eng.wait_param_updates()
        ids = input_ids.to(eng.device)
        if fps_start is None and point_clouds is not None:
            fps_start = torch.randint(0, point_clouds.shape[1], (ids.shape[0],), dtype=torch.long)
        return ids, fps_start

    def _bin_window(self, bin_token_ids):
        from ..decode import bin_window
        if bin_token_ids is None:
            raise ValueError("output_bin_stats=True needs `bin_token_ids` = (first bin token id, number of bins), the tokenizer's p0 and "
                             "num_bins: the model does not know which of its ids are bins")
        return bin_window(bin_token_ids, self.dims.lm.vocab_size)

    @torch.no_grad()
    def score(self, input_ids, attention_mask, point_clouds, candidates, fps_start=None, eos_token_id="config", rank_length_penalty=1.0,
              row_budget=16384, output_bin_stats=False, bin_token_ids=None):
        """Teacher-forced log-probs of GIVEN trajectories on a shared prompt: candidates int64 [B, K, T] are K token suffixes per prompt
        (1 <= K <= 32; sampled by another call, another seed or a quantized decoder, proposed by a planner, or the ground truth at K = 1).
        Every prompt is prefilled once; ONE further pass over tokens 0 .. T-2 of all B * K candidates gives the logits of tokens 1 .. T-1
        (decode.Decoder.score, egomi_attn_suffix_shared in csrc/shared.hip: each suffix query attends over its clip's prompt cache and
        its own causal suffix), always on the model's own weights (with merged LoRA adapters), never on quantized ones.  `row_budget`
        bounds the token rows of one pass: larger batches run clip group by clip group.

        eos_token_id: generate()'s rule ("config", an int or None).  A candidate counts through its first eos; whatever follows it is
        ignored and scores 0.  None counts all T tokens.  Returns a GenerateOutput with the fields, dtypes and row order (b * K + j) of
        generate(output_logprobs=True): token_logprobs fp32 [B*K, T], sequences_logprobs fp32 [B*K], sequences_lengths int32 [B*K],
        sample_scores fp32 [B, K] = sum / length ** rank_length_penalty, rank int32 [B, K]; sequences = the candidates [B*K, T], scores = ().
        output_bin_stats=True with bin_token_ids=(p0, nb) (generate()'s arguments): also bin_mass / bin_mean / bin_std / bin_entropy fp32
        [B, K, T] -- where the model would have put each waypoint coordinate of a proposal and how sure it was there (egomi_bin_stats on
        the logits every token is scored under, clip group by clip group; no [B*K*T, V] logits are kept); 0 at and after a candidate's eos.
        ValueError: K > 32, T < 1, candidates of another rank / dtype / batch, S0 + T beyond max_position_embeddings.
        NotImplementedError: a list of ragged clouds."""
        from ..decode import Decoder
        if isinstance(point_clouds, (list, tuple)):
            raise NotImplementedError("score() with a list of ragged clouds is not built")
        if not torch.is_tensor(candidates) or candidates.dim() != 3 or candidates.dtype != torch.int64:
            raise ValueError("score(): `candidates` must be an int64 tensor [B, K, T]")
        B, S0 = input_ids.shape
        Bc, K, T = candidates.shape
        if Bc != B:
            raise ValueError(f"score(): {Bc} candidate sets for {B} prompts")
        if not 1 <= K <= 32:
            raise ValueError(f"score() supports 1 to 32 candidates per prompt, not {K}")
        if T < 1:
            raise ValueError("score() needs candidates of at least one token")
        if S0 + T > self.dims.lm.max_position_embeddings:
            raise ValueError(f"score(): prompt ({S0}) + candidate ({T}) tokens exceed max_position_embeddings "
                             f"({self.dims.lm.max_position_embeddings})")
        if isinstance(eos_token_id, str):
            eos_token_id = self.dims.tok.eos
        bins = self._bin_window(bin_token_ids) if output_bin_stats else None
        ids, fps_start = self._decode_inputs(input_ids, point_clouds, fps_start)
        # scorer decoders have a cache of their own (_cached_decoder's rule): generate()'s two cached decoders stay what they were
        dec = self._cached_decoder("_scorers", (B, K, S0, T), lambda eng: Decoder(eng, B * K, S0 + T, samples_per_prompt=K, max_new_tokens=T,
                                                                                   score_cache=True))
        self._prefill_prompts(dec, ids, attention_mask, point_clouds, fps_start, T)
        cand = candidates.to(ids.device).reshape(B * K, T)
        dec.score(cand, eos_token_id, row_budget=row_budget, bin_stats=bins)
        out = GenerateOutput(sequences=cand.clone(), scores=())
        if bins is not None:
            _fill_bin_stats(out, dec, T, shape=(B, K, T))
        _fill_logprobs(out, dec, T, (B, K), rank_length_penalty)
        return out

    def _sampling_args(self, eos_token_id, pad_token_id, temperature, repetition_penalty, top_p):
        """-> (eos, pad) as HF resolves them: eos "config" = the config's, pad defaults to the config's or, when it has none, to eos; raises
        on a temperature, repetition penalty or top_p that HF's processors reject (logits_process.py:239,307)."""
        if isinstance(eos_token_id, str):
            eos_token_id = self.dims.tok.eos
        if eos_token_id is not None and pad_token_id is None:
            pad_token_id = self.dims.tok.pad if self.dims.tok.pad is not None else eos_token_id
        for name, v in (("temperature", temperature), ("repetition_penalty", repetition_penalty)):
            if v is not None and not float(v) > 0:
                raise ValueError(f"`{name}` has to be a strictly positive float, but is {v}")
        if top_p is not None and not (0 < float(top_p) <= 1.0):
            raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
        return eos_token_id, pad_token_id

    def _prefill_prompts(self, dec, ids, attention_mask, point_clouds, fps_start, T, nb=1):
        """Prefill of a decoder whose prompts are fewer than its rows (beams, shared prompt): more than 16 prompts run chunked."""
        return dec.prefill(ids, attention_mask, point_clouds, fps_start, T, nb=nb, chunk=16 if ids.shape[0] > 16 else None)

    def _decoder(self, B, max_len, nb=1, kv=None, wd=None, share=None, split=None):
        """The cached Decoder of this geometry.  The key holds the engine's identity and the epoch of its prepared weights, taken AFTER
        prepare(): load_state_dict() / _apply() leave the engine unprepared (or replace it), and a decoder made before them holds stacked
        copies of the old weights and the old RoPE tables.  It also holds the KV dtype and the decode weight dtype: a bf16 and an fp8 decoder never
        stand in for each other.  share = (K, Tmax): the shared-prompt decoder of K samples per prompt; the key holds the mode and K.
        split = Tmax: the beam decoder on the prompt / suffix cache layout; the key holds the layout and Tmax."""
        from ..decode import Decoder
        kw, layout = dict(kv_dtype=kv, weight_dtype=wd), ()
        if share is not None:
            kw.update(samples_per_prompt=share[0], max_new_tokens=share[1])
            layout = ("share", *share)
        elif split is not None:
            kw.update(split_cache=True, max_new_tokens=split)
            layout = ("split", split)
        return self._cached_decoder("_decoders", (B, max_len, nb, kv, wd), lambda eng: Decoder(eng, B * nb, max_len, num_beams=nb, **kw), layout)

    def _cached_decoder(self, attr, geometry, build, layout=()):
        """The one rule of both decoder caches (self._decoders, self._scorers: plain dicts, made on first use, dropped by _build_engine):
        prepare the engine FIRST, then key on its identity, the epoch of its prepared weights, `geometry`, the LoRA key (adapters: a decoder
        holds merged copies of their values) and `layout`; reuse a decoder only while no decoder layer is trainable and EGOMI_DECODER_CACHE
        is not "0", else build(engine) a fresh one every call and keep nothing; keep at most two per cache, the oldest goes first (the full
        batch and the short last one; a KV cache is 2 * L * B * H * Smax * hd elements)."""
        eng = self.engine
        if not eng.prepared:
            eng.prepare()
        key = (id(eng), eng.prepare_epoch, *geometry, eng.lora_key(), *layout)
        cache = self.__dict__.setdefault(attr, {})
        reuse = not eng.any_layer_trainable and os.environ.get("EGOMI_DECODER_CACHE", "1") != "0"
        dec = cache.get(key) if reuse else None
        if dec is None:
            dec = build(eng)
            if reuse:
                while len(cache) >= 2:
                    cache.pop(next(iter(cache)))
                cache[key] = dec
        return dec

    def _generate_beam(self, ids, attention_mask, point_clouds, fps_start, T, nb, n_ret, length_penalty, early_stopping, do_sample, temperature,
                       top_k, top_p, repetition_penalty, eos_token_id, pad_token_id, seed, use_graph, kv=None, wd=None, split=False):
        B, S0 = ids.shape
        eos_token_id, pad_token_id = self._sampling_args(eos_token_id, pad_token_id, temperature, repetition_penalty, top_p)
        dec = self._decoder(B, S0 + T, nb, kv=kv, wd=wd, split=T if split else None)
        self._prefill_prompts(dec, ids, attention_mask, point_clouds, fps_start, T, nb=nb)
        seq, ss, sc, bidx = dec.beam(T, num_return_sequences=n_ret, length_penalty=length_penalty, early_stopping=early_stopping,
                                     do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                                     eos=eos_token_id, pad=pad_token_id, seed=seed, use_graph=use_graph)
        return GenerateBeamOutput(sequences=seq, sequences_scores=ss, scores=tuple(sc[t] for t in range(sc.shape[0])), beam_indices=bidx)

    def train(self, mode: bool = True):
        """model_arch.py:110-124: frozen parts stay in eval(); embed_tokens follows `mode`."""
        super().train(mode)
        if not getattr(self.args, "unfreeze_language_model", False):
            self.model.layers.eval()
            self.model.embed_tokens.train(mode)
        if not getattr(self.args, "unfreeze_pc_encoder", False):
            self.model.point_backbone.eval()
        self.engine.pb_train_mode = bool(mode) and bool(getattr(self.args, "unfreeze_pc_encoder", False))
        if self.engine.prepared_bn_stale and not self.engine.pb_train_mode:
            self.engine.fold_stale, self.engine.prepared_bn_stale = True, False     # running stats moved: re-fold BN for eval
        return self
