"""Llama-architecture decoder (Llama, Mistral, Qwen3 dense) that threads an ``InferenceController`` through ``QuestAttention``.

The reference ships a fork of HF's modeling_llama (quest/models/llama.py, 835 lines) whose only
Quest-specific parts are: ``quest_init`` / ``quest_clear`` (:520-560), the per-forward controller
sequence in ``LlamaModel.forward`` (:424-439, :486: prepare_metadata -> begin_forward with a huge budget
for the first ``_quest_skip_layer`` = 2 layers -> re-plan with the real budget -> end_forward) and the
fused RMSNorm call (:72).  This module restates exactly those parts around a minimal decoder (embedding,
RMSNorm, QuestAttention, SwiGLU MLP, lm_head) with HF parameter names, so a HF Llama state_dict loads
with ``load_state_dict``; everything else of the HF class hierarchy (generation mixin, attention-mask
plumbing, gradient checkpointing) is out of scope.  Batch size 1, like the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch
from torch import nn

from .. import _kernels
from .. import utils as qutils
from . import rope as rope_mod
from .QuestAttention import QuestAttention


@dataclass
class LlamaConfig:
    vocab_size: int = 32000
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: Optional[int] = None
    rms_norm_eps: float = 1e-5
    max_position_embeddings: int = 32768
    rope_scaling: Optional[dict] = None
    rope_theta: float = 1e4
    head_dim: Optional[int] = None   # None: hidden_size // num_attention_heads (Qwen3, Mistral-Nemo set their own)
    qk_norm: bool = False            # Qwen3: RMSNorm over each head's q and k vector before RoPE
    model_type: str = "llama"        # "llama", "mistral" or "qwen3": what to_hf_dict / save_pretrained write back

    def __post_init__(self):
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads
        if self.model_type not in _ARCHITECTURES:
            raise ValueError(f"model_type = {self.model_type!r}: supported are {sorted(_ARCHITECTURES)}")

    # ---- Hugging Face config.json <-> LlamaConfig (the fields the Quest path reads; quest/models/llama.py takes the
    # whole HF LlamaConfig, of which it uses exactly these)
    @classmethod
    def from_hf_dict(cls, d: dict) -> "LlamaConfig":
        model_type = d.get("model_type", "llama")
        if model_type not in _ARCHITECTURES:
            moe = " (mixture-of-experts models are not supported)" if "moe" in str(model_type) or model_type == "mixtral" else ""
            raise ValueError(f"model_type = {model_type!r} is not supported{moe}: the decoder serves "
                             f"{sorted(_ARCHITECTURES)} (Llama arithmetic, for qwen3 with the per-head q/k norm)")
        rope = d.get("rope_parameters") or {}        # transformers >= 5 nests theta / scaling here
        scaling = d.get("rope_scaling")
        if scaling is None and rope.get("rope_type", "default") not in ("default", None):
            scaling = {k: v for k, v in rope.items() if k != "rope_theta"}
        if float(d.get("partial_rotary_factor", rope.get("partial_rotary_factor", 1.0))) != 1.0:
            raise ValueError("partial rotary embeddings (partial_rotary_factor != 1) are not supported")
        for field in ("attention_bias", "mlp_bias"):
            if d.get(field):
                raise ValueError(f"{field} = true: bias terms are not part of the reference's Llama fork")
        # sliding-window attention is not built: the paged kernels attend the whole cache
        if d.get("use_sliding_window"):
            raise ValueError("use_sliding_window = true: sliding-window attention is not supported")
        if d.get("sliding_window") is not None and d.get("use_sliding_window", True):
            raise ValueError(f"sliding_window = {d['sliding_window']} is set and active: sliding-window attention is not "
                             "supported (a checkpoint trained without it has sliding_window: null)")
        other = sorted({t for t in (d.get("layer_types") or []) if t != "full_attention"})
        if other:
            raise ValueError(f"layer_types holds {other}: only 'full_attention' layers are supported")
        head_dim = d.get("head_dim")
        return cls(vocab_size=d["vocab_size"], hidden_size=d["hidden_size"], intermediate_size=d["intermediate_size"],
                   num_hidden_layers=d["num_hidden_layers"], num_attention_heads=d["num_attention_heads"],
                   num_key_value_heads=d.get("num_key_value_heads"), rms_norm_eps=d.get("rms_norm_eps", 1e-5),
                   max_position_embeddings=d.get("max_position_embeddings", 32768), rope_scaling=scaling,
                   rope_theta=float(d.get("rope_theta", rope.get("rope_theta", 1e4))),
                   head_dim=int(head_dim) if head_dim is not None else None, qk_norm=model_type == "qwen3",
                   model_type=model_type)

    def to_hf_dict(self, dtype: str = "float16", tie_word_embeddings: bool = False) -> dict:
        extra = {}
        if self.head_dim is not None:
            extra["head_dim"] = self.head_dim
        if self.model_type == "mistral":
            extra["sliding_window"] = None  # (transformers' MistralConfig defaults to 4096)
        elif self.model_type == "qwen3":
            extra.update(sliding_window=None, use_sliding_window=False)
        return {**extra, "architectures": [_ARCHITECTURES[self.model_type]], "model_type": self.model_type,
                "hidden_act": "silu",
                "attention_bias": False, "mlp_bias": False, "torch_dtype": dtype, "dtype": dtype,
                "vocab_size": self.vocab_size, "hidden_size": self.hidden_size,
                "intermediate_size": self.intermediate_size, "num_hidden_layers": self.num_hidden_layers,
                "num_attention_heads": self.num_attention_heads, "num_key_value_heads": self.num_key_value_heads,
                "rms_norm_eps": self.rms_norm_eps, "max_position_embeddings": self.max_position_embeddings,
                "rope_scaling": self.rope_scaling, "rope_theta": self.rope_theta,
                "tie_word_embeddings": tie_word_embeddings}


# model_type -> the transformers class that loads what save_pretrained writes
_ARCHITECTURES = {"llama": "LlamaForCausalLM", "mistral": "MistralForCausalLM", "qwen3": "Qwen3ForCausalLM"}


class LlamaRMSNorm(nn.Module):
    def __init__(self, hidden_size: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return qutils.rms_norm_forward(hidden_states, self.weight, self.variance_epsilon)  # llama.py:72


class LlamaMLP(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.gate_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.up_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.down_proj = nn.Linear(config.intermediate_size, config.hidden_size, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.down_proj(torch.nn.functional.silu(self.gate_proj(x)) * self.up_proj(x))


class LlamaDecoderLayer(nn.Module):
    def __init__(self, config: LlamaConfig, layer_idx: int, fused: bool = True):
        super().__init__()
        self.self_attn = QuestAttention(config, layer_idx, fused=fused)
        self.mlp = LlamaMLP(config)
        self.input_layernorm = LlamaRMSNorm(config.hidden_size, config.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNorm(config.hidden_size, config.rms_norm_eps)

    def forward(self, hidden_states: torch.Tensor, iController) -> torch.Tensor:
        h, _, _ = self.self_attn(self.input_layernorm(hidden_states), iController=iController)
        hidden_states = hidden_states + h
        return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))

    def forward_state(self, hidden_states: torch.Tensor, controller, scores, dense: bool) -> torch.Tensor:
        """State-driven decode token of every sequence of ``controller`` (``QuestAttention.forward_state``)."""
        h = self.self_attn.forward_state(self.input_layernorm(hidden_states), controller, scores, dense)
        hidden_states = hidden_states + h
        return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))

    def forward_state_fused(self, h: torch.Tensor, controller, scores, dense: bool, ws: "DecodeWorkspace") -> torch.Tensor:
        """``forward_state`` in 4 launches besides the attention's: RMSNorm + q/k/v projections + RoPE, o_proj + residual,
        RMSNorm + gate/up + SiLU*up, down_proj + residual (csrc/decode_layer.hip; EXTENSION).  A model with a per-head q/k
        norm (Qwen3) takes FIVE: the norm needs a whole head row, which the q/k/v launch spreads over several workgroups,
        so that launch stores q, k, v unrotated and the q/k norm + RoPE launch follows.  ``h`` is the residual stream,
        updated IN PLACE; fp16 or bf16.  An ``InferenceController`` takes the batch-1 launches (``h`` ``[hidden]``), a
        ``BatchedInferenceController`` the n-token ones at every n <= 16 (``h`` ``[n, hidden]``; the weights are read once
        per batch: persist_kernel) -- different kernels, whose results differ in the last bits."""
        a, m = self.self_attn, self.mlp
        launches = _fused_layer_launches(controller)
        freqs = a.rotary(h.device)
        qkv = (h, self.input_layernorm.weight, self.input_layernorm.variance_epsilon, a.q_proj.weight, a.k_proj.weight,
               a.v_proj.weight, ws.q, ws.k, ws.v)
        if a.qk_norm:
            launches.qkv(*qkv)
            qutils.apply_qk_norm_rope_in_place(ws.q, ws.k, 0, *a.qk_norm_args(), rope_scale=a.rope_scale,
                                               rope_theta=a.rope_theta, rope_freqs=freqs, states=controller.step_states)
        elif freqs is None:
            launches.qkv_rope(*qkv, a.head_dim, a.rope_scale, a.rope_theta, controller.step_states)
        else:
            launches.qkv_rope_freqs(*qkv, a.head_dim, freqs[0], freqs[1], controller.step_states)
        if dense:
            attn = qutils.decode_layer_dense_batched(ws.q, ws.k, ws.v, controller, a.layer_idx, out=ws.attn)
        else:
            attn = qutils.decode_layer_batched(ws.q, ws.k, ws.v, controller, a.layer_idx, scores, out=ws.attn)
        launches.gemv_residual(attn, a.o_proj.weight, h)
        launches.mlp_gate_up(h, self.post_attention_layernorm.weight, self.post_attention_layernorm.variance_epsilon,
                             m.gate_proj.weight, m.up_proj.weight, ws.act)
        launches.gemv_residual(ws.act, m.down_proj.weight, h)
        return h


def _fused_layer_launches(controller):
    """The projection launches of the fused decoder layer and of the final norm + lm_head for ``controller``'s kind, by name:
    a ``BatchedInferenceController`` takes the n-token form of each at every n, an ``InferenceController`` the one-token form.
    (Looked up in ``_kernels`` per call, so that a test can wrap the functions there.)"""
    k = _kernels
    if isinstance(controller, qutils.BatchedInferenceController):
        return SimpleNamespace(qkv_rope=k.decode_qkv_rope_batched, qkv_rope_freqs=k.decode_qkv_rope_batched_freqs,
                               qkv=k.decode_qkv_batched, gemv_residual=k.decode_gemv_residual_batched,
                               mlp_gate_up=k.decode_mlp_gate_up_batched, norm_gemv=k.decode_norm_gemv_batched)
    return SimpleNamespace(qkv_rope=k.decode_qkv_rope, qkv_rope_freqs=k.decode_qkv_rope_freqs, qkv=k.decode_qkv,
                           gemv_residual=k.decode_gemv_residual, mlp_gate_up=k.decode_mlp_gate_up, norm_gemv=k.decode_norm_gemv)


def fused_layer_launches_supported(config, n_tokens: int) -> bool:
    """Shapes the fused decoder-layer launches (csrc/decode_layer.hip) serve -- checked BEFORE a decode graph is captured,
    so that a model outside them falls back to the module path (nn.Linear + separate norm / RoPE / activation launches)
    instead of failing inside the capture with QUEST_EUNSUPPORTED: input dimensions a multiple of 8 halves (16-byte
    vectors); the batch-1 kernels stage an input vector of at most 30720 halves in LDS (24576 with the RMSNorm prologue
    of the n-token fallback kernel); RoPE pairs need head_dim % 4 == 0 (batch 1) / % 16 == 0 (n tokens).  o_proj reads
    heads x head_dim inputs, which a config with its own head_dim makes differ from hidden_size; a per-head q/k norm
    needs a head_dim its launch serves (64 / 128 / 256)."""
    hidden, inter = config.hidden_size, config.intermediate_size
    head_dim = rope_mod.head_dim_of(config)
    attn_dim = config.num_attention_heads * head_dim
    if hidden % 8 or inter % 8 or attn_dim % 8 or head_dim % 4:
        return False
    if max(hidden, inter, attn_dim) > 30720:
        return False
    if getattr(config, "qk_norm", False) and head_dim not in (64, 128, 256):
        return False
    if n_tokens > 1 and (head_dim % 16 or hidden > 24576):
        return False
    return True


class DecodeWorkspace:
    """Scratch of the fused decode layer (one set for the whole model: layers run one after the other); ``n`` tokens
    (sequences of a batch) per step."""

    def __init__(self, config: LlamaConfig, dtype, device, n: int = 1):
        d = rope_mod.head_dim_of(config)
        self.q = torch.empty(n, config.num_attention_heads, d, dtype=dtype, device=device)
        self.k = torch.empty(n, config.num_key_value_heads, d, dtype=dtype, device=device)
        self.v = torch.empty(n, config.num_key_value_heads, d, dtype=dtype, device=device)
        self.attn = torch.empty(n, config.num_attention_heads, d, dtype=dtype, device=device)
        self.act = torch.empty((n, config.intermediate_size) if n > 1 else (config.intermediate_size,), dtype=dtype, device=device)
        self.h = torch.empty((n, config.hidden_size) if n > 1 else (config.hidden_size,), dtype=dtype, device=device)


class LlamaModel(nn.Module):
    def __init__(self, config: LlamaConfig, fused: bool = True):
        super().__init__()
        self.config = config
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size)
        self.layers = nn.ModuleList([LlamaDecoderLayer(config, i, fused) for i in range(config.num_hidden_layers)])
        self.norm = LlamaRMSNorm(config.hidden_size, config.rms_norm_eps)
        self._quest_skip_layer = 2            # llama.py:538
        self._quest_max_page_limit = 1 << 20  # llama.py:537
        self._quest_page_budget = None
        self.iController: Optional[qutils.InferenceController] = None

    def forward(self, input_ids: Optional[torch.Tensor] = None, inputs_embeds: Optional[torch.Tensor] = None):
        ctl = self.iController
        assert ctl is not None, "call quest_init() first"
        h = self.embed_tokens(input_ids) if inputs_embeds is None else inputs_embeds
        q_len = h.shape[1]
        ctl.prepare_metadata(q_len)                                   # llama.py:425
        ctl.set_page_budget(self._quest_max_page_limit)               # llama.py:428-430: dense first layers
        ctl.begin_forward(q_len)
        for idx, layer in enumerate(self.layers):
            if idx == self._quest_skip_layer:                         # llama.py:434-439
                ctl.end_forward()
                ctl.set_page_budget(self._quest_page_budget)
                ctl.begin_forward(q_len, updateTensor=False)
            h = layer(h, ctl)
        ctl.end_forward()                                             # llama.py:486
        return self.norm(h)


    def forward_decode(self, h: torch.Tensor, scores: torch.Tensor, controller) -> torch.Tensor:
        """One decode token of every sequence of ``controller`` (``h``: ``[n, 1, hidden]``) with no host-side planning:
        the device-side state advance replaces prepare_metadata / begin_forward / end_forward (capturable, replayable)."""
        qutils.step_advance_batched(controller)
        for idx, layer in enumerate(self.layers):
            h = layer.forward_state(h, controller, scores, dense=idx < self._quest_skip_layer)
        return self.norm(h)

    def forward_decode_fused(self, h: torch.Tensor, scores: torch.Tensor, controller, ws: DecodeWorkspace) -> torch.Tensor:
        """``forward_decode`` with the fused decoder layers; returns the residual stream (``ws.h``: ``[hidden]`` or
        ``[n, hidden]``) BEFORE the final norm (the caller fuses that into its lm_head launch)."""
        qutils.step_advance_batched(controller)
        ws.h.copy_(h.reshape(ws.h.shape))
        for idx, layer in enumerate(self.layers):
            layer.forward_state_fused(ws.h, controller, scores, idx < self._quest_skip_layer, ws)
        return ws.h


class LlamaForCausalLM(nn.Module):
    def __init__(self, config: LlamaConfig, fused: bool = True):
        super().__init__()
        self.config = config
        self.model = LlamaModel(config, fused)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)

    # ------------------------------------------------------------------ Hugging Face checkpoint format
    @classmethod
    def from_pretrained(cls, path: str, device=torch.device("cuda:0"), dtype=torch.float16,
                        fused: bool = True) -> "LlamaForCausalLM":
        """Load a Hugging Face Llama, Mistral or Qwen3 (dense) checkpoint directory -- ``config.json`` + ``model.safetensors`` or the sharded
        ``model-0000x-of-0000y.safetensors`` + ``model.safetensors.index.json`` -- the way the reference does with
        ``LlamaForCausalLM.from_pretrained(...)`` (scripts/bench_textgen.py:53-58, evaluation/*).  Parameter names
        are HF's (``model.layers.N.self_attn.q_proj.weight`` ...), so tensors are copied by name, shard by shard,
        straight to ``device``.  ``dtype``: float16 (default) or bfloat16 -- a bf16 checkpoint loads without a cast, and
        with ``quest_init(dtype=torch.bfloat16)`` its KV cache, metadata and attention stay bf16.  The fused decode-layer
        projections run both types, but a bf16 model's captured step takes them only on request
        (``capture_decode_graph(fused_layers=True)``): by default it keeps the module path, see there."""
        import json
        import os

        from safetensors import safe_open

        with open(os.path.join(path, "config.json")) as f:
            hf = json.load(f)
        cfg = LlamaConfig.from_hf_dict(hf)
        # parameters are created directly in `dtype` on `device` and left uninitialised (every one of them is overwritten
        # from the checkpoint below, or reported missing): no fp32 copy of the model, no random-init pass
        prev = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            with torch.device("meta"):
                model = cls(cfg, fused=fused)
            model = model.to_empty(device=device)
        finally:
            torch.set_default_dtype(prev)
        index = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(index):
            with open(index) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
        else:
            files = ["model.safetensors"]
        params = dict(model.state_dict())
        seen = set()
        with torch.no_grad():
            for fn in files:
                with safe_open(os.path.join(path, fn), framework="pt", device=str(device)) as sf:
                    for name in sf.keys():
                        if name.endswith("rotary_emb.inv_freq"):  # buffer of older HF exports; recomputed by the rope kernel
                            continue
                        if name not in params:
                            raise KeyError(f"{fn}: unexpected tensor {name!r} (not a parameter of this decoder)")
                        t = sf.get_tensor(name)
                        if t.shape != params[name].shape:
                            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != model {tuple(params[name].shape)}")
                        params[name].copy_(t)
                        if t.dtype != params[name].dtype and t.dtype in (torch.bfloat16, torch.float32) \
                                and not bool(torch.isfinite(params[name]).all()):
                            # e.g. a bf16 checkpoint whose values exceed fp16's range
                            raise ValueError(f"{name}: {t.dtype} values overflow {params[name].dtype}. Load the checkpoint "
                                             "in its own type with from_pretrained(dtype=torch.bfloat16) and give "
                                             "quest_init / quest_init_batched the same dtype: the attention kernels "
                                             "run bf16 pools natively.")
                        seen.add(name)
        missing = set(params) - seen
        if missing == {"lm_head.weight"} and hf.get("tie_word_embeddings", False):
            model.lm_head.weight = model.model.embed_tokens.weight
            missing = set()
        if missing:
            raise KeyError(f"checkpoint lacks {sorted(missing)[:5]}{' ...' if len(missing) > 5 else ''}")
        return model

    def save_pretrained(self, path: str, max_shard_bytes: int = 4 << 30) -> None:
        """Write ``config.json`` + safetensors shard(s) in the Hugging Face layout (tensor names = HF's), so that
        ``transformers.LlamaForCausalLM.from_pretrained(path)`` (``MistralForCausalLM`` / ``Qwen3ForCausalLM`` for those
        model types; a config's own ``head_dim`` and Qwen3's q/k norm weights are written back) -- or ``from_pretrained``
        above -- reads it."""
        import json
        import os

        from safetensors.torch import save_file

        os.makedirs(path, exist_ok=True)
        sd = self.state_dict()
        tied = self.lm_head.weight.data_ptr() == self.model.embed_tokens.weight.data_ptr()
        if tied:
            sd.pop("lm_head.weight")
        dt = {torch.float16: "float16", torch.bfloat16: "bfloat16", torch.float32: "float32"}[self.lm_head.weight.dtype]
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config.to_hf_dict(dt, tied), f, indent=1)
        shards, cur, size = [], {}, 0
        for name, t in sd.items():
            nbytes = t.numel() * t.element_size()
            if cur and size + nbytes > max_shard_bytes:
                shards.append(cur)
                cur, size = {}, 0
            cur[name] = t
            size += nbytes
        shards.append(cur)
        if len(shards) == 1:
            save_file({k: v.detach().contiguous().cpu() for k, v in shards[0].items()},
                      os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
            return
        weight_map, total = {}, 0
        for i, shard in enumerate(shards):
            fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
            save_file({k: v.detach().contiguous().cpu() for k, v in shard.items()}, os.path.join(path, fn),
                      metadata={"format": "pt"})
            for k, v in shard.items():
                weight_map[k] = fn
                total += v.numel() * v.element_size()
        with open(os.path.join(path, "model.safetensors.index.json"), "w") as f:
            json.dump({"metadata": {"total_size": total}, "weight_map": weight_map}, f, indent=1)

    def quest_init(self, page_size: int, max_seq_len: int, token_budget: int = 512, dtype=torch.float16,
                   device=torch.device("cuda:0"), kv_layout="NHD", group_selection: bool = False) -> None:
        """llama.py:520-552: build the controller; ``token_budget`` is in TOKENS, the controller's page
        budget is ``token_budget // page_size`` pages (llama.py:536).  ``kv_layout`` (EXTENSION; the reference hard-wires
        NHD, controller.py:38): "NHD", "HND" or this build's row-rotated "NHD_ROT" (same results, faster batched launches).
        ``group_selection`` (EXTENSION, opt-in; GQA models): ONE page selection per kv head, attended by all query heads of
        its group, instead of the reference's selection per query head -- eager, captured and fused-layer steps all follow
        it.  Raises ValueError for a shape the group-selection launch does not serve.  Its effect on a real checkpoint's
        accuracy has not been measured."""
        assert self.model.iController is None, "Can't init Quest Controller twice."
        cfg = self.config
        self.model._quest_page_budget = token_budget // page_size
        self.model.iController = qutils.InferenceController(
            cfg.num_hidden_layers, cfg.num_attention_heads, rope_mod.head_dim_of(cfg), page_size,
            self.model._quest_page_budget, max_seq_len, dtype, device, num_kv_heads=cfg.num_key_value_heads,
            layout=qutils.TensorLayout.parse(kv_layout), group_selection=group_selection)
        self._share_rope_table(device)
        print(f"Quest allocates KV-Cache of {max_seq_len} tokens; token_budget {token_budget} = "
              f"{self.model._quest_page_budget} pages of {page_size}")

    def _share_rope_table(self, device) -> None:
        """llama3 / yarn configs: ONE fp32 frequency table on ``device`` for every layer (kept referenced by the layers
        for as long as a captured graph may use its address)."""
        freqs = rope_mod.device_rope_parameters(self.config, device)
        for layer in self.model.layers:
            layer.self_attn.rope_freqs = freqs

    def quest_clear(self) -> None:
        """llama.py:554-560: release the pages for the next request."""
        assert self.model.iController is not None, "Must quest_init() before quest_clear()."
        self.model.iController.clean_states()
        self._graph = None  # the captured step addressed the finished request's pages (re-capture after prefill)

    def forward(self, input_ids: Optional[torch.Tensor] = None, inputs_embeds: Optional[torch.Tensor] = None):
        h = self.model(input_ids=input_ids, inputs_embeds=inputs_embeds)
        return self.lm_head(h[:, -1:, :])  # decode only needs the last position

    # ------------------------------------------------------------------ one hipGraph per generated token
    def capture_decode_graph(self, fused_layers: Optional[bool] = None, sampler=None) -> None:
        """Capture ONE decode step (all layers + lm_head) and keep it for ``decode_graph_step``.  ``fused_layers``
        (None, the default: on for fp16 models unless ``QUEST_FUSED_LAYER=0``, OFF for bf16 models; True / False: as
        asked, for both types): the decoder layers' projections, norms, RoPE,
        activation and residual adds run as 4 fused HIP launches per layer (csrc/decode_layer.hip; 5 for a model with a
        per-head q/k norm, ``forward_state_fused``) instead of ~14 rocBLAS / PyTorch launches.  bf16 fused layers are
        opt-in: the fused step rounds at other places than the module path (one rounding per launch instead of one per
        module), so its logits differ from the module path's in the last bits, and callers of the default on bf16 models
        rely on the module path; turning the default on for bf16 is a change of its own.  Inside the fused bf16 step the
        attention is what a bf16 controller runs anyway (the two- / three-launch forms; no one-launch layer).  Call after
        the prompt has been processed (any length: while the cache holds fewer pages than the budget the
        sparse layers attend all of them, like the reference's full-attention branch).  The
        graph reads its input from ``self.graph_input`` ``[1, 1, hidden]`` and leaves the logits in
        ``self.graph_logits``; sequence lengths live on the device (EXTENSION).
        ``sampler`` (a ``quest_amd.utils.Sampler`` for one sequence; None, the default: today's graph, launch for launch):
        the captured step ends with the sampling launch (csrc/sampling.hip), which picks the token from the logits at
        position ``seq_len`` of the device state and writes its embedding row into ``self.graph_input`` -- a replay then
        feeds the next one, with no host round trip in between (``generate``)."""
        ctl = self.model.iController
        ctl.set_page_budget(self.model._quest_page_budget)
        self._capture_decode_graph(ctl, fused_layers, sampler)

    def _capture_decode_graph(self, ctl, fused_layers: Optional[bool], sampler=None) -> None:
        """Capture one decode step of every sequence of ``ctl`` (an ``InferenceController`` is the batch of one)."""
        m, n = self.model, ctl.n_seqs
        dev = next(self.parameters()).device
        ctl.enable_device_state()
        ctl.begin_graph_decode(dense_layers=m._quest_skip_layer > 0)
        self.graph_input = torch.zeros(n, 1, self.config.hidden_size, dtype=self.lm_head.weight.dtype, device=dev)
        self._graph_scores = qutils.score_scratch(ctl)
        dtype = self.lm_head.weight.dtype
        if fused_layers is None:
            import os

            fused_layers = dtype == torch.float16 and os.environ.get("QUEST_FUSED_LAYER", "1") != "0"
        fused_layers = (fused_layers and dtype in (torch.float16, torch.bfloat16) and ctl.dtype == dtype
                        and n <= _kernels.MAX_BATCHED_TOKENS and fused_layer_launches_supported(self.config, n))
        self.fused_layers = fused_layers
        if fused_layers:
            # (kept on self: the captured launches hold these buffers' addresses)
            ws = self._graph_ws = DecodeWorkspace(self.config, dtype, dev, n)
            logits = torch.empty(n, 1, self.config.vocab_size, dtype=dtype, device=dev)
            norm_gemv = _fused_layer_launches(ctl).norm_gemv

            def forward():
                hs = m.forward_decode_fused(self.graph_input, self._graph_scores, ctl, ws)
                norm_gemv(hs, m.norm.weight, m.norm.variance_epsilon, self.lm_head.weight, logits)
                return logits
        else:
            def forward():
                return self.lm_head(m.forward_decode(self.graph_input, self._graph_scores, ctl))

        if sampler is None:
            step = forward
        else:
            if sampler.n != n or sampler.vocab_size != self.config.vocab_size:
                raise ValueError(f"the sampler serves {sampler.n} sequences of vocabulary {sampler.vocab_size}, the step "
                                 f"{n} of {self.config.vocab_size}")

            def step():
                out = forward()
                # (the state was advanced at the head of the step: seq_len = the index the sampled token will occupy)
                sampler.sample(out.view(n, -1), states=ctl.step_states, embed=m.embed_tokens.weight,
                               next_input=self.graph_input.view(n, -1))
                return out

        # Warm-up (allocator, rocBLAS workspaces) runs a real step on a dummy input: it advances the device
        # state and folds the dummy key into every sequence's current (max, min) metadata entry.  K/V bytes it wrote
        # are overwritten by the first real token, but the metadata fold is not idempotent -> snapshot the
        # current metadata page(s) of every layer and restore them, then rewind the state.
        seqs = getattr(ctl, "seqs", [ctl])
        pool = seqs[0].metadata_cache.pool  # (one pool for all sequences of a batch)
        pages = torch.tensor([c.metadata_cache.indicies[-1] for c in seqs], device=dev)
        saved = pool.buf[:, pages].clone()
        saved_sampler = sampler.snapshot() if sampler is not None else None  # (the warm-up samples from the dummy step)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.inference_mode():
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        pool.buf[:, pages] = saved
        if sampler is not None:
            sampler.restore(saved_sampler)
        ctl.sync_device_state()
        self._graph = torch.cuda.CUDAGraph()
        with torch.inference_mode(), torch.cuda.graph(self._graph):
            self.graph_logits = step()
        self._graph_epoch = ctl.state_epoch
        self._graph_sampler = sampler

    def decode_graph_step(self, inputs_embeds: Optional[torch.Tensor] = None,
                          input_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Generate one token's logits by replaying the captured step; returns ``self.graph_logits``."""
        if getattr(self, "_graph", None) is None or self._graph_epoch != self.model.iController.state_epoch:
            raise RuntimeError("no decode graph for the current request: call capture_decode_graph() after the "
                               "prompt (quest_clear() / enable_device_state() invalidate a captured graph)")
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        self.graph_input.copy_(inputs_embeds.view(1, 1, -1))
        self._graph.replay()
        self.model.iController.prepare_metadata(1)  # host mirror of the device-side reservation
        return self.graph_logits

    # ------------------------------------------------------------------ batched serving (EXTENSION)
    def quest_init_batched(self, n_seqs: int, page_size: int, max_seq_len: int, token_budget: int = 512,
                           dtype=torch.float16, device=torch.device("cuda:0"), kv_layout="NHD",
                           group_selection: bool = False) -> None:
        """``quest_init`` for ``n_seqs`` sequences decoded together: one shared KV pool and metadata pool
        (``BatchedInferenceController``).  Prompts are processed one sequence at a time with
        ``prefill_sequence``; decode steps then run all sequences in one hipGraph replay.  ``group_selection``: as in
        ``quest_init``."""
        assert self.model.iController is None and getattr(self.model, "bController", None) is None
        cfg = self.config
        self.model._quest_page_budget = token_budget // page_size
        self.model.bController = qutils.BatchedInferenceController(
            n_seqs, cfg.num_hidden_layers, cfg.num_attention_heads, rope_mod.head_dim_of(cfg),
            page_size, self.model._quest_page_budget, max_seq_len, dtype, device,
            num_kv_heads=cfg.num_key_value_heads, layout=qutils.TensorLayout.parse(kv_layout),
            group_selection=group_selection)
        self._share_rope_table(device)

    def prefill_sequence(self, seq: int, input_ids: torch.Tensor) -> torch.Tensor:
        """Run the prompt of sequence ``seq`` (``[1, L]``) through the ordinary single-sequence path over the
        shared pools; returns the logits of its last position."""
        m = self.model
        m.iController = m.bController.seqs[seq]
        try:
            return self.forward(input_ids=input_ids)
        finally:
            m.iController = None

    def capture_decode_graph_batched(self, fused_layers: Optional[bool] = None, sampler=None) -> None:
        """Batched ``capture_decode_graph``: input ``self.graph_input`` ``[n, 1, hidden]``, logits
        ``self.graph_logits`` ``[n, 1, vocab]``.  ``fused_layers`` as in ``capture_decode_graph`` (default on for fp16
        models and n <= 16 unless ``QUEST_FUSED_LAYER=0``, off for bf16 models, which take them with ``fused_layers=True``):
        4 fused launches per layer for the whole batch.  ``sampler`` (for ``n`` sequences) as in ``capture_decode_graph``."""
        self._capture_decode_graph(self.model.bController, fused_layers, sampler)

    def decode_graph_step_batched(self, input_ids: torch.Tensor) -> torch.Tensor:
        """One token for every sequence: ``input_ids`` ``[n]`` -> logits ``[n, 1, vocab]`` (the graph's buffer)."""
        if getattr(self, "_graph", None) is None or self._graph_epoch != self.model.bController.state_epoch:
            raise RuntimeError("no decode graph for the current batch: call capture_decode_graph_batched()")
        self.graph_input.copy_(self.model.embed_tokens(input_ids.view(-1, 1)))
        self._graph.replay()
        self.model.bController.prepare_metadata(1)
        return self.graph_logits

    # ------------------------------------------------------------------ generation with device-side sampling (EXTENSION)
    def _generate(self, ctl, capture, logits: torch.Tensor, prompt_lens, max_new_tokens: int, sampling, eos_token_id,
                  sync_every: int, fused_layers: Optional[bool]):
        """The loop behind ``generate`` / ``generate_batched``: ``logits`` ``[n, vocab]`` of the prompts' last positions."""
        from ..utils.sampling import Sampler, SamplingParams

        n, dev = logits.size(0), logits.device
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        sampler = Sampler(n, self.config.vocab_size, dev, max_tokens=max_new_tokens, eos_token_id=eos_token_id)
        if sampling is None or isinstance(sampling, SamplingParams):
            sampling = [sampling or SamplingParams()] * n
        if len(sampling) != n:
            raise ValueError(f"{len(sampling)} sampling parameter sets for {n} sequences")
        for i, params in enumerate(sampling):
            sampler.set_params(i, params)
        # the first token: an eager call of the same entry on the prefill logits (it will sit at index prompt length)
        first = torch.empty(n, 1, self.config.hidden_size, dtype=self.lm_head.weight.dtype, device=dev)
        sampler.sample(logits, positions=torch.tensor(list(prompt_lens), dtype=torch.int32, device=dev),
                       embed=self.model.embed_tokens.weight, next_input=first.view(n, -1))
        if max_new_tokens > 1 and not (sampler.eos_ids is not None and sampler.all_finished()):
            capture(fused_layers=fused_layers, sampler=sampler)
            with torch.inference_mode():
                self.graph_input.copy_(first)
            for t in range(1, max_new_tokens):
                self._graph.replay()       # the step and its token choice; nothing is copied to the host
                ctl.prepare_metadata(1)    # host mirror of the device-side reservation
                if sampler.eos_ids is not None and sync_every > 0 and t % sync_every == 0 and sampler.all_finished():
                    break
        self.last_sampler = sampler
        return sampler.sequences()

    def generate(self, input_ids: torch.Tensor, max_new_tokens: int, sampling=None, eos_token_id=None, sync_every: int = 16,
                 fused_layers: Optional[bool] = None) -> torch.Tensor:
        """Generate up to ``max_new_tokens`` tokens after the prompt ``input_ids`` ``[1, L]`` (after ``quest_init``, on an
        empty cache: ``quest_clear()`` between requests) and return them (int64, CPU), ending with the eos id when one was
        reached.  ``sampling``: a ``quest_amd.utils.SamplingParams`` (None: greedy); ``eos_token_id``: an id or up to 8.
        The prompt runs through the ordinary forward; the first token is an eager call of the sampling launch on its logits;
        the rest are replays of ONE captured step that ends with the sampling launch and feeds itself (``sampler`` of
        ``capture_decode_graph``) -- no device-to-host copy between replays; the finished flag is read every ``sync_every``
        steps to stop early.  ``fused_layers`` as in ``capture_decode_graph``."""
        with torch.inference_mode():
            logits = self(input_ids=input_ids)
        return self._generate(self.model.iController, self.capture_decode_graph, logits.view(1, -1), [input_ids.size(1)],
                              max_new_tokens, sampling, eos_token_id, sync_every, fused_layers)[0]

    def generate_batched(self, prompts, max_new_tokens: int, sampling=None, eos_token_id=None, sync_every: int = 16,
                         fused_layers: Optional[bool] = None):
        """``generate`` for the sequences of ``quest_init_batched``: ``prompts`` = one ``[1, L_i]`` tensor per sequence,
        ``sampling`` one ``SamplingParams`` for all or a list of one per sequence.  Prompts are prefilled one by one
        (``prefill_sequence``), the decode steps run all sequences per replay.  A finished sequence keeps stepping with the
        pad id until all are finished (seen at the next flag check) or ``max_new_tokens`` is reached; the returned list
        holds each sequence's tokens, ending with its eos id when it reached one."""
        ctl = self.model.bController
        if len(prompts) != ctl.n_seqs:
            raise ValueError(f"{len(prompts)} prompts for {ctl.n_seqs} sequences")
        with torch.inference_mode():
            logits = torch.cat([self.prefill_sequence(i, p).view(1, -1) for i, p in enumerate(prompts)])
        return self._generate(ctl, self.capture_decode_graph_batched, logits, [p.size(1) for p in prompts], max_new_tokens,
                              sampling, eos_token_id, sync_every, fused_layers)
