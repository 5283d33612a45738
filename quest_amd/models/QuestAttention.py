"""Attention module that runs Quest's query-aware sparse decode on MI355X.

Module API of the reference kept (quest/models/QuestAttention.py:15-181): same constructor
``QuestAttention(config, layer_idx)``, same parameter names (``q_proj``/``k_proj``/``v_proj``/``o_proj``, so
HF checkpoints load unchanged), same ``forward(hidden_states, ..., iController)`` returning
``(attn_output, None, past_key_value)``.  ``config`` only needs the ``LlamaConfig`` attributes read
below, so the module has no import-time dependency on transformers.

Per decode token the reference issues RoPE, append, estimate, top-k, attention (+merge) as separate
launches (QuestAttention.py:99-157); here append+estimate and top-k+attention are single launches
(``quest_amd.utils.decode_append_estimate`` / ``decode_topk_sparse_attn``), bit-identical to the pairs.
The projections stay ``nn.Linear`` (rocBLAS/hipBLASLt GEMV) -- they are not part of this path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn

from .. import utils as qutils
from . import rope as qrope


class QuestAttention(nn.Module):
    def __init__(self, config, layer_idx: int, fused: bool = True):
        super().__init__()
        self.layer_idx = layer_idx
        self.config = config
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        # the config's own head_dim where it has one (Qwen3, Mistral-Nemo: heads x head_dim != hidden_size)
        self.head_dim = qrope.head_dim_of(config)
        self.num_key_value_heads = getattr(config, "num_key_value_heads", self.num_heads)
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.max_position_embeddings = getattr(config, "max_position_embeddings", None)
        self.fused = fused
        if getattr(config, "head_dim", None) is None and self.head_dim * self.num_heads != self.hidden_size:
            raise ValueError(f"hidden_size must be divisible by num_heads (got `hidden_size`: {self.hidden_size}"
                             f" and `num_heads`: {self.num_heads}).")
        self.q_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=False)
        self.k_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=False)
        self.v_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=False)
        self.o_proj = nn.Linear(self.num_heads * self.head_dim, self.hidden_size, bias=False)
        # Qwen3: RMSNorm over each head's q and k vector before RoPE (weights [head_dim], shared by the heads; HF names
        # self_attn.q_norm.weight / k_norm.weight).  Never run as modules: the fused norm + RoPE launch reads the weights.
        self.qk_norm = bool(getattr(config, "qk_norm", False))
        if self.qk_norm:
            from .llama import LlamaRMSNorm

            if self.head_dim not in (64, 128, 256):  # the norm has no other implementation to fall back to
                raise ValueError(f"head_dim = {self.head_dim}: the per-head q/k norm + RoPE launch serves head_dim 64, 128 "
                                 "and 256")

            self.q_norm = LlamaRMSNorm(self.head_dim, config.rms_norm_eps)
            self.k_norm = LlamaRMSNorm(self.head_dim, config.rms_norm_eps)
        # rope: default theta 1e4.  Default and linear position interpolation run the kernels' formula, as in the
        # reference kernel path (QuestAttention.py:40-51); llama3 and yarn scaling -- and the default RoPE of the model
        # types after Llama -- the kernels' frequency table (models/rope.py), held in `rope_freqs` = (device inv_freq, attention_factor) -- NOT a buffer: it must survive
        # the meta-device construction of from_pretrained, stay out of the state_dict and stay fp32 under .half()
        scaling = getattr(config, "rope_scaling", None)
        kind = qrope.rope_type(scaling)
        self.rope_scale = float(scaling["factor"]) if kind == "linear" else 1.0
        self.rope_theta = float(getattr(config, "rope_theta", 1e4))
        self.rope_table = qrope.takes_table(config)
        self.rope_freqs = None  # set by LlamaForCausalLM.quest_init* (one table for all layers), else on first use

    def rotary(self, device):
        """The ``rope_freqs`` argument of the ``quest_amd.utils`` launches: None (formula) or the frequency table on
        ``device``, materialised on first use."""
        if self.rope_table and (self.rope_freqs is None or self.rope_freqs[0].device != device):
            self.rope_freqs = qrope.device_rope_parameters(self.config, device)
        return self.rope_freqs

    def qk_norm_args(self):
        """The ``qk_norm`` argument of the ``quest_amd.utils`` launches: None or (q weight, k weight, eps)."""
        if not self.qk_norm:
            return None
        return self.q_norm.weight, self.k_norm.weight, self.q_norm.variance_epsilon

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.LongTensor] = None, past_key_value: Optional[Tuple[torch.Tensor]] = None,
                output_attentions: bool = False, use_cache: bool = False,
                iController: Optional[qutils.InferenceController] = None,
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[Tuple[torch.Tensor]]]:
        bsz, q_len, _ = hidden_states.size()
        assert bsz == 1, "QuestAttention only supports batch size 1."
        assert iController is not None, "QuestAttention requires an InferenceController."
        nvtx = torch.cuda.nvtx  # range names of the reference (roctx on ROCm)

        nvtx.range_push("qkv_proj")
        q = self.q_proj(hidden_states).view(q_len, self.num_heads, self.head_dim)
        k = self.k_proj(hidden_states).view(q_len, self.num_key_value_heads, self.head_dim)
        v = self.v_proj(hidden_states).view(q_len, self.num_key_value_heads, self.head_dim)
        nvtx.range_pop()

        nvtx.range_push("RoPE")
        if self.qk_norm:
            qutils.apply_qk_norm_rope_in_place(q, k, iController.kv_cache.seqlen - q_len, *self.qk_norm_args(),
                                               rope_scale=self.rope_scale, rope_theta=self.rope_theta,
                                               rope_freqs=self.rotary(q.device))
        else:
            qutils.apply_rope_in_place(q, k, iController.kv_cache.seqlen - q_len, rope_scale=self.rope_scale,
                                       rope_theta=self.rope_theta, rope_freqs=self.rotary(q.device))
        nvtx.range_pop()

        if q_len > 1:
            nvtx.range_push("append_kv")
            qutils.append_kv(k, v, iController, self.layer_idx)
            nvtx.range_pop()
            nvtx.range_push("prefill_attn")
            attn = qutils.prefill_forward(q, iController, self.layer_idx)
            nvtx.range_pop()
        elif not iController.need_estimate():
            # budget covers the whole cache (or a layer the model keeps dense): plain paged decode
            nvtx.range_push("append_kv")
            qutils.append_kv(k, v, iController, self.layer_idx)
            nvtx.range_pop()
            nvtx.range_push("full_attn")
            attn = qutils.decode_sparse_attn(q, iController, self.layer_idx, iController.kv_indices_without_last)
            nvtx.range_pop()
        elif iController.group_selection:
            # opt-in group-shared selection with the existing operators: key-max over the group, top-k on the kv heads'
            # rows, attention with every row repeated for its group (the same pages as the group-selection launch)
            nvtx.range_push("append_kv+estimate")
            if self.fused:
                scores = qutils.decode_append_estimate(q, k, v, iController, self.layer_idx)
            else:
                qutils.append_kv(k, v, iController, self.layer_idx)
                scores = qutils.decode_estimate(q, iController, self.layer_idx)
            nvtx.range_pop()
            nvtx.range_push("group_topk")
            pages = qutils.decode_group_topk(scores, iController)
            nvtx.range_pop()
            nvtx.range_push("approx_attn")
            attn = qutils.decode_sparse_attn(q, iController, self.layer_idx, pages)
            nvtx.range_pop()
        elif self.fused:
            nvtx.range_push("append_kv+estimate")
            scores = qutils.decode_append_estimate(q, k, v, iController, self.layer_idx)
            nvtx.range_pop()
            nvtx.range_push("topk+approx_attn")
            # the selected page ids stay inside the kernel (nothing downstream reads topk_dindices_buffer)
            attn = qutils.decode_topk_sparse_attn(q, scores, iController, self.layer_idx, write_topk=False)
            nvtx.range_pop()
        else:
            nvtx.range_push("append_kv")
            qutils.append_kv(k, v, iController, self.layer_idx)
            nvtx.range_pop()
            nvtx.range_push("estimate")
            scores = qutils.decode_estimate(q, iController, self.layer_idx)
            nvtx.range_pop()
            nvtx.range_push("topk")
            qutils.decode_topk(scores, iController)
            nvtx.range_pop()
            nvtx.range_push("approx_attn")
            attn = qutils.decode_sparse_attn(q, iController, self.layer_idx, iController.topk_dindices_buffer)
            nvtx.range_pop()

        attn = attn.unsqueeze(0)
        if attn.size() != (bsz, q_len, self.num_heads, self.head_dim):
            raise ValueError(f"`attn_output` should be of size {(bsz, q_len, self.num_heads, self.head_dim)}, but is"
                             f" {attn.size()}")
        nvtx.range_push("o_proj")
        out = self.o_proj(attn.reshape(bsz, q_len, self.num_heads * self.head_dim))
        nvtx.range_pop()
        return out, None, past_key_value

    def forward_state(self, hidden_states: torch.Tensor, controller, scores: torch.Tensor, dense: bool) -> torch.Tensor:
        """Decode-token forward whose every length comes from the controller's device-resident step state
        (``enable_device_state`` + ``begin_graph_decode(dense_layers=True)``), so a whole model step can be
        captured in one hipGraph and replayed as the sequences grow.  ``hidden_states`` is ``[n, 1, hidden]``, one decode
        token per sequence of ``controller`` -- a ``BatchedInferenceController`` (shared pools, every op ONE launch for
        the batch) or an ``InferenceController``, the batch of one.  ``dense``: full-KV layer (the model's first layers)
        vs Quest sparse layer.  EXTENSION: the reference module asserts batch size 1 and plans every token on the host."""
        n, q_len, _ = hidden_states.size()
        assert q_len == 1 and n == controller.n_seqs
        q = self.q_proj(hidden_states).view(n, self.num_heads, self.head_dim)
        k = self.k_proj(hidden_states).view(n, self.num_key_value_heads, self.head_dim)
        v = self.v_proj(hidden_states).view(n, self.num_key_value_heads, self.head_dim)
        if dense:
            attn = qutils.decode_layer_dense_batched(q, k, v, controller, self.layer_idx, self.rope_scale,
                                                     self.rope_theta, apply_rope=True, rope_freqs=self.rotary(q.device),
                                                     qk_norm=self.qk_norm_args())
        else:
            attn = qutils.decode_layer_batched(q, k, v, controller, self.layer_idx, scores, self.rope_scale,
                                               self.rope_theta, apply_rope=True, rope_freqs=self.rotary(q.device),
                                               qk_norm=self.qk_norm_args())
        return self.o_proj(attn.reshape(n, 1, self.num_heads * self.head_dim))
