"""A plain-torch restatement of the decoder with Quest's sparse decode, on the CPU, for the model-level tests.

It imports nothing of ``quest_amd`` and nothing of ``oracle``: it is the independent side of
tests/test_gpu_model_sparse_reference.py, made trustworthy by tests/test_quest_model_ref_host.py (against transformers
in float64 and against the oracle's estimate / top-k).

Arithmetic: embedding, RMSNorm, q/k/v projections, Qwen3's per-head q/k RMSNorm before RoPE, half-split RoPE (default
and linear, free theta), GQA causal attention, SwiGLU, final norm, lm_head (tied where the state_dict has none).

Quest's decode rule, from the reference's sources as SURVEY.md cites them (llama.py:428-439, controller.py:112 / :137-142,
QuestAttention.py:123-157, the estimate kernel's sum over channels):
  * layers below ``skip_layers`` (2) attend everything;
  * in a later layer, with P pages holding the cache INCLUDING the new token and a budget of B pages: P <= B attends
    everything; otherwise the first P - 1 pages are scored per query head with sum_d max(q_d * max_d, q_d * min_d) over
    that kv head's per-page channel extrema of K (after RoPE), the B - 1 best are attended plus the last page, which is
    never scored.

``dtype`` float64 is the reference.  float16 / bfloat16 is the yardstick: the same code with weights, activations and
caches in that type.  ``acc_dtype`` is the type of what low-precision pipelines keep wider -- the RMSNorm statistics,
the softmax and the rotary table: float64 for the reference, float32 for a yardstick (transformers' convention).
transformers keeps those three in float32 even in a ``.double()`` model, which is why the host test compares it with
``dtype=float64, acc_dtype=float32``.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch


class SparseLayer(NamedTuple):
    scores: torch.Tensor  # [Hq, P - 1] page scores in the model's dtype
    own: torch.Tensor     # [Hq, B - 1] logical pages of its own top-k
    pages: torch.Tensor   # [Hq, B - 1] logical pages attended besides the last one (``forced`` or ``own``)
    n_pages: int          # P


def _rope_kind(scaling: Optional[dict]):
    if not scaling:
        return "default", 1.0
    kind = scaling.get("rope_type", scaling.get("type")) or "default"
    if kind not in ("default", "linear"):
        raise ValueError(f"rope type {kind!r}: the restatement covers default and linear RoPE")
    return kind, float(scaling["factor"]) if kind == "linear" else 1.0


class QuestModelRef:
    def __init__(self, state_dict: Dict[str, torch.Tensor], config, page_size: int = 16, page_budget: int = 4,
                 dtype=torch.float64, acc_dtype=None, skip_layers: int = 2):
        self.dtype = dtype
        self.acc = acc_dtype or (torch.float64 if dtype == torch.float64 else torch.float32)
        self.w = {k: v.detach().to("cpu").to(dtype) for k, v in state_dict.items()}
        if "lm_head.weight" not in self.w:  # tied embeddings
            self.w["lm_head.weight"] = self.w["model.embed_tokens.weight"]
        self.layers = int(config.num_hidden_layers)
        self.hq = int(config.num_attention_heads)
        self.hkv = int(getattr(config, "num_key_value_heads", None) or self.hq)
        self.d = int(getattr(config, "head_dim", None) or config.hidden_size // self.hq)
        self.eps = float(config.rms_norm_eps)
        self.qk_norm = bool(getattr(config, "qk_norm", False))
        self.theta = float(getattr(config, "rope_theta", 1e4))
        _, self.rope_factor = _rope_kind(getattr(config, "rope_scaling", None))
        self.page, self.budget, self.skip = int(page_size), int(page_budget), int(skip_layers)
        self.kvh = torch.arange(self.hq) // (self.hq // self.hkv)  # kv head of every query head
        self.k = [torch.empty(0, self.hkv, self.d, dtype=dtype) for _ in range(self.layers)]  # after RoPE
        self.v = [torch.empty(0, self.hkv, self.d, dtype=dtype) for _ in range(self.layers)]

    # ------------------------------------------------------------------ arithmetic
    @property
    def seqlen(self) -> int:
        return self.k[0].shape[0]

    def _norm(self, x, weight):
        xa = x.to(self.acc)
        xa = xa * torch.rsqrt(xa.pow(2).mean(-1, keepdim=True) + self.eps)
        return weight * xa.to(x.dtype)

    def _rope(self, x, pos0: int):
        """x ``[N, H, D]``, row i at position pos0 + i; half-split (rotate-half) form."""
        n, _, d = x.shape
        inv_freq = 1.0 / (self.theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(self.acc) / d))
        if self.rope_factor != 1.0:
            inv_freq = inv_freq / self.rope_factor
        ang = torch.arange(pos0, pos0 + n).to(self.acc)[:, None] * inv_freq[None, :]
        emb = torch.cat([ang, ang], -1)
        cos, sin = emb.cos().to(x.dtype)[:, None], emb.sin().to(x.dtype)[:, None]
        rot = torch.cat([-x[..., d // 2:], x[..., : d // 2]], -1)
        return x * cos + rot * sin

    def _softmax(self, s):
        return torch.softmax(s, -1, dtype=self.acc).to(self.dtype)

    def _qkv(self, layer: int, x, pos0: int):
        p, n = f"model.layers.{layer}.self_attn.", x.shape[0]
        q = (x @ self.w[p + "q_proj.weight"].t()).view(n, self.hq, self.d)
        k = (x @ self.w[p + "k_proj.weight"].t()).view(n, self.hkv, self.d)
        v = (x @ self.w[p + "v_proj.weight"].t()).view(n, self.hkv, self.d)
        if self.qk_norm:
            q, k = self._norm(q, self.w[p + "q_norm.weight"]), self._norm(k, self.w[p + "k_norm.weight"])
        q, k = self._rope(q, pos0), self._rope(k, pos0)
        self.k[layer] = torch.cat([self.k[layer], k])
        self.v[layer] = torch.cat([self.v[layer], v])
        return q

    def _mlp(self, layer: int, x):
        p = f"model.layers.{layer}.mlp."
        gate = torch.nn.functional.silu(x @ self.w[p + "gate_proj.weight"].t())
        return (gate * (x @ self.w[p + "up_proj.weight"].t())) @ self.w[p + "down_proj.weight"].t()

    def _layer(self, layer: int, h, attention):
        p = f"model.layers.{layer}."
        a = attention(self._norm(h, self.w[p + "input_layernorm.weight"]))
        h = h + a.reshape(h.shape[0], -1) @ self.w[p + "self_attn.o_proj.weight"].t()
        return h + self._mlp(layer, self._norm(h, self.w[p + "post_attention_layernorm.weight"]))

    def _logits(self, h):
        return self._norm(h, self.w["model.norm.weight"]) @ self.w["lm_head.weight"].t()

    # ------------------------------------------------------------------ prefill: causal attention over the prompt
    def prefill(self, ids) -> torch.Tensor:
        """The prompt ``[N]`` into an empty cache; logits of all positions ``[N, vocab]``."""
        assert self.seqlen == 0, "prefill starts a sequence"
        ids = torch.as_tensor(ids).reshape(-1).cpu()
        n = ids.numel()
        h = self.w["model.embed_tokens.weight"][ids]
        future = torch.ones(n, n, dtype=torch.bool).triu(1)

        def attention(layer):
            def run(x):
                q = self._qkv(layer, x, 0)
                k, v = self.k[layer][:, self.kvh], self.v[layer][:, self.kvh]  # [N, Hq, D]
                s = torch.einsum("nhd,thd->hnt", q, k) * self.d ** -0.5
                p = self._softmax(s.masked_fill(future, float("-inf")))
                return torch.einsum("hnt,thd->nhd", p, v)
            return run

        for layer in range(self.layers):
            h = self._layer(layer, h, attention(layer))
        return self._logits(h)

    # ------------------------------------------------------------------ decode: Quest's rule
    def page_scores(self, layer: int, q) -> torch.Tensor:
        """``[Hq, P - 1]``: the estimate of every page of ``layer``'s cache but the last, for the query ``q`` ``[Hq, D]``."""
        full = (-(-self.k[layer].shape[0] // self.page) - 1) * self.page
        pages = self.k[layer][:full].view(-1, self.page, self.hkv, self.d)
        mx, mn = pages.amax(1)[:, self.kvh], pages.amin(1)[:, self.kvh]  # [P - 1, Hq, D]
        return torch.maximum(q[None] * mx, q[None] * mn).sum(-1).t().contiguous()

    def top_pages(self, scores) -> torch.Tensor:
        """``[Hq, B - 1]``: the B - 1 best-scored logical pages of every head."""
        return scores.to(torch.float64).topk(self.budget - 1, dim=-1).indices

    def _attend(self, layer: int, q, tokens):
        """q ``[Hq, D]`` over the cache rows ``tokens`` ``[Hq, n]`` of each head's kv head."""
        k, v = self.k[layer][tokens, self.kvh[:, None]], self.v[layer][tokens, self.kvh[:, None]]  # [Hq, n, D]
        p = self._softmax(torch.einsum("hd,hnd->hn", q, k) * self.d ** -0.5)
        return torch.einsum("hn,hnd->hd", p, v)[None]

    def step(self, token: int, forced: Optional[Dict[int, torch.Tensor]] = None):
        """One decode token.  Returns ``(logits [vocab], {layer: SparseLayer})`` with an entry for every layer that took
        the sparse branch.  ``forced``: layer -> ``[Hq, B - 1]`` logical pages to attend instead of the layer's own top-k."""
        assert self.seqlen > 0, "prefill first"
        pos = self.seqlen
        h = self.w["model.embed_tokens.weight"][torch.tensor([int(token)])]
        info: Dict[int, SparseLayer] = {}
        n_tok = pos + 1
        n_pages = -(-n_tok // self.page)
        last = torch.arange((n_pages - 1) * self.page, n_tok)[None].expand(self.hq, -1)

        def attention(layer):
            def run(x):
                q = self._qkv(layer, x, pos)[0]
                if layer < self.skip or n_pages <= self.budget:
                    return self._attend(layer, q, torch.arange(n_tok)[None].expand(self.hq, -1))
                scores = self.page_scores(layer, q)
                assert scores.shape == (self.hq, n_pages - 1)
                own = self.top_pages(scores)
                pages = own if forced is None or layer not in forced else torch.as_tensor(forced[layer]).long().cpu()
                assert pages.shape == own.shape and int(pages.min()) >= 0 and int(pages.max()) <= n_pages - 2
                info[layer] = SparseLayer(scores, own, pages, n_pages)
                tokens = (pages[:, :, None] * self.page + torch.arange(self.page)).reshape(self.hq, -1)
                return self._attend(layer, q, torch.cat([tokens, last], 1))
            return run

        for layer in range(self.layers):
            h = self._layer(layer, h, attention(layer))
        return self._logits(h)[0], info
