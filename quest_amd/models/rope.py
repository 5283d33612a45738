"""Rotary-embedding parameters of a Llama config: which form the kernels take and, for the scaled types, the frequency
table.

Default and linear RoPE run the kernels' in-kernel formula ``(1 / rope_scale) * rope_theta^(-2i / D)``; the model types
added after Llama (``mistral``, ``qwen3``: 32K-128K contexts with unscaled RoPE) take the table for default RoPE too --
the formula's exp2f frequency differs from transformers' ``1 / theta^(2i / D)`` by up to 8e-7 relative and by an fp32 ulp
of the highest frequencies, which times the position is an angle error of up to 0.008 rad at 131071 (2.4e-4 at 4096),
where the table's angle equals transformers' bit for bit.  (Llama configs keep the formula for default RoPE, drift
included: their behaviour is unchanged.)  The ``llama3``
(Llama-3.1 / 3.2) and ``yarn`` (YaRN, e.g. NousResearch Yarn-Llama-2-7b-128k) scalings go through the kernels' table
form: ``inv_freq`` (``D/2`` fp32) and ``attention_factor``, computed here with the fp32 torch expressions of Hugging
Face's ``modeling_rope_utils`` (``_compute_llama3_parameters`` / ``_compute_yarn_parameters``), so that the frequencies
-- and with them the kernels' sin/cos arguments ``pos * inv_freq[i]`` -- equal transformers' bit for bit.  No import of
transformers.  Every tensor is created on the CPU explicitly: ``from_pretrained`` builds the model under
``torch.device("meta")`` with an fp16 default dtype.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

TABLE_TYPES = ("llama3", "yarn")
_LLAMA3_KEYS = ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings")


def rope_type(scaling: Optional[dict]) -> str:
    """``"default"``, ``"linear"``, ``"llama3"`` or ``"yarn"`` for a transformers-4 ``rope_scaling`` dict (``type`` or
    ``rope_type``; ``None`` = default); ``ValueError`` for anything else or a dict missing what its type needs."""
    if scaling is None:
        return "default"
    kind = scaling.get("rope_type", scaling.get("type"))
    if kind in (None, "default"):
        kind = "default"
    elif kind not in ("linear",) + TABLE_TYPES:
        raise ValueError(f"Unknown RoPE scaling type {scaling}")
    if float(scaling.get("partial_rotary_factor", 1.0)) != 1.0:
        raise ValueError(f"partial rotary embeddings are not supported: {scaling}")
    if kind in ("linear", "yarn") and scaling.get("factor") is None:
        raise ValueError(f"RoPE scaling {kind!r} needs a 'factor': {scaling}")
    if kind == "llama3":
        missing = [k for k in _LLAMA3_KEYS if scaling.get(k) is None]
        if missing:
            raise ValueError(f"RoPE scaling 'llama3' needs {missing}: {scaling}")
    return kind


def head_dim_of(config) -> int:
    """The head dimension of a config: its ``head_dim`` field where it has one that is set (Qwen3, Mistral-Nemo: not
    ``hidden_size / num_attention_heads``), else ``hidden_size // num_attention_heads``."""
    return int(getattr(config, "head_dim", None) or config.hidden_size // config.num_attention_heads)


def takes_table(config) -> bool:
    """Whether the config's RoPE runs through the kernels' frequency-table form (else: the in-kernel formula)."""
    kind = rope_type(getattr(config, "rope_scaling", None))
    return kind in TABLE_TYPES or (kind == "default" and getattr(config, "model_type", "llama") != "llama")


def rope_parameters(config) -> Optional[Tuple[torch.Tensor, float]]:
    """``(inv_freq, attention_factor)`` of a config whose RoPE takes the kernels' table form (``inv_freq``: CPU fp32
    ``[D/2]``, D = ``head_dim_of(config)``), ``None`` where the in-kernel formula runs (``takes_table``: linear RoPE, and default RoPE of Llama configs)."""
    scaling = getattr(config, "rope_scaling", None)
    kind = rope_type(scaling)
    if not takes_table(config):
        return None
    base = float(getattr(config, "rope_theta", 1e4))
    dim = head_dim_of(config)
    if kind == "default":  # modeling_rope_utils' default: the unscaled frequencies, as transformers computes them
        return 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.int64, device="cpu").to(dtype=torch.float) / dim)), 1.0
    if kind == "llama3":
        return _llama3(scaling, base, dim), 1.0
    orig = scaling.get("original_max_position_embeddings") or config.max_position_embeddings
    return _yarn(scaling, base, dim, orig)


def _llama3(sc: dict, base: float, dim: int) -> torch.Tensor:
    # modeling_rope_utils._compute_llama3_parameters
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.int64, device="cpu").to(dtype=torch.float) / dim))
    factor, low_freq_factor, high_freq_factor = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"]
    old_context_len = sc["original_max_position_embeddings"]
    low_freq_wavelen = old_context_len / low_freq_factor
    high_freq_wavelen = old_context_len / high_freq_factor
    wavelen = 2 * math.pi / inv_freq
    inv_freq_llama = torch.where(wavelen > low_freq_wavelen, inv_freq / factor, inv_freq)
    smooth_factor = (old_context_len / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor)
    smoothed_inv_freq = (1 - smooth_factor) * inv_freq_llama / factor + smooth_factor * inv_freq_llama
    is_medium_freq = ~(wavelen < high_freq_wavelen) * ~(wavelen > low_freq_wavelen)
    return torch.where(is_medium_freq, smoothed_inv_freq, inv_freq_llama)


def _yarn(sc: dict, base: float, dim: int, orig: int) -> Tuple[torch.Tensor, float]:
    # modeling_rope_utils._compute_yarn_parameters (Nous's "finetuned" key plays no part there either)
    factor = sc["factor"]
    attention_factor = sc.get("attention_factor")
    mscale, mscale_all_dim = sc.get("mscale"), sc.get("mscale_all_dim")

    def get_mscale(scale, m=1):
        return 1.0 if scale <= 1 else 0.1 * m * math.log(scale) + 1.0

    if attention_factor is None:
        if mscale and mscale_all_dim:
            attention_factor = float(get_mscale(factor, mscale) / get_mscale(factor, mscale_all_dim))
        else:
            attention_factor = get_mscale(factor)
    beta_fast = sc.get("beta_fast") or 32
    beta_slow = sc.get("beta_slow") or 1

    def correction_dim(num_rotations):
        return (dim * math.log(orig / (num_rotations * 2 * math.pi))) / (2 * math.log(base))

    low, high = correction_dim(beta_fast), correction_dim(beta_slow)
    if sc.get("truncate", True):
        low, high = math.floor(low), math.ceil(high)
    low, high = max(low, 0), min(high, dim - 1)
    if low == high:
        high += 0.001  # as transformers: no singularity
    ramp = torch.clamp((torch.arange(dim // 2, dtype=torch.float32, device="cpu") - low) / (high - low), 0, 1)
    pos_freqs = base ** (torch.arange(0, dim, 2, device="cpu").to(dtype=torch.float) / dim)
    inv_freq_extrapolation = 1.0 / pos_freqs
    inv_freq_interpolation = 1.0 / (factor * pos_freqs)
    extrapolation_factor = 1 - ramp.to(dtype=torch.float)
    inv_freq = inv_freq_interpolation * (1 - extrapolation_factor) + inv_freq_extrapolation * extrapolation_factor
    return inv_freq, float(attention_factor)


def device_rope_parameters(config, device) -> Optional[Tuple[torch.Tensor, float]]:
    """``rope_parameters`` with the table on ``device`` (fp32, contiguous): the ``rope_freqs`` argument of the
    ``quest_amd.utils`` launches.  A captured graph holds the table's address: keep the tuple referenced."""
    p = rope_parameters(config)
    if p is None:
        return None
    return p[0].to(device=device, dtype=torch.float32).contiguous(), p[1]
