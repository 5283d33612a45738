#!/usr/bin/env python3
"""Per-head q/k RMSNorm + RoPE fixtures from Hugging Face transformers: the oracle of the fused norm + RoPE launch
(csrc/rope_norm.hip qk_norm_rope_kernel).

Per config of tests/_qk_norm.py: ``inv_freq`` and ``attention_factor`` from ``ROPE_INIT_FUNCTIONS`` (the default type:
``Qwen3RotaryEmbedding``'s own), and q / k passed through ``Qwen3RMSNorm`` (random weights) and then
``Qwen3RotaryEmbedding`` + ``apply_rotary_pos_emb``, everything in fp32 (inputs: seeded fp16 values, for the bf16 variant
restricted to bf16-representable ones), at the (past, n) grid -- the last row at position 131071.  Only the outputs are
stored, in fp32: they also referee the bf16 launch, whose bar is finer than an fp16 rounding.

    python tests/golden/make_qk_norm_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS  # noqa: E402
from transformers.models.qwen3.configuration_qwen3 import Qwen3Config  # noqa: E402
from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, Qwen3RotaryEmbedding, apply_rotary_pos_emb  # noqa: E402

from _qk_norm import CASES, CONFIGS, DTYPES, EPS, inputs  # noqa: E402


def hf_config(d, hq, hkv, max_pos, theta, scaling):
    params = dict(scaling) if scaling else {"rope_type": "default"}
    params["rope_theta"] = theta
    return Qwen3Config(hidden_size=640, head_dim=d, num_attention_heads=hq, num_key_value_heads=hkv,
                       max_position_embeddings=max_pos, rms_norm_eps=EPS, rope_parameters=params)


def main():
    out = {}
    for ci, (name, (d, hq, hkv, max_pos, theta, scaling)) in enumerate(CONFIGS.items()):
        cfg = hf_config(d, hq, hkv, max_pos, theta, scaling)
        rot = Qwen3RotaryEmbedding(cfg)
        assert rot.inv_freq.dtype == torch.float32 and rot.inv_freq.numel() == d // 2
        kind = cfg.rope_parameters["rope_type"]
        if kind != "default":
            inv_freq, factor = ROPE_INIT_FUNCTIONS[kind](cfg, torch.device("cpu"))
            assert torch.equal(inv_freq, rot.inv_freq) and factor == rot.attention_scaling
        out[f"{name}_inv_freq"] = rot.inv_freq.numpy().astype(np.float32)
        out[f"{name}_attention_factor"] = np.array(rot.attention_scaling, np.float64)
        for i, (past, n) in enumerate(CASES):
            for dt in DTYPES:
                q, k, wq, wk = (torch.from_numpy(a).float() for a in inputs(ci, i, dt))
                qn, kn = Qwen3RMSNorm(d, eps=EPS), Qwen3RMSNorm(d, eps=EPS)
                qn.weight.data.copy_(wq)
                kn.weight.data.copy_(wk)
                pos = torch.arange(past, past + n, dtype=torch.long).unsqueeze(0)
                with torch.inference_mode():
                    cos, sin = rot(q, pos)  # fp32 (q's dtype), attention_factor applied
                    assert cos.dtype == torch.float32
                    # modeling_qwen3.Qwen3Attention.forward: norm over head_dim, [batch, heads, tokens, dim], then the rotation
                    qr, kr = apply_rotary_pos_emb(qn(q).transpose(0, 1).unsqueeze(0), kn(k).transpose(0, 1).unsqueeze(0), cos, sin)
                out[f"{name}_{dt}_q_{past}_{n}"] = qr.squeeze(0).transpose(0, 1).contiguous().numpy().astype(np.float32)
                out[f"{name}_{dt}_k_{past}_{n}"] = kr.squeeze(0).transpose(0, 1).contiguous().numpy().astype(np.float32)
    out["cases"] = np.array(CASES, dtype=np.int64)
    path = os.path.join(HERE, "qk_norm_rope.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
