#!/usr/bin/env python3
"""Scaled-RoPE fixtures (llama3 / yarn) from Hugging Face transformers, the oracle of quest_amd/models/rope.py and the
kernels' frequency-table form.

Per config: ``inv_freq`` and ``attention_factor`` from ``ROPE_INIT_FUNCTIONS`` (modeling_rope_utils), and q / k rotated by
``LlamaRotaryEmbedding`` + ``apply_rotary_pos_emb`` in fp32 at the (past, n) grid below -- the rotary module is built
directly in fp32 (``Module.half()`` would also round its ``inv_freq`` buffer to fp16).  Inputs come from oracle.synth
seeds (fp16 values, rotated in fp32); only outputs are stored, rounded to fp16 (the kernels' output type) to keep the
file small.

    python tests/golden/make_rope_scaling_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS  # noqa: E402
from transformers.models.llama.configuration_llama import LlamaConfig  # noqa: E402
from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding, apply_rotary_pos_emb  # noqa: E402

from oracle.synth import normal_f16  # noqa: E402

# name -> (head_dim, num_heads, max_position_embeddings, rope_theta, rope_scaling dict as in the checkpoints' config.json)
CONFIGS = {
    "llama31_8b": (128, 32, 131072, 500000.0, {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                               "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "llama32_1b": (64, 32, 131072, 500000.0, {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0,
                                              "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "yarn_llama2_7b_128k": (128, 32, 131072, 10000.0, {"type": "yarn", "factor": 32.0,
                                                       "original_max_position_embeddings": 4096}),
    "yarn_mscale": (128, 32, 65536, 10000.0, {"type": "yarn", "factor": 16.0, "original_max_position_embeddings": 4096,
                                              "mscale": 0.707, "mscale_all_dim": 0.5, "beta_fast": 24,
                                              "beta_slow": 2}),
}
CASES = [(0, 5), (4090, 64), (8190, 4), (32760, 16), (131068, 4)]
HQ, HKV = 1, 1  # one head each: the file stays small (the kernels' head indexing is the formula path's)


def hf_config(head_dim, heads, max_pos, theta, scaling):
    params = dict(scaling)
    params["rope_type"] = params.pop("type", params.get("rope_type"))
    params["rope_theta"] = theta
    return LlamaConfig(hidden_size=head_dim * heads, num_attention_heads=heads, num_key_value_heads=heads,
                       max_position_embeddings=max_pos, rope_parameters=params)


def main():
    out = {}
    for ci, (name, (d, heads, max_pos, theta, scaling)) in enumerate(CONFIGS.items()):
        cfg = hf_config(d, heads, max_pos, theta, scaling)
        kind = cfg.rope_parameters["rope_type"]
        inv_freq, factor = ROPE_INIT_FUNCTIONS[kind](cfg, torch.device("cpu"))
        rot = LlamaRotaryEmbedding(cfg)
        assert rot.inv_freq.dtype == torch.float32 and torch.equal(rot.inv_freq, inv_freq)
        out[f"{name}_inv_freq"] = inv_freq.numpy().astype(np.float32)
        out[f"{name}_attention_factor"] = np.array(factor, np.float64)
        for i, (past, n) in enumerate(CASES):
            seed = 900 + 10 * ci + i
            q = torch.from_numpy(normal_f16(seed * 3, (n, HQ, d))).float()
            k = torch.from_numpy(normal_f16(seed * 3 + 1, (n, HKV, d))).float()
            pos = torch.arange(past, past + n, dtype=torch.long).unsqueeze(0)
            with torch.inference_mode():
                cos, sin = rot(q, pos)  # fp32 (q's dtype), attention_factor applied
                qr, kr = apply_rotary_pos_emb(q.transpose(0, 1).unsqueeze(0), k.transpose(0, 1).unsqueeze(0), cos, sin)
            out[f"{name}_q_{past}_{n}"] = qr.squeeze(0).transpose(0, 1).contiguous().numpy().astype(np.float16)
            out[f"{name}_k_{past}_{n}"] = kr.squeeze(0).transpose(0, 1).contiguous().numpy().astype(np.float16)
    out["cases"] = np.array(CASES, dtype=np.int64)
    out["seeds_base"] = np.array([900, 10, HQ, HKV], dtype=np.int64)  # seed = 900 + 10 * config index + case index
    path = os.path.join(HERE, "hf_rope_scaling_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
