"""Shared by the q/k norm + RoPE fixture (tests/golden/make_qk_norm_golden.py) and its tests: the configurations, the
(past, n) grid and the seeded inputs.  Only outputs are stored in tests/golden/qk_norm_rope.npz; generator and tests
rebuild the same inputs from oracle.synth seeds.

Inputs are fp16 values; the ``bf16`` variant clears their low three mantissa bits, which makes every value exactly
representable in bf16 (tests/_bf16.py), so that one reference serves the same real numbers in either type.  q is scaled
by 4 and k by 1/4 (exact) so that the normalisation has something to do; the norm weights are 1 + N(0, 1) / 2, not ones."""
import numpy as np

from oracle.synth import normal_f16

EPS = 1e-6  # Qwen3's rms_norm_eps
# name -> (head_dim, q heads, kv heads, max_position_embeddings, rope_theta, rope_scaling as in a config.json or None)
CONFIGS = {
    "qwen3_default_mha": (128, 2, 2, 40960, 1000000.0, None),
    "qwen3_yarn_gqa4": (128, 4, 1, 131072, 1000000.0, {"rope_type": "yarn", "factor": 4.0,
                                                       "original_max_position_embeddings": 32768}),
    "llama3_d64_gqa2": (64, 4, 2, 131072, 500000.0, {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0,
                                                     "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "default_d256_gqa2": (256, 2, 1, 131072, 10000.0, None),
}
CASES = [(0, 2), (4094, 2), (131069, 3)]  # (past_kv_len, rows): the last row of the last case sits at position 131071
DTYPES = ("fp16", "bf16")


def mask3(a: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(a, np.float16).view(np.uint16) & np.uint16(0xFFF8)).view(np.float16)


def inputs(ci: int, i: int, dtype: str):
    """q ``[n, Hq, D]``, k ``[n, Hkv, D]``, q weight ``[D]``, k weight ``[D]`` of config index ``ci``, case index ``i``: fp16
    arrays (bf16: of bf16-representable values)."""
    d, hq, hkv = list(CONFIGS.values())[ci][:3]
    n = CASES[i][1]
    seed = 4000 + 100 * ci + 10 * i + (5 if dtype == "bf16" else 0)
    q = (normal_f16(seed * 4, (n, hq, d)).astype(np.float32) * 4.0).astype(np.float16)
    k = (normal_f16(seed * 4 + 1, (n, hkv, d)).astype(np.float32) * 0.25).astype(np.float16)
    wq = (1.0 + 0.5 * normal_f16(seed * 4 + 2, (d,)).astype(np.float32)).astype(np.float16)
    wk = (1.0 + 0.5 * normal_f16(seed * 4 + 3, (d,)).astype(np.float32)).astype(np.float16)
    if dtype == "bf16":
        q, k, wq, wk = mask3(q), mask3(k), mask3(wq), mask3(wk)
    return q, k, wq, wk


def quest_config(name: str):
    """The ``LlamaConfig`` whose RoPE parameters ``quest_amd.models.rope`` turns into the kernels' table."""
    from quest_amd.models.llama import LlamaConfig

    d, hq, hkv, max_pos, theta, scaling = CONFIGS[name]
    return LlamaConfig(hidden_size=640, num_attention_heads=hq, num_key_value_heads=hkv, head_dim=d,
                       max_position_embeddings=max_pos, rope_theta=theta, rope_scaling=dict(scaling) if scaling else None,
                       qk_norm=True, model_type="qwen3")
