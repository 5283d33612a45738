"""Scaled RoPE (llama3 / yarn) on the host: the frequency table of quest_amd/models/rope.py against transformers'
(tests/golden/hf_rope_scaling_golden.npz, make_rope_scaling_golden.py), the real config.json of the models that use it,
the refusals, and the table's C entries' argument checks (no GPU: they return before anything is launched)."""
import copy
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hf_rope_scaling_golden.npz")

# name -> (head_dim, num_heads, max_position_embeddings, rope_theta, rope_scaling): make_rope_scaling_golden.CONFIGS
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

# config.json of the published checkpoints (the fields the Quest path reads and the rope ones, verbatim)
LLAMA31_8B = {
    "architectures": ["LlamaForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "bos_token_id": 128000,
    "eos_token_id": 128001, "hidden_act": "silu", "hidden_size": 4096, "initializer_range": 0.02,
    "intermediate_size": 14336, "max_position_embeddings": 131072, "mlp_bias": False, "model_type": "llama",
    "num_attention_heads": 32, "num_hidden_layers": 32, "num_key_value_heads": 8, "pretraining_tp": 1,
    "rms_norm_eps": 1e-05,
    "rope_scaling": {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                     "original_max_position_embeddings": 8192, "rope_type": "llama3"},
    "rope_theta": 500000.0, "tie_word_embeddings": False, "torch_dtype": "bfloat16", "use_cache": True,
    "vocab_size": 128256}
LLAMA32_1B = {
    "architectures": ["LlamaForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "bos_token_id": 128000,
    "eos_token_id": 128001, "head_dim": 64, "hidden_act": "silu", "hidden_size": 2048, "initializer_range": 0.02,
    "intermediate_size": 8192, "max_position_embeddings": 131072, "mlp_bias": False, "model_type": "llama",
    "num_attention_heads": 32, "num_hidden_layers": 16, "num_key_value_heads": 8, "pretraining_tp": 1,
    "rms_norm_eps": 1e-05,
    "rope_scaling": {"factor": 32.0, "high_freq_factor": 4.0, "low_freq_factor": 1.0,
                     "original_max_position_embeddings": 8192, "rope_type": "llama3"},
    "rope_theta": 500000.0, "tie_word_embeddings": True, "torch_dtype": "bfloat16", "use_cache": True,
    "vocab_size": 128256}
YARN_LLAMA2_7B_128K = {
    "architectures": ["LlamaForCausalLM"], "bos_token_id": 1, "eos_token_id": 2, "hidden_act": "silu",
    "hidden_size": 4096, "initializer_range": 0.02, "intermediate_size": 11008, "max_position_embeddings": 131072,
    "model_type": "llama", "num_attention_heads": 32, "num_hidden_layers": 32, "num_key_value_heads": 32,
    "pretraining_tp": 1, "rms_norm_eps": 1e-05,
    "rope_scaling": {"factor": 32.0, "original_max_position_embeddings": 4096, "type": "yarn", "finetuned": True},
    "rope_theta": 10000.0, "tie_word_embeddings": False, "torch_dtype": "float16", "use_cache": True,
    "vocab_size": 32000}
CHECKPOINTS = {"llama31_8b": LLAMA31_8B, "llama32_1b": LLAMA32_1B, "yarn_llama2_7b_128k": YARN_LLAMA2_7B_128K}


def _v5(d: dict) -> dict:
    """The transformers-5 spelling of a config.json: theta and scaling nested in rope_parameters."""
    d = copy.deepcopy(d)
    sc = d.pop("rope_scaling")
    params = {k: v for k, v in sc.items() if k != "type"}
    params["rope_type"] = sc.get("rope_type", sc.get("type"))
    params["rope_theta"] = d.pop("rope_theta")
    d["rope_parameters"] = params
    return d


def _cfg(name):
    d, heads, max_pos, theta, sc = CONFIGS[name]
    return SimpleNamespace(hidden_size=d * heads, num_attention_heads=heads, max_position_embeddings=max_pos,
                           rope_theta=theta, rope_scaling=copy.deepcopy(sc))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_inv_freq_and_attention_factor_equal_transformers(golden, name):
    from quest_amd.models import rope

    inv_freq, factor = rope.rope_parameters(_cfg(name))
    want = torch.from_numpy(golden[f"{name}_inv_freq"])
    assert inv_freq.dtype == torch.float32 and inv_freq.shape == want.shape == (CONFIGS[name][0] // 2,)
    assert torch.equal(inv_freq, want), (inv_freq - want).abs().max()
    ref = float(golden[f"{name}_attention_factor"])
    assert abs(factor - ref) <= 1e-7 * ref, (factor, ref)


def test_yarn_attention_factor_of_the_128k_checkpoint():
    from quest_amd.models import rope

    assert abs(rope.rope_parameters(_cfg("yarn_llama2_7b_128k"))[1] - 1.3466) < 1e-4
    assert rope.rope_parameters(_cfg("llama31_8b"))[1] == 1.0


def test_default_and_linear_keep_the_kernel_formula():
    from quest_amd.models import rope
    from quest_amd.models.QuestAttention import QuestAttention

    for sc in (None, {"type": "linear", "factor": 4.0}, {"rope_type": "default"}):
        cfg = SimpleNamespace(hidden_size=256, num_attention_heads=2, rope_scaling=sc)
        assert rope.rope_parameters(cfg) is None
        m = QuestAttention(cfg, 0)
        assert not m.rope_table and m.rotary(torch.device("cpu")) is None
        assert m.rope_scale == (4.0 if sc and sc.get("type") == "linear" else 1.0)


@pytest.mark.parametrize("name", list(CHECKPOINTS))
@pytest.mark.parametrize("spelling", ["transformers4", "transformers5"])
def test_from_hf_dict_accepts_the_checkpoints(golden, name, spelling):
    from quest_amd.models import rope
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    hf = CHECKPOINTS[name] if spelling == "transformers4" else _v5(CHECKPOINTS[name])
    cfg = LlamaConfig.from_hf_dict(hf)
    assert cfg.rope_theta == CHECKPOINTS[name]["rope_theta"]
    assert rope.rope_type(cfg.rope_scaling) == ("yarn" if "yarn" in name else "llama3")
    inv_freq, factor = rope.rope_parameters(cfg)
    assert torch.equal(inv_freq, torch.from_numpy(golden[f"{name}_inv_freq"]))
    assert factor == pytest.approx(float(golden[f"{name}_attention_factor"]), rel=1e-7)
    with torch.device("meta"):  # how from_pretrained builds the model
        m = LlamaForCausalLM(cfg)
    attn = m.model.layers[0].self_attn
    assert attn.rope_table and attn.rope_scale == 1.0 and attn.rope_theta == cfg.rope_theta
    assert not any("inv_freq" in k or "rope" in k for k in m.state_dict())  # nothing a checkpoint would lack


def test_save_load_round_trip_keeps_the_rope_dict(tmp_path, golden):
    """A small llama3 model through save_pretrained / from_pretrained (on the CPU): the rope dict survives, the model is
    built on `meta` under an fp16 default dtype, and the table it materialises is still transformers' fp32 one."""
    pytest.importorskip("safetensors")
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    sc = dict(CONFIGS["llama31_8b"][4])
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=1, max_position_embeddings=131072, rope_scaling=sc, rope_theta=500000.0)
    m = LlamaForCausalLM(cfg).half()
    m.save_pretrained(str(tmp_path))
    with open(tmp_path / "config.json") as f:
        assert json.load(f)["rope_scaling"] == sc
    back = LlamaForCausalLM.from_pretrained(str(tmp_path), device=torch.device("cpu"))
    assert back.config.rope_scaling == sc and back.config.rope_theta == 500000.0
    inv_freq, factor = back.model.layers[1].self_attn.rotary(torch.device("cpu"))
    assert inv_freq.dtype == torch.float32 and factor == 1.0
    assert torch.equal(inv_freq, torch.from_numpy(golden["llama31_8b_inv_freq"]))


@pytest.mark.parametrize("scaling", [
    {"type": "yarn"},
    {"rope_type": "yarn", "original_max_position_embeddings": 4096},
    {"rope_type": "llama3", "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192},
    {"rope_type": "llama3", "factor": 8.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192},
    {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "original_max_position_embeddings": 8192},
    {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0},
    {"type": "dynamic", "factor": 2.0},
    {"rope_type": "longrope", "factor": 2.0, "short_factor": [1.0], "long_factor": [1.0]},
    {"rope_type": "yarn", "factor": 4.0, "partial_rotary_factor": 0.5},
])
def test_refusals(scaling):
    from quest_amd.models import rope
    from quest_amd.models.QuestAttention import QuestAttention

    cfg = SimpleNamespace(hidden_size=512, num_attention_heads=4, max_position_embeddings=4096, rope_scaling=scaling)
    with pytest.raises(ValueError):
        rope.rope_parameters(cfg)
    with pytest.raises(ValueError):
        QuestAttention(cfg, 0)


def test_from_hf_dict_refuses_partial_rotary():
    from quest_amd.models.llama import LlamaConfig

    for d in (dict(LLAMA31_8B, partial_rotary_factor=0.5), _v5(LLAMA31_8B)):
        if "rope_parameters" in d:
            d["rope_parameters"]["partial_rotary_factor"] = 0.5
        with pytest.raises(ValueError):
            LlamaConfig.from_hf_dict(d)


def test_c_entries_refuse_a_missing_table_or_a_bad_attention_factor():
    """QUEST_EINVAL before any launch: no frequency source (NULL table = the formula, and no usable rope_scale / rope_theta
    for it), attention_factor <= 0, NaN or infinite.  With a table rope_scale / rope_theta are not looked at.  (Dummy non-NULL
    tensor pointers: nothing is dereferenced on these paths.)"""
    from quest_amd._lib import lib

    EINVAL, F16 = -1, 0  # QUEST_EINVAL, QUEST_DTYPE_F16
    assert lib.quest_error_string(EINVAL).decode()
    p = ctypes.c_void_p(16)
    table = ctypes.c_void_p(64)
    for tab, f in ((None, 1.0), (table, 0.0), (table, -1.0), (table, float("nan")), (table, float("inf"))):
        assert lib.quest_apply_rope_in_place_dtype(p, p, 1, 0, 4, 4, 128, 0.0, 0.0, tab, f, None, 0, None) == EINVAL
        assert lib.quest_apply_rope_in_place_dtype(p, p, 1, 0, 4, 4, 128, 0.0, 0.0, tab, f, p, 0, None) == EINVAL
        assert lib.quest_decode_qkv_rope(p, p, 1e-5, p, p, p, p, p, p, 512, 4, 4, 128, 0.0, 0.0, tab, f, p, F16, None) == EINVAL
        assert lib.quest_decode_qkv_rope_batched(p, p, 1e-5, p, p, p, p, p, p, 512, 4, 4, 128, 0.0, 0.0, tab, f, p, 2,
                                                 F16, None) == EINVAL
    # head-dim rules of the existing entries (checked before any launch as well); n == 0 launches nothing
    assert lib.quest_apply_rope_in_place_dtype(p, p, 1, 0, 4, 4, 96, 0.0, 0.0, table, 1.0, None, 0, None) < 0
    assert lib.quest_apply_rope_in_place_dtype(p, p, 0, 0, 4, 4, 128, 0.0, 0.0, table, 1.0, None, 0, None) == 0
    assert lib.quest_apply_rope_in_place_dtype(None, p, 1, 0, 4, 4, 128, 0.0, 0.0, table, 1.0, None, 0, None) == EINVAL
    assert lib.quest_decode_qkv_rope(p, p, 1e-5, p, p, p, p, p, p, 512, 4, 4, 130, 0.0, 0.0, table, 1.0, p, F16, None) < 0
    assert lib.quest_decode_qkv_rope_batched(p, p, 1e-5, p, p, p, p, p, p, 512, 4, 4, 72, 0.0, 0.0, table, 1.0, p, 2,
                                             F16, None) < 0
