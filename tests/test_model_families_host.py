"""Qwen3 (dense) and Mistral on the host: config parsing and refusals, the checkpoint round trip with transformers, the
frequency tables, the new C entries' symbols and return codes.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from _qk_norm import CONFIGS, quest_config

EINVAL, EUNSUPPORTED = -1, -2

# config.json of the published checkpoints (the fields that matter here, as published: transformers-4 spelling)
QWEN3_8B = {
    "architectures": ["Qwen3ForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "head_dim": 128,
    "hidden_act": "silu", "hidden_size": 4096, "intermediate_size": 12288, "max_position_embeddings": 40960,
    "max_window_layers": 36, "model_type": "qwen3", "num_attention_heads": 32, "num_hidden_layers": 36,
    "num_key_value_heads": 8, "rms_norm_eps": 1e-06, "rope_scaling": None, "rope_theta": 1000000, "sliding_window": None,
    "tie_word_embeddings": False, "torch_dtype": "bfloat16", "use_cache": True, "use_sliding_window": False,
    "vocab_size": 151936}
QWEN3_4B = dict(QWEN3_8B, hidden_size=2560, intermediate_size=9728, tie_word_embeddings=True)
MISTRAL_NEMO = {
    "architectures": ["MistralForCausalLM"], "attention_dropout": 0.0, "head_dim": 128, "hidden_act": "silu",
    "hidden_size": 5120, "intermediate_size": 14336, "max_position_embeddings": 131072, "model_type": "mistral",
    "num_attention_heads": 32, "num_hidden_layers": 40, "num_key_value_heads": 8, "rms_norm_eps": 1e-05,
    "rope_theta": 1000000.0, "sliding_window": None, "tie_word_embeddings": False, "torch_dtype": "bfloat16",
    "vocab_size": 131072}


def _parse(d):
    from quest_amd.models.llama import LlamaConfig

    return LlamaConfig.from_hf_dict(d)


@pytest.mark.parametrize("hf,head_dim,qk_norm,group,theta,eps", [
    (QWEN3_8B, 128, True, 4, 1e6, 1e-6), (QWEN3_4B, 128, True, 4, 1e6, 1e-6), (MISTRAL_NEMO, 128, False, 4, 1e6, 1e-5)],
    ids=["qwen3_8b", "qwen3_4b", "mistral_nemo"])
def test_from_hf_dict_parses_the_published_configs(hf, head_dim, qk_norm, group, theta, eps):
    from quest_amd.models import rope
    from quest_amd.models.llama import fused_layer_launches_supported

    cfg = _parse(hf)
    assert cfg.head_dim == head_dim and rope.head_dim_of(cfg) == head_dim
    assert cfg.qk_norm is qk_norm and cfg.model_type == hf["model_type"]
    assert cfg.num_attention_heads // cfg.num_key_value_heads == group
    assert cfg.rope_theta == theta and cfg.rope_scaling is None and cfg.rms_norm_eps == eps
    assert cfg.hidden_size == hf["hidden_size"] and cfg.num_attention_heads * cfg.head_dim == 4096
    assert cfg.max_position_embeddings == hf["max_position_embeddings"]
    # default RoPE of these families: the frequency table, transformers' expression
    inv_freq, factor = rope.rope_parameters(cfg)
    want = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    assert factor == 1.0 and torch.equal(inv_freq, want)
    assert fused_layer_launches_supported(cfg, 1) and fused_layer_launches_supported(cfg, 8)


def test_from_hf_dict_reads_qwen3_yarn_in_both_spellings():
    """Qwen3's 128K recipe: YaRN factor 4 over 32768, as ``rope_scaling`` (transformers 4) and as ``rope_parameters`` (5)."""
    from quest_amd.models import rope

    sc = {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}
    old = _parse(dict(QWEN3_8B, rope_scaling=dict(sc), max_position_embeddings=131072))
    new = dict(QWEN3_8B, max_position_embeddings=131072, rope_parameters=dict(sc, rope_theta=1000000.0))
    del new["rope_scaling"], new["rope_theta"]
    new = _parse(new)
    for cfg in (old, new):
        assert rope.rope_type(cfg.rope_scaling) == "yarn" and cfg.rope_theta == 1e6 and cfg.qk_norm
        inv_freq, factor = rope.rope_parameters(cfg)
        assert inv_freq.numel() == 64 and factor == pytest.approx(0.1 * math.log(4.0) + 1.0)
    assert torch.equal(rope.rope_parameters(old)[0], rope.rope_parameters(new)[0])


@pytest.mark.parametrize("change,field", [
    ({"attention_bias": True}, "attention_bias"),
    ({"mlp_bias": True}, "mlp_bias"),
    ({"partial_rotary_factor": 0.5}, "partial_rotary_factor"),
    ({"sliding_window": 4096, "use_sliding_window": True}, "use_sliding_window"),
    ({"layer_types": ["full_attention", "sliding_attention"] * 18}, "layer_types"),
    ({"model_type": "qwen3_moe"}, "model_type"),
    ({"model_type": "mixtral"}, "model_type"),
    ({"model_type": "qwen2"}, "model_type"),
])
def test_from_hf_dict_refusals_name_the_field(change, field):
    with pytest.raises(ValueError, match=field):
        _parse(dict(QWEN3_8B, **change))


def test_from_hf_dict_sliding_window():
    """Mistral-7B-v0.1 (sliding_window 4096, always active for that model type) is refused by name; a Qwen3 config that
    carries a window but has it switched off, and all-full-attention ``layer_types``, load."""
    with pytest.raises(ValueError, match="sliding_window"):
        _parse(dict(MISTRAL_NEMO, hidden_size=4096, sliding_window=4096))
    cfg = _parse(dict(QWEN3_8B, sliding_window=4096, use_sliding_window=False, layer_types=["full_attention"] * 36))
    assert cfg.qk_norm and cfg.head_dim == 128


@pytest.mark.parametrize("name", list(CONFIGS))
def test_rope_table_with_a_config_head_dim_equals_transformers(name):
    """models/rope.py with head_dim != hidden / heads: the table of the fixture's configs == transformers' inv_freq (stored
    in the fixture), bit for bit, and the attention factor."""
    from quest_amd.models import rope

    g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "qk_norm_rope.npz"))
    cfg = quest_config(name)
    assert cfg.hidden_size // cfg.num_attention_heads != cfg.head_dim
    inv_freq, factor = rope.rope_parameters(cfg)
    assert inv_freq.dtype == torch.float32 and inv_freq.numel() == cfg.head_dim // 2
    assert np.array_equal(inv_freq.numpy(), g[f"{name}_inv_freq"])
    assert factor == float(g[f"{name}_attention_factor"])


def _tiny(kind, transformers):
    common = dict(vocab_size=320, intermediate_size=1024, num_hidden_layers=2, max_position_embeddings=1024)
    if kind == "qwen3":
        cfg = transformers.Qwen3Config(hidden_size=512, head_dim=64, num_attention_heads=4, num_key_value_heads=2,
                                       rms_norm_eps=1e-6, tie_word_embeddings=True, **common)
        return transformers.Qwen3ForCausalLM, cfg
    cfg = transformers.MistralConfig(hidden_size=640, head_dim=128, num_attention_heads=4, num_key_value_heads=2,
                                     rms_norm_eps=1e-5, sliding_window=None, **common)
    return transformers.MistralForCausalLM, cfg


@pytest.mark.parametrize("kind", ["qwen3", "mistral"])
def test_checkpoint_round_trip_with_transformers(tmp_path, kind):
    """A tiny checkpoint written by transformers (head_dim != hidden / heads) loads; the parameter names are transformers';
    what save_pretrained writes, transformers' own class loads back with equal tensors and the same config."""
    transformers = pytest.importorskip("transformers")
    from quest_amd.models.llama import LlamaForCausalLM

    cls, hcfg = _tiny(kind, transformers)
    torch.manual_seed(5)
    hf = cls(hcfg)
    for n, p in hf.named_parameters():
        if "norm" in n:
            p.data.uniform_(0.5, 1.5)
    src = str(tmp_path / "hf")
    hf.half().save_pretrained(src, safe_serialization=True)
    m = LlamaForCausalLM.from_pretrained(src, device=torch.device("cpu"))
    cfg = m.config
    assert cfg.model_type == kind and cfg.qk_norm is (kind == "qwen3")
    assert cfg.head_dim == hcfg.head_dim and cfg.head_dim != cfg.hidden_size // cfg.num_attention_heads
    a = m.model.layers[0].self_attn
    assert a.head_dim == hcfg.head_dim and tuple(a.q_proj.weight.shape) == (4 * hcfg.head_dim, hcfg.hidden_size)
    assert tuple(a.o_proj.weight.shape) == (hcfg.hidden_size, 4 * hcfg.head_dim)
    want = hf.state_dict()
    assert set(m.state_dict()) == set(want)
    if kind == "qwen3":
        assert "model.layers.0.self_attn.q_norm.weight" in want and tuple(a.k_norm.weight.shape) == (64,)
        assert m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr()
    for n, t in m.state_dict().items():
        assert torch.equal(t, want[n]), n
    dst = str(tmp_path / "ours")
    m.save_pretrained(dst)
    back = cls.from_pretrained(dst, dtype=torch.float16)
    assert type(back.config) is type(hcfg) and back.config.head_dim == hcfg.head_dim
    assert getattr(back.config, "sliding_window", None) is None
    assert back.config.tie_word_embeddings == hcfg.tie_word_embeddings
    assert back.config.rms_norm_eps == hcfg.rms_norm_eps
    got = back.state_dict()
    assert set(got) == set(want)
    for n, t in want.items():
        assert torch.equal(got[n], t), n
    # and transformers runs what we wrote: the config it read back describes the same network as the one it wrote itself
    # (both loaded from disk: ``hf.half()`` above also rounded that instance's rotary buffer)
    first = cls.from_pretrained(src, dtype=torch.float16)
    ids = (torch.arange(12)[None] * 37 + 11) % 320
    with torch.no_grad():
        assert torch.equal(back.float()(input_ids=ids).logits, first.float()(input_ids=ids).logits)


def test_attention_module_without_a_config_head_dim_is_unchanged():
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    with torch.device("meta"):
        m = LlamaForCausalLM(LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=512, num_hidden_layers=1,
                                         num_attention_heads=4, num_key_value_heads=2))
    a = m.model.layers[0].self_attn
    assert a.head_dim == 64 and not a.qk_norm and not a.rope_table and not hasattr(a, "q_norm")
    assert "head_dim" not in m.config.to_hf_dict() and m.config.to_hf_dict()["model_type"] == "llama"
    with pytest.raises(ValueError):
        LlamaConfig(model_type="qwen3_moe")


# ---------------------------------------------------------------------------------------------- the C entries
def test_new_symbols_are_exported_and_declared():
    import os

    from quest_amd import _kernels
    from quest_amd._lib import SIGNATURES, lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quest_hip.h")).read()
    for name, n_args in (("quest_apply_qk_norm_rope_in_place_dtype", 17), ("quest_decode_qkv", 14),
                         ("quest_decode_qkv_batched", 15)):
        assert hasattr(lib, name) and len(SIGNATURES[name][1]) == n_args
        assert f"int {name}(" in header
    for fn in ("apply_qk_norm_rope_in_place", "decode_qkv", "decode_qkv_batched"):
        assert callable(getattr(_kernels, fn))
    import quest_amd.utils as qu

    assert "apply_qk_norm_rope_in_place" in qu.__all__


ONE = ctypes.c_void_p(16)  # non-null, never dereferenced: every call below is refused before a launch
NAN, INF = float("nan"), float("inf")


def _norm_rope(**kw):
    a = dict(q=ONE, k=ONE, n=4, past=0, hq=8, hkv=2, d=128, wq=ONE, wk=ONE, eps=1e-6, scale=1.0, theta=1e6, inv_freq=None,
             attn=1.0, states=None, dtype=0, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("change,code", [
    (dict(q=None), EINVAL), (dict(k=None), EINVAL), (dict(wq=None), EINVAL), (dict(wk=None), EINVAL),
    (dict(hq=0), EINVAL), (dict(hkv=0), EINVAL),
    (dict(dtype=2), EINVAL), (dict(dtype=7, d=96), EINVAL),
    (dict(eps=-1e-6), EINVAL), (dict(eps=NAN), EINVAL), (dict(eps=INF), EINVAL),
    (dict(scale=0.0), EINVAL), (dict(theta=0.0), EINVAL), (dict(theta=-1.0), EINVAL),
    (dict(inv_freq=ONE, attn=0.0), EINVAL), (dict(inv_freq=ONE, attn=NAN), EINVAL), (dict(inv_freq=ONE, attn=INF), EINVAL),
    (dict(inv_freq=ONE, attn=-1.0), EINVAL),
    (dict(d=96), EUNSUPPORTED), (dict(d=32), EUNSUPPORTED), (dict(d=512), EUNSUPPORTED), (dict(d=0), EUNSUPPORTED),
    (dict(d=96, dtype=1, inv_freq=ONE), EUNSUPPORTED),
    (dict(d=96, wq=None), EINVAL), (dict(d=96, eps=NAN), EINVAL),  # the argument checks come before the shape's
    (dict(n=0), 0), (dict(n=0, dtype=1, d=64, inv_freq=ONE, attn=1.2), 0), (dict(n=0, d=256, eps=0.0), 0),
])
def test_qk_norm_rope_return_codes(change, code):
    from quest_amd._lib import lib

    assert lib.quest_apply_qk_norm_rope_in_place_dtype(*_norm_rope(**change)) == code


def _qkv(batched, **kw):
    a = dict(h=ONE, gamma=ONE, eps=1e-6, wq=ONE, wk=ONE, wv=ONE, q=ONE, k=ONE, v=ONE, hidden=4096, q_rows=4096, kv_rows=1024)
    if batched:
        a["n"] = 8
    a["dtype"], a["stream"] = 0, None  # QUEST_DTYPE_F16
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("batched", [False, True])
def test_decode_qkv_return_codes(batched):
    from quest_amd._lib import lib

    fn = lib.quest_decode_qkv_batched if batched else lib.quest_decode_qkv
    for name in ("h", "gamma", "wq", "wk", "wv", "q", "k", "v"):
        assert fn(*_qkv(batched, **{name: None})) == EINVAL, name
    for name in ("hidden", "q_rows", "kv_rows"):
        assert fn(*_qkv(batched, **{name: 0})) == EINVAL, name
    assert fn(*_qkv(batched, hidden=4100)) == EUNSUPPORTED  # not a multiple of 8 halves
    assert fn(*_qkv(batched, hidden=4100, q=None)) == EINVAL
    if batched:
        assert fn(*_qkv(True, n=0)) == EINVAL and fn(*_qkv(True, n=17)) == EINVAL
    else:
        assert fn(*_qkv(False, hidden=30728)) == EUNSUPPORTED  # the input vector does not fit the workgroup's LDS


def test_batched_plan_of_the_unrotated_launch():
    """quest_decode_qkv_batched is planned with the rotating launch's LDS budget, so the n-token kernel it takes is
    quest_decode_batched_plan's answer with rope = 1: Qwen3-8B shapes stay in the persistent kernel at every batch size,
    inputs longer than its LDS take the inputs-from-L2 kernel."""
    from quest_amd._lib import lib

    info = (ctypes.c_uint32 * 6)()
    for n in (1, 4, 8, 16):
        assert lib.quest_decode_batched_plan(4096, 6144, n, 1, info) == 1
        assert lib.quest_decode_batched_plan(2560, 6144, n, 1, info) == 1  # Qwen3-4B
    assert lib.quest_decode_batched_plan(8704, 1536, 8, 1, info) == 0
    # the plain launches' budget is 4 KiB per token group larger; today the per-thread input-vector limit binds first, so
    # both budgets choose alike at every shape -- the unrotated launch does not rely on that
    for n in (1, 4, 5, 8, 9, 16):
        for hidden in range(512, 16384, 128):
            assert lib.quest_decode_batched_plan(hidden, 6144, n, 0, info) == lib.quest_decode_batched_plan(hidden, 6144, n, 1, info)


def test_new_kernels_use_no_scratch_and_do_not_spill():
    """Code-object metadata of the built library (no GPU): the six instantiations of the q/k norm + RoPE kernel -- fp16 and
    bf16, head_dim 64 / 128 / 256 -- exist, use no scratch and spill nothing (sincosf's large-argument path and the 8-way
    unroll are what could start to), and need no LDS.  The unrotated q/k/v launches add no kernel: of the plain-mode GEMV
    kernels they launch, the batch-1 and the persistent one are held to the same (the inputs-from-L2 fallback's 16-token
    instantiation has spilled 8 registers since it was written: csrc/decode_layer.hip, launch_skinny_tg)."""
    import os

    from quest_amd.build import LIB, kernel_metadata

    llvm = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
    if not os.path.exists(os.path.join(llvm, "llvm-readelf")):
        pytest.skip("needs the ROCm LLVM tools (llvm-objcopy / llvm-readelf)")
    meta = kernel_metadata(LIB)
    for d in (64, 128, 256):
        for frag in (f"19qk_norm_rope_kernelILi{d}E", f"24qk_norm_rope_kernel_bf16ILi{d}E"):
            hits = [v for k, v in meta.items() if frag in k]
            assert len(hits) == 1, (frag, [k for k in meta if "qk_norm_rope" in k])
            v = hits[0]
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["lds"] == 0, (frag, v)
            assert v["vgpr"] <= 128, (frag, v)  # 256-thread workgroups, several per SIMD
    assert len([k for k in meta if "qk_norm_rope_kernel" in k]) == 6
    for frag in ("11gemv_kernelILi0E", "14persist_kernelILi0E"):  # MODE = kGvPlain
        hits = {k: v for k, v in meta.items() if frag in k}
        assert hits, frag
        for k, v in hits.items():
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)


def test_qk_norm_model_refuses_a_head_dim_its_launch_does_not_serve():
    """The q/k norm runs only inside the fused norm + RoPE launch (head_dim 64 / 128 / 256): a config outside that is refused
    when the model is built, by name, not at the first forward."""
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=64, hidden_size=384, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=96, qk_norm=True, model_type="qwen3")
    with pytest.raises(ValueError, match="head_dim"):
        with torch.device("meta"):
            LlamaForCausalLM(cfg)
    cfg.qk_norm, cfg.model_type = False, "mistral"  # without the norm the module path serves any head_dim
    with torch.device("meta"):
        assert LlamaForCausalLM(cfg).model.layers[0].self_attn.head_dim == 96
