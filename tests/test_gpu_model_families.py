"""Qwen3 (per-head q/k RMSNorm before RoPE, head_dim a config field) and Mistral (Llama arithmetic, free head_dim)
checkpoints written by transformers, through from_pretrained -> quest_init -> prefill -> graph-replayed decode, against
transformers' logits.

Yardstick (tests/test_gpu_hf_checkpoint.py's, unchanged): with r32 = transformers in fp32 and r16 = transformers' own fp16
run on the same GPU, rel(got, r32) <= 1.5 rel(r16, r32) + 2e-3 and rel(got, r16) <= 1e-2; bf16 models
(tests/test_gpu_bf16_model.py's): rel(got, r32) <= 1.5 rel(rbf, r32) + 2e-3.  The fused norm + RoPE launch rounds once
where transformers rounds after the normalisation, after the weight and on cos / sin: these tests are the arbiter of
that deviation.  On the sparse path (budget 4 pages) eager == graph replay and NHD == NHD_ROT bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
YARN = {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 256, "rope_theta": 1000000.0}
KINDS = ["qwen3", "qwen3_yarn", "mistral"]
N_NEW = 20  # 150 prompt tokens + 20: crosses the page boundary at 160


def _hf_class(kind, transformers):
    common = dict(vocab_size=320, intermediate_size=1024, num_hidden_layers=3, max_position_embeddings=1024)
    if kind.startswith("qwen3"):
        rope = dict(YARN) if kind == "qwen3_yarn" else {"rope_type": "default", "rope_theta": 1000000.0}
        # head_dim 64 at hidden 512 with 4 heads (4 x 64 != 512), GQA, tied embeddings, eps 1e-6
        return transformers.Qwen3ForCausalLM, transformers.Qwen3Config(
            hidden_size=512, head_dim=64, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-6,
            tie_word_embeddings=True, rope_parameters=rope, **common)
    # head_dim 128 at hidden 640 with 4 heads (4 x 128 != 640)
    return transformers.MistralForCausalLM, transformers.MistralConfig(
        hidden_size=640, head_dim=128, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-5,
        sliding_window=None, rope_parameters={"rope_type": "default", "rope_theta": 1000000.0}, **common)


def _checkpoint(tmp_path, kind, dtype=torch.float16):
    """A tiny random checkpoint of the family saved by transformers in ``dtype``; the q/k norm weights are random
    (uniform 0.5 .. 1.5), the other norms ones as in tests/test_gpu_hf_checkpoint.py.  Returns the directory, transformers'
    fp32 model (CPU) and its ``dtype`` model (GPU)."""
    transformers = pytest.importorskip("transformers")
    cls, hcfg = _hf_class(kind, transformers)
    torch.manual_seed(3)
    hf = cls(hcfg)
    for p in hf.parameters():
        p.data.mul_(2.0)
    g = torch.Generator().manual_seed(9)
    for n, p in hf.named_parameters():
        if "q_norm" in n or "k_norm" in n:
            p.data.copy_(0.5 + torch.rand(p.shape, generator=g))
        elif "norm" in n:
            p.data.fill_(1.0)
    d = str(tmp_path / "ckpt")
    hf.to(dtype).save_pretrained(d, safe_serialization=True)
    hf32 = cls.from_pretrained(d, dtype=torch.float32, attn_implementation="eager").eval()
    hflo = cls.from_pretrained(d, dtype=dtype, attn_implementation="eager").to(DEV).eval()
    if kind == "qwen3_yarn":
        assert hf32.model.rotary_emb.rope_type == "yarn"
    return d, hf32, hflo


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _check(got, rlo, r32, what, bf16=False):
    got, rlo = got.float().cpu(), rlo.float().cpu()
    e, y = _rel(got, r32), _rel(rlo, r32)
    print(f"{what}: rel(got, hf_fp32)={e:.4e} rel(hf_low, hf_fp32)={y:.4e} rel(got, hf_low)={_rel(got, rlo):.4e}")
    assert torch.isfinite(got).all(), what
    assert e <= 1.5 * y + 2e-3, f"{what}: {e:.4f} vs transformers' own low-precision run {y:.4f}"
    if not bf16:
        assert _rel(got, rlo) <= 1e-2, f"{what}: {_rel(got, rlo):.4f} from transformers' fp16 logits"


def _hf_run(hf32, hflo, prompt, n_new):
    """transformers' logits (fp32 on the CPU, the low-precision model on the GPU) for the prompt's positions and n_new
    greedy tokens (the fp32 model's choice feeds both)."""
    with torch.no_grad():
        r32 = hf32(input_ids=prompt.cpu(), use_cache=True)
        rlo = hflo(input_ids=prompt.to(DEV), use_cache=True)
    first = (r32.logits[0], rlo.logits[0])
    p32, plo, tok = r32.past_key_values, rlo.past_key_values, r32.logits[0, -1].argmax()
    toks, steps = [], []
    for _ in range(n_new):
        toks.append(int(tok))
        with torch.no_grad():
            r32 = hf32(input_ids=tok.view(1, 1), past_key_values=p32, use_cache=True)
            rlo = hflo(input_ids=tok.view(1, 1).to(DEV), past_key_values=plo, use_cache=True)
        p32, plo = r32.past_key_values, rlo.past_key_values
        steps.append((r32.logits[0, -1], rlo.logits[0, -1]))
        tok = r32.logits[0, -1].argmax()
    return first, toks, steps


def _expect(kind, m):
    """What the loaded model must look like for the family."""
    a = m.model.layers[0].self_attn
    qwen = kind.startswith("qwen3")
    assert m.config.model_type == ("qwen3" if qwen else "mistral")
    assert a.qk_norm is qwen and a.head_dim == (64 if qwen else 128)
    assert a.head_dim * a.num_heads != m.config.hidden_size and a.rope_table and a.rope_scale == 1.0
    if qwen:
        assert m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr()  # tied embeddings
        assert float(a.q_norm.weight.detach().float().std()) > 0.1  # random, not ones
    return 5 if qwen else 4  # projection launches per layer of the fused step


class _CountLaunches:
    """Counts the calls of the projection launches of a step while it is captured (the capture runs the step twice: a
    warm-up and the recording), by wrapping the ``_kernels`` functions the model layer calls."""
    NAMES = ("decode_qkv", "decode_qkv_batched", "decode_qkv_rope", "decode_qkv_rope_freqs", "decode_qkv_rope_batched",
             "decode_qkv_rope_batched_freqs", "apply_qk_norm_rope_in_place", "apply_rope_in_place_freqs",
             "apply_rope_in_place_batched", "decode_gemv_residual", "decode_gemv_residual_batched", "decode_mlp_gate_up",
             "decode_mlp_gate_up_batched")

    def __enter__(self):
        from quest_amd import _kernels

        self.calls, self._saved = {n: 0 for n in self.NAMES}, {}
        for n in self.NAMES:
            fn = self._saved[n] = getattr(_kernels, n)

            def wrapped(*a, _n=n, _fn=fn, **kw):
                self.calls[_n] += 1
                return _fn(*a, **kw)
            setattr(_kernels, n, wrapped)
        return self

    def __exit__(self, *exc):
        from quest_amd import _kernels

        for n, fn in self._saved.items():
            setattr(_kernels, n, fn)

    def check_fused(self, qk_norm: bool, layers: int, batched: bool):
        """Per layer and run of the step: a Qwen3 layer = q/k/v unrotated + norm-RoPE + 2 GEMV-residual + gate/up (five), any
        other = rotating q/k/v + 2 GEMV-residual + gate/up (four); nothing of the other form, no stand-alone RoPE."""
        c, runs = self.calls, 2 * layers
        sfx = "_batched" if batched else ""
        rot = c["decode_qkv_rope"] + c["decode_qkv_rope_freqs"] + c["decode_qkv_rope_batched"] + c["decode_qkv_rope_batched_freqs"]
        plain = c["decode_qkv"] + c["decode_qkv_batched"]
        assert c["decode_gemv_residual" + sfx] == 2 * runs and c["decode_mlp_gate_up" + sfx] == runs, c
        assert c["apply_rope_in_place_freqs"] == 0 and c["apply_rope_in_place_batched"] == 0, c
        if qk_norm:
            assert c["decode_qkv" + sfx] == runs and plain == runs and rot == 0 and c["apply_qk_norm_rope_in_place"] == runs, c
        else:
            assert rot == runs and plain == 0 and c["apply_qk_norm_rope_in_place"] == 0, c


def _single_sequence(tmp_path, kind, dtype, fused):
    from quest_amd.models.llama import LlamaForCausalLM

    d, hf32, hflo = _checkpoint(tmp_path, kind, dtype)
    dev, bf16 = torch.device(DEV), dtype == BF
    prompt = (torch.arange(150)[None] * 37 + 11) % 320
    first, toks, steps = _hf_run(hf32, hflo, prompt, N_NEW)
    m = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=dtype)
    launches = _expect(kind, m)
    m.quest_init(16, 512, token_budget=16 * 1024, dtype=dtype)  # budget >= pages: full attention, comparable with HF
    with torch.inference_mode():
        got_all = m.lm_head(m.model(input_ids=prompt.to(dev)))[0]
    _check(got_all, first[1], first[0], "prefill, all positions", bf16)
    _check(got_all[-1], first[1][-1], first[0][-1], "prefill, last position", bf16)
    with _CountLaunches() as count:
        m.capture_decode_graph(fused_layers=fused)
    if bf16:
        assert not m.fused_layers  # the fused projection launches are fp16-only: the module path
    else:
        assert m.fused_layers == (fused is not False)
    if m.fused_layers:
        count.check_fused(launches == 5, m.config.num_hidden_layers, batched=False)
    else:  # module path: nn.Linear projections; a Qwen3 layer's norm + RoPE launch takes the RoPE launch's place
        c, runs = count.calls, 2 * m.config.num_hidden_layers
        assert c["apply_qk_norm_rope_in_place"] == (runs if launches == 5 else 0), c
        assert c["apply_rope_in_place_freqs"] == (0 if launches == 5 else runs), c
        assert not any(v for n, v in c.items() if n.startswith("decode_")), c
    for t in range(N_NEW):
        with torch.inference_mode():
            got = m.decode_graph_step(input_ids=torch.tensor([[toks[t]]], device=dev))
        _check(got[0, -1], steps[t][1], steps[t][0], f"decode token {t}", bf16)
    assert m.model.iController.kv_cache.seqlen == 150 + N_NEW


@pytest.mark.parametrize("fused", [None, False], ids=["fused_default", "module_path"])
@pytest.mark.parametrize("kind", KINDS)
def test_fp16_checkpoint_matches_transformers(tmp_path, kind, fused):
    """Prefill at all positions, then 20 captured decode tokens across a page boundary; ``fused_default``: fused_layers is on
    by default and a Qwen3 layer takes the five-launch form (a Mistral layer the four launches)."""
    _single_sequence(tmp_path, kind, torch.float16, fused)


@pytest.mark.parametrize("kind", ["qwen3", "mistral"])
def test_bf16_checkpoint_matches_transformers_on_the_module_path(tmp_path, kind):
    _single_sequence(tmp_path, kind, BF, None)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_of_three_ragged_prompts(tmp_path, kind):
    """Three prompts of different lengths over the shared pools, decoded together by the fused n-token launches: every
    sequence against transformers at the single-sequence yardstick."""
    from quest_amd.models.llama import LlamaForCausalLM

    d, hf32, hf16 = _checkpoint(tmp_path, kind)
    dev = torch.device(DEV)
    prompts = [((torch.arange(L)[None] * (7 + i) + i) % 320) for i, L in enumerate((150, 97, 201))]
    refs = [_hf_run(hf32, hf16, pr, N_NEW) for pr in prompts]
    mb = LlamaForCausalLM.from_pretrained(d, device=dev)
    launches = _expect(kind, mb)
    mb.quest_init_batched(len(prompts), 16, 512, token_budget=16 * 1024)
    with torch.inference_mode():
        for i, pr in enumerate(prompts):
            lg = mb.prefill_sequence(i, pr.to(dev))
            _check(lg[0, -1], refs[i][0][1][-1], refs[i][0][0][-1], f"sequence {i} prefill, last position")
    with _CountLaunches() as count:
        mb.capture_decode_graph_batched()
    assert mb.fused_layers
    count.check_fused(launches == 5, mb.config.num_hidden_layers, batched=True)
    with torch.inference_mode():
        for t in range(N_NEW):
            ids = torch.tensor([refs[i][1][t] for i in range(len(prompts))], device=dev)
            out = mb.decode_graph_step_batched(ids)
            for i in range(len(prompts)):
                _check(out[i, -1], refs[i][2][t][1], refs[i][2][t][0], f"sequence {i} decode token {t}")


@pytest.mark.parametrize("kind", KINDS)
def test_sparse_path_eager_equals_graph_and_layouts_agree(tmp_path, kind):
    """Quest sparse path, budget 4 pages of 16 tokens: eager == graph replay of the module path, NHD == NHD_ROT, bit for
    bit; all logits finite."""
    from quest_amd.models.llama import LlamaForCausalLM

    d, _, _ = _checkpoint(tmp_path, kind)
    dev = torch.device(DEV)
    prompt = ((torch.arange(150)[None] * 37 + 11) % 320).to(dev)
    outs = []
    for graph, kv_layout in ((False, "NHD"), (True, "NHD"), (True, "NHD_ROT")):
        s = LlamaForCausalLM.from_pretrained(d, device=dev)
        s.quest_init(16, 512, token_budget=64, kv_layout=kv_layout)
        with torch.inference_mode():
            lg = s(input_ids=prompt)
            if graph:
                s.capture_decode_graph(fused_layers=False)
                assert not s.fused_layers
            seq = []
            for t in range(12):
                tk = lg[0, -1].argmax().view(1, 1)
                lg = s.decode_graph_step(input_ids=tk) if graph else s(input_ids=tk)
                seq.append(lg.float().clone())
        assert s.model.iController.need_estimate() or graph
        outs.append(torch.stack(seq))
        del s
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])
