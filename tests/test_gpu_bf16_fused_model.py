"""bf16 checkpoints through the FUSED decoder-layer launches (``capture_decode_graph(fused_layers=True)``): the tiny
synthetic checkpoints of tests/test_gpu_bf16_model.py (Llama, llama3 RoPE, weights / keys / values beyond fp16's 65504) and
tests/test_gpu_model_families.py (Mistral, Qwen3), against transformers.

Yardstick: the project's bf16 one (tests/test_gpu_bf16_model.py), rel(got, hf_fp32) <= 1.5 * rel(hf_bf16, hf_fp32) + 2e-3
with hf_bf16 = transformers' own bf16 run on the same GPU.  The captured step is 4 projection launches per layer (5 with a
per-head q/k norm) and the fused final norm + lm_head, no nn.Linear; on the sparse path (budget 4 pages) the step run
eagerly == its replay and NHD == NHD_ROT, bit for bit.  The default (``fused_layers=None``) leaves a bf16 model on the module
path."""
import pytest
import torch

import test_gpu_bf16_model as L
import test_gpu_model_families as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
KINDS = ["llama", "mistral", "qwen3"]
N_NEW = 20  # 150 prompt tokens + 20: crosses the page boundary at 160


def _checkpoint(tmp_path, kind):
    """(directory, transformers fp32 on the CPU, transformers bf16 on the GPU) of the kind's tiny bf16 checkpoint"""
    return L._checkpoint(tmp_path) if kind == "llama" else F._checkpoint(tmp_path, kind, BF)


class _CountLinear:
    """Counts nn.Linear forward calls while a step is captured."""

    def __enter__(self):
        self.calls, self._saved = 0, torch.nn.Linear.forward

        def forward(mod, x, _fn=self._saved):
            self.calls += 1
            return _fn(mod, x)
        torch.nn.Linear.forward = forward
        return self

    def __exit__(self, *exc):
        torch.nn.Linear.forward = self._saved


def _capture_fused(m, batched):
    """Capture the fused step and check what it is made of: the launches per layer, the final norm + lm_head launch, no
    nn.Linear."""
    from quest_amd import _kernels

    qk_norm = m.model.layers[0].self_attn.qk_norm
    name = "decode_norm_gemv_batched" if batched else "decode_norm_gemv"
    head, saved = [0], getattr(_kernels, name)

    def norm_gemv(*a, **kw):
        head[0] += 1
        return saved(*a, **kw)
    setattr(_kernels, name, norm_gemv)
    try:
        with F._CountLaunches() as count, _CountLinear() as linear:
            (m.capture_decode_graph_batched if batched else m.capture_decode_graph)(fused_layers=True)
    finally:
        setattr(_kernels, name, saved)
    assert m.fused_layers is True
    count.check_fused(qk_norm, m.config.num_hidden_layers, batched=batched)  # 4 per layer, 5 with the q/k norm
    assert head[0] == 2 and linear.calls == 0, (head[0], linear.calls)        # (warm-up + recording)
    assert m.graph_input.dtype == BF and m.graph_logits.dtype == BF and m._graph_ws.h.dtype == BF
    ctl = m.model.bController if batched else m.model.iController
    assert ctl.one_launch_layers is False


@pytest.mark.parametrize("kind", KINDS)
def test_fused_bf16_single_sequence_matches_transformers(tmp_path, kind):
    from quest_amd.models.llama import LlamaForCausalLM

    d, hf32, hfbf = _checkpoint(tmp_path, kind)
    dev = torch.device(DEV)
    prompt = (torch.arange(150)[None] * 37 + 11) % 320
    first, toks, steps = F._hf_run(hf32, hfbf, prompt, N_NEW)
    m = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
    m.quest_init(16, 512, token_budget=16 * 1024, dtype=BF)  # budget >= pages: full attention, comparable with HF
    ctl = m.model.iController
    with torch.inference_mode():
        got_all = m.lm_head(m.model(input_ids=prompt.to(dev)))[0]
    L._check(got_all[-1], first[1][-1], first[0][-1], f"{kind} prefill, last position")
    if kind == "llama":  # the cache holds what fp16 cannot
        assert float(ctl.kv_cache.buf_layer(0)[ctl.kv_cache.indicies[0]].float().abs().max()) > 65504
        assert float(ctl.metadata_cache.buf_layer(0)[ctl.metadata_cache.indicies[0], 0, :2].float().abs().max()) > 65504
    _capture_fused(m, batched=False)
    for t in range(N_NEW):
        with torch.inference_mode():
            got = m.decode_graph_step(input_ids=torch.tensor([[toks[t]]], device=dev))
        L._check(got[0, -1], steps[t][1], steps[t][0], f"{kind} fused decode token {t}")
    assert ctl.kv_cache.seqlen == 150 + N_NEW


@pytest.mark.parametrize("kind", KINDS)
def test_fused_bf16_batch_of_three_matches_transformers(tmp_path, kind):
    from quest_amd.models.llama import LlamaForCausalLM

    d, hf32, hfbf = _checkpoint(tmp_path, kind)
    dev = torch.device(DEV)
    prompts = [((torch.arange(n)[None] * (7 + i) + i) % 320) for i, n in enumerate((150, 97, 201))]
    refs = [F._hf_run(hf32, hfbf, pr, N_NEW) for pr in prompts]
    mb = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
    mb.quest_init_batched(len(prompts), 16, 512, token_budget=16 * 1024, dtype=BF)
    with torch.inference_mode():
        for i, pr in enumerate(prompts):
            lg = mb.prefill_sequence(i, pr.to(dev))
            L._check(lg[0, -1], refs[i][0][1][-1], refs[i][0][0][-1], f"{kind} sequence {i} prefill, last position")
    _capture_fused(mb, batched=True)
    with torch.inference_mode():
        for t in range(N_NEW):
            ids = torch.tensor([refs[i][1][t] for i in range(len(prompts))], device=dev)
            out = mb.decode_graph_step_batched(ids)
            for i in range(len(prompts)):
                L._check(out[i, -1], refs[i][2][t][1], refs[i][2][t][0], f"{kind} sequence {i} fused decode token {t}")


def test_fused_bf16_sparse_path_eager_equals_replay_and_layouts_agree(tmp_path):
    """Budget 4 pages of 16 tokens on the checkpoint beyond fp16's range: the fused step run eagerly, its replay, and its
    replay over the row-rotated pool give the same logits bit for bit; all finite."""
    from quest_amd import _kernels
    from quest_amd.models.llama import LlamaForCausalLM

    d, _, _ = L._checkpoint(tmp_path)
    dev = torch.device(DEV)
    prompt = ((torch.arange(150)[None] * 37 + 11) % 320).to(dev)
    outs = []
    for replay, kv_layout in ((False, "NHD"), (True, "NHD"), (True, "NHD_ROT")):
        s = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
        s.quest_init(16, 512, token_budget=64, dtype=BF, kv_layout=kv_layout)
        ctl = s.model.iController
        with torch.inference_mode():
            lg = s(input_ids=prompt)
            s.capture_decode_graph(fused_layers=True)
            assert s.fused_layers is True
            seq = []
            for t in range(12):
                tk = lg[0, -1].argmax().view(1, 1)
                if replay:
                    lg = s.decode_graph_step(input_ids=tk)
                else:  # the captured step's own launches, issued eagerly: the fused layers, then final norm + lm_head
                    s.graph_input.copy_(s.model.embed_tokens(tk).view(1, 1, -1))
                    hs = s.model.forward_decode_fused(s.graph_input, s._graph_scores, ctl, s._graph_ws)
                    _kernels.decode_norm_gemv(hs, s.model.norm.weight, s.model.norm.variance_epsilon, s.lm_head.weight,
                                              s.graph_logits)
                    lg = s.graph_logits
                    torch.cuda.synchronize()
                    ctl.prepare_metadata(1)
                seq.append(lg.float().clone())
        assert ctl.kv_cache.seqlen == 150 + 12
        outs.append(torch.stack(seq))
        del s
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


def test_fused_bf16_sparse_path_batched_layouts_agree(tmp_path):
    from quest_amd.models.llama import LlamaForCausalLM

    d, _, _ = L._checkpoint(tmp_path)
    dev = torch.device(DEV)
    prompts = [((torch.arange(n)[None] * (7 + i) + i) % 320) for i, n in enumerate((150, 97, 201))]
    outs = []
    for kv_layout in ("NHD", "NHD_ROT"):
        s = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
        s.quest_init_batched(len(prompts), 16, 512, token_budget=64, dtype=BF, kv_layout=kv_layout)
        with torch.inference_mode():
            ids = torch.stack([s.prefill_sequence(i, pr.to(dev))[0, -1].argmax() for i, pr in enumerate(prompts)])
            s.capture_decode_graph_batched(fused_layers=True)
            assert s.fused_layers is True
            seq = []
            for t in range(12):
                lg = s.decode_graph_step_batched(ids)
                seq.append(lg.float().clone())
                ids = lg[:, -1].argmax(-1)
        outs.append(torch.stack(seq))
        del s
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_default_leaves_a_bf16_model_on_the_module_path(tmp_path):
    """``fused_layers=None``: on for fp16, off for bf16 -- bf16 fused layers are opt-in."""
    from quest_amd.models.llama import LlamaForCausalLM

    d, _, _ = F._checkpoint(tmp_path, "mistral", BF)
    dev = torch.device(DEV)
    m = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
    m.quest_init(16, 512, token_budget=16 * 1024, dtype=BF)
    with torch.inference_mode():
        m(input_ids=((torch.arange(40)[None] * 37 + 11) % 320).to(dev))
    with F._CountLaunches() as count:
        m.capture_decode_graph()
    assert m.fused_layers is False
    assert not any(v for n, v in count.calls.items() if n.startswith("decode_")), count.calls
