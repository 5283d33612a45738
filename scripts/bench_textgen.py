#!/usr/bin/env python3
"""End-to-end decode latency of a Llama-architecture model with Quest attention vs full-KV attention
(the shape of the reference's scripts/bench_textgen.py:75-97 and README Fig. 10).

Random weights (no checkpoints offline) of Llama-2-7B shape by default; the KV cache of `--ctx` tokens is
filled with synthetic keys/values through append_kv -- or, with --real-prefill, by the reference harness's own prefill: one
model forward over `--ctx` random hidden states, timed (attention on the MFMA kernel of csrc/prefill.hip) --, then one
decode token -- RMSNorm, QKV GEMV, RoPE, [append+estimate | top-k+sparse attention | merge], o_proj, MLP,
lm_head -- is captured in a hipGraph and replayed.  First `skip` = 2 layers run dense like the reference
(quest/models/llama.py:428-439).

    python scripts/bench_textgen.py --ctx 32768 --token-budget 2048
    # Qwen3-8B shapes (per-head q/k norm, head_dim its own field); QUEST_FUSED_LAYER=0 takes the module path
    python scripts/bench_textgen.py --family qwen3 --layers 36 --heads 32 --kv-heads 8 --head-dim 128 --inter 12288 \
        --vocab 151936 --generate 64 [--seqs 8]
    # a bf16 model (weights, KV cache, metadata): its captured step takes the fused decoder layers (fused_layers=True, which a
    # bf16 model does not take by default); with QUEST_FUSED_LAYER=0 the same command times the module path
    python scripts/bench_textgen.py --dtype bf16 --generate 64 [--seqs 8]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def fused_layers_arg(a):
    """capture_decode_graph*'s fused_layers: the default for fp16 (on unless QUEST_FUSED_LAYER=0); bf16 fused layers are
    opt-in, so asked for here -- unless QUEST_FUSED_LAYER=0 asks for the module path"""
    return None if a.dtype == "f16" else os.environ.get("QUEST_FUSED_LAYER", "1") != "0"


def time_decode(model, ctl, emb, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.inference_mode():
        model(inputs_embeds=emb)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.inference_mode(), torch.cuda.graph(g):
        out = model(inputs_embeds=emb)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    return e0.elapsed_time(e1) / reps


def time_batched(cfg, a, dense, dev):
    """`--seqs` > 1: all sequences decode together, one hipGraph replay per token for the batch
    (LlamaForCausalLM.capture_decode_graph_batched).  dense = every layer full-KV (group-shared kernel)."""
    from quest_amd.models.llama import LlamaForCausalLM
    import quest_amd.utils as qu

    with torch.device(dev):
        model = LlamaForCausalLM(cfg).to(DTYPES[a.dtype])
    for p in model.parameters():
        p.data.normal_(0, 0.02)
    for m in model.modules():
        if hasattr(m, "variance_epsilon"):
            m.weight.data.fill_(1.0)
    model.quest_init_batched(a.seqs, 16, a.ctx + 256, a.token_budget, dtype=DTYPES[a.dtype], kv_layout=a.layout)
    if dense:
        model.model._quest_skip_layer = a.layers
    b = model.model.bController
    g = torch.Generator(device=dev).manual_seed(1)
    D = a.head_dim
    k = torch.empty(a.ctx, a.kv_heads, D, dtype=DTYPES[a.dtype], device=dev)
    v = torch.empty_like(k)
    for c in b.seqs:
        c.prepare_metadata(a.ctx)
        c.begin_forward(a.ctx)
        for l in range(a.layers):
            k.normal_(generator=g)
            v.normal_(generator=g)
            qu.append_kv(k, v, c, l)
        c.end_forward()
    del k, v
    model.capture_decode_graph_batched(fused_layers=fused_layers_arg(a))
    time_batched.fused_layers = bool(model.fused_layers)
    model.graph_input.copy_(torch.randn(a.seqs, 1, a.hidden, generator=g, device=dev, dtype=DTYPES[a.dtype]) * 0.1)
    for _ in range(3):
        model._graph.replay()
        b.prepare_metadata(1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        model._graph.replay()
        b.prepare_metadata(1)
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(model.graph_logits.float()).all()
    ms = e0.elapsed_time(e1) / a.reps
    del model, b
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--token-budget", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=32)
    ap.add_argument("--inter", type=int, default=11008)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layout", choices=["NHD", "HND", "NHD_ROT"], default="NHD_ROT",
                    help="pool layout (quest_init's kv_layout): the row-rotated NHD of round 6 by default, NHD = the reference's")
    ap.add_argument("--seqs", type=int, default=1, help="sequences decoded together (batched launches)")
    ap.add_argument("--checkpoint", default=None,
                    help="Hugging Face Llama checkpoint directory (config.json + safetensors) to load instead of "
                         "random-initialising; shapes come from its config.json")
    ap.add_argument("--make-checkpoint", default=None,
                    help="first WRITE a random-weight checkpoint of the given shape in HF layout to this directory "
                         "(save_pretrained), then load it back with from_pretrained and bench that model")
    ap.add_argument("--generate", type=int, default=0,
                    help="also generate this many tokens greedily by graph replay from the synthetic cache and report "
                         "ms/token over the whole run (host loop included)")
    ap.add_argument("--real-prefill", action="store_true",
                    help="fill the cache the way the reference's harness does (scripts/bench_textgen.py:77-84): ONE model "
                         "forward over --ctx random hidden states -- projections, RoPE, append with page metadata, the MFMA "
                         "prefill attention kernel, MLP in every layer -- and report its latency (time to first token)")
    ap.add_argument("--rope", choices=["default", "llama3"], default="default",
                    help="RoPE of the random-weight model: default (theta 1e4, the in-kernel formula) or Llama-3.1's "
                         "llama3 scaling (theta 5e5, factor 8: the kernels' frequency-table form)")
    ap.add_argument("--family", choices=["llama", "mistral", "qwen3"], default="llama",
                    help="model family of the random-weight model: mistral = Llama arithmetic, qwen3 = per-head q/k RMSNorm "
                         "before RoPE; both run their default RoPE through the frequency table (theta 1e6)")
    ap.add_argument("--head-dim", type=int, default=None, help="head dimension (default: hidden / heads)")
    ap.add_argument("--dtype", choices=["f16", "bf16"], default="f16",
                    help="element type of the weights, the KV cache and the metadata; bf16 captures with fused_layers=True")
    a = ap.parse_args()
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM
    import quest_amd.utils as qu

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=a.vocab, hidden_size=a.hidden, intermediate_size=a.inter, num_hidden_layers=a.layers,
                      num_attention_heads=a.heads, num_key_value_heads=a.kv_heads, max_position_embeddings=a.ctx + 1024,
                      head_dim=a.head_dim, qk_norm=a.family == "qwen3", model_type=a.family,
                      rope_theta=1e4 if a.family == "llama" else 1e6)
    a.head_dim = a.head_dim or a.hidden // a.heads
    if a.rope == "llama3":
        cfg.rope_scaling = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                            "original_max_position_embeddings": 8192}
        cfg.rope_theta = 500000.0
    ckpt_info = None
    if a.make_checkpoint:
        import time
        t0 = time.perf_counter()
        with torch.device(dev):
            tmp = LlamaForCausalLM(cfg).to(DTYPES[a.dtype])
        for p in tmp.parameters():
            p.data.normal_(0, 0.02)
        for m in tmp.modules():
            if hasattr(m, "variance_epsilon"):
                m.weight.data.fill_(1.0)
        tmp.save_pretrained(a.make_checkpoint)
        del tmp
        torch.cuda.empty_cache()
        a.checkpoint = a.make_checkpoint
        ckpt_info = {"written_s": time.perf_counter() - t0}
    if a.checkpoint:
        with open(os.path.join(a.checkpoint, "config.json")) as f:
            cfg = LlamaConfig.from_hf_dict(json.load(f))
        a.layers, a.hidden, a.heads, a.kv_heads = (cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads,
                                                   cfg.num_key_value_heads)
        a.head_dim, a.family = cfg.head_dim or a.hidden // a.heads, cfg.model_type
        ckpt_info = dict(ckpt_info or {}, path=a.checkpoint,
                         files=sorted(f for f in os.listdir(a.checkpoint) if f.endswith((".safetensors", ".json"))),
                         bytes=sum(os.path.getsize(os.path.join(a.checkpoint, f)) for f in os.listdir(a.checkpoint)))
    if a.seqs > 1:
        q_ms = time_batched(cfg, a, False, dev)
        d_ms = time_batched(cfg, a, True, dev)
        print(json.dumps({"bench": "e2e batched decode, random-weight Llama", "sequences": a.seqs, "ctx": a.ctx, "kv_layout": a.layout,
                          "token_budget": a.token_budget, "layers": a.layers, "hidden": a.hidden, "heads": a.heads,
                          "kv_heads": a.kv_heads, "intermediate": a.inter, "vocab": a.vocab, "dense_first_layers": 2,
                          "family": a.family, "head_dim": a.head_dim, "dtype": a.dtype,
                          "fused_decoder_layer_launches": getattr(time_batched, "fused_layers", None), "ms_per_step_quest": q_ms,
                          "ms_per_step_full_kv": d_ms, "tokens_per_s_quest": a.seqs / (q_ms * 1e-3),
                          "tokens_per_s_full_kv": a.seqs / (d_ms * 1e-3), "speedup": d_ms / q_ms}))
        return
    results = {}
    gen_ms = {}
    prefill_s = {}
    for name, budget in (("quest", a.token_budget), ("dense", 1 << 24)):
        if a.checkpoint:
            import time
            t0 = time.perf_counter()
            model = LlamaForCausalLM.from_pretrained(a.checkpoint, device=dev, dtype=DTYPES[a.dtype])
            ckpt_info["load_s"] = time.perf_counter() - t0
        else:
            with torch.device(dev):
                model = LlamaForCausalLM(cfg).to(DTYPES[a.dtype])
            for p in model.parameters():
                p.data.normal_(0, 0.02)
            for m in model.modules():
                if hasattr(m, "variance_epsilon"):
                    m.weight.data.fill_(1.0)
        model.quest_init(16, a.ctx + 256 + a.generate, budget, dtype=DTYPES[a.dtype], kv_layout=a.layout)
        ctl = model.model.iController
        g = torch.Generator(device=dev).manual_seed(1)
        D = a.head_dim
        if a.real_prefill:
            import time
            x = torch.randn(1, a.ctx, a.hidden, generator=g, device=dev, dtype=DTYPES[a.dtype])
            with torch.inference_mode():
                model(inputs_embeds=x[:, :256])  # warm the libraries' kernels on a short request, then start over
                model.quest_clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                first = model(inputs_embeds=x)
                torch.cuda.synchronize()
            prefill_s[name] = time.perf_counter() - t0
            assert torch.isfinite(first.float()).all() and ctl.kv_cache.seqlen == a.ctx
            del x, first
        else:
            ctl.prepare_metadata(a.ctx)
            ctl.begin_forward(a.ctx)
            k = torch.empty(a.ctx, a.kv_heads, D, dtype=DTYPES[a.dtype], device=dev)
            v = torch.empty_like(k)
            for l in range(a.layers):
                k.normal_(generator=g)
                v.normal_(generator=g)
                qu.append_kv(k, v, ctl, l)
            ctl.end_forward()
            del k, v
        emb = torch.randn(1, 1, a.hidden, generator=g, device=dev, dtype=DTYPES[a.dtype]) * 0.1
        results[name] = time_decode(model, ctl, emb, a.reps)
        if a.generate:
            # greedy generation by one graph replay per token (device-resident lengths; the host only feeds the token)
            import time
            model.capture_decode_graph(fused_layers=fused_layers_arg(a))
            gen_fused = bool(model.fused_layers)
            tok = torch.zeros(1, 1, dtype=torch.long, device=dev)
            with torch.inference_mode():
                for _ in range(3):
                    tok = model.decode_graph_step(input_ids=tok).argmax(-1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.generate):
                    tok = model.decode_graph_step(input_ids=tok).argmax(-1)
                torch.cuda.synchronize()
            gen_ms[name] = (time.perf_counter() - t0) * 1e3 / a.generate
        del model, ctl
        torch.cuda.empty_cache()
    out = {"bench": "e2e decode latency, random-weight Llama", "ctx": a.ctx, "token_budget": a.token_budget,
           "page_budget_pages": a.token_budget // 16, "layers": a.layers, "hidden": a.hidden, "heads": a.heads,
           "kv_heads": a.kv_heads, "dense_first_layers": 2, "kv_layout": a.layout, "rope": a.rope, "family": a.family,
           "head_dim": a.head_dim, "intermediate": a.inter, "vocab": a.vocab, "dtype": a.dtype,
           "ms_per_token_quest": results["quest"], "ms_per_token_full_kv": results["dense"],
           "speedup": results["dense"] / results["quest"],
           "reference_published": "RTX 6000 Ada, ctx 32768 FP16: 36.8 ms -> 21.2 ms @ budget 2048 (1.74x)"}
    if gen_ms:
        out["generation_fused_decoder_layers"] = gen_fused
        out["generated_tokens"] = a.generate
        out["ms_per_generated_token_quest"] = gen_ms["quest"]
        out["ms_per_generated_token_full_kv"] = gen_ms["dense"]
    if prefill_s:
        out["prefill_s_quest"] = prefill_s["quest"]  # the same work in both runs (prefill is dense): two samples
        out["prefill_s_full_kv"] = prefill_s["dense"]
        out["prefill"] = ("one model forward over ctx random hidden states, as the reference harness "
                          "(scripts/bench_textgen.py:77-84); attention = csrc/prefill.hip")
    if ckpt_info:
        out["checkpoint"] = ckpt_info
        out["bench"] = "e2e decode latency, Llama checkpoint in Hugging Face layout loaded with from_pretrained"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
