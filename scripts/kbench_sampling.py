"""The device-side sampling launch against what callers did before, same process, A B A B (profiles/device_sampling.txt is this
script's output).

Part 1, the launch (``--launch``): HIP events around a hipGraph of ``--reps`` launches, logits L2-warm as behind an lm_head
    A  torch.argmax + embedding lookup + copy into the next step's input (the parent commit's device work; the host loop
       adds a device-to-host copy of the token on top)
    B  quest_sample_tokens, greedy (temperature 0), embedding row copied by the same launch
    C  quest_sample_tokens, temperature 0.8 / top_k 50 / top_p 0.9
at vocab {32000, 128256, 151936} x n {1, 8, 16}, fp16, normal(0, 3) logits.

Part 2, ms per generated token (``--e2e``): a random-weight model of Llama-2-7B shape, a synthetic cache of ``--ctx`` tokens
(as scripts/bench_textgen.py fills it), token budget 2048, fused layers; one sequence and eight
    A  decode_graph_step + argmax of the logits + the next id back into the step (the parent commit's loop)
    B  the step captured with a sampler (greedy): replay after replay, no device-to-host copy
wall clock around ``--tokens`` tokens ending in a device synchronise.

    python scripts/kbench_sampling.py [--launch] [--e2e] [--rounds 3] [--reps 20] [--tokens 64] [--ctx 32768]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = torch.device("cuda:0")


def graph_us(fn, reps, samples=5):
    """Median and (min, max) over `samples` timings of a captured graph of `reps` calls of fn: us per call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def launch_part(a):
    from quest_amd.utils import Sampler, SamplingParams

    hidden = 4096
    for vocab in (32000, 128256, 151936):
        embed = torch.randn(vocab, hidden, device=DEV).half()
        for n in (1, 8, 16):
            logits = (torch.randn(n, vocab, device=DEV) * 3).half()
            nxt = torch.empty(n, hidden, dtype=torch.float16, device=DEV)
            pos = torch.full((n,), 1000, dtype=torch.int32, device=DEV)
            greedy, sampled = Sampler(n, vocab, DEV), Sampler(n, vocab, DEV)
            for i in range(n):
                sampled.set_params(i, SamplingParams(0.8, 50, 0.9, 1234 + i))
            forms = {
                "A argmax+embedding+copy": lambda: nxt.copy_(torch.nn.functional.embedding(logits.argmax(-1), embed)),
                "B sample_tokens greedy": lambda: greedy.sample(logits, positions=pos, embed=embed, next_input=nxt),
                "C sample_tokens T0.8 k50 p0.9": lambda: sampled.sample(logits, positions=pos, embed=embed, next_input=nxt),
            }
            for rnd in range(a.rounds):
                for name, fn in forms.items():
                    med, lo, hi = graph_us(fn, a.reps)
                    print(f"launch vocab {vocab} n {n} round {rnd} {name}: {med:.2f} us (min {lo:.2f} max {hi:.2f})", flush=True)


def e2e_part(a):
    import quest_amd.utils as qu
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from quest_amd.utils import Sampler

    cfg = LlamaConfig(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=a.layers,
                      num_attention_heads=32, num_key_value_heads=32)
    for n in (1, 8):
        with torch.device(DEV):
            model = LlamaForCausalLM(cfg).half()
        for p in model.parameters():
            p.data.normal_(0, 0.02)
        for m in model.modules():
            if hasattr(m, "variance_epsilon"):
                m.weight.data.fill_(1.0)
        room = a.ctx + 256 + 2 * a.rounds * (a.tokens + 4)
        if n == 1:
            model.quest_init(16, room, 2048, kv_layout="NHD_ROT")
            ctl, seqs = model.model.iController, [model.model.iController]
        else:
            model.quest_init_batched(n, 16, room, 2048, kv_layout="NHD_ROT")
            ctl, seqs = model.model.bController, model.model.bController.seqs
        g = torch.Generator(device=DEV).manual_seed(1)
        k = torch.empty(a.ctx, 32, 128, dtype=torch.float16, device=DEV)
        v = torch.empty_like(k)
        for c in seqs:
            c.prepare_metadata(a.ctx)
            c.begin_forward(a.ctx)
            for l in range(a.layers):
                k.normal_(generator=g)
                v.normal_(generator=g)
                qu.append_kv(k, v, c, l)
            c.end_forward()
        del k, v
        capture = model.capture_decode_graph if n == 1 else model.capture_decode_graph_batched
        tok0 = torch.arange(n, device=DEV) + 5

        def host_loop():
            capture(fused_layers=True)
            step = (lambda t: model.decode_graph_step(input_ids=t.view(1, 1))) if n == 1 else model.decode_graph_step_batched
            tok = tok0
            with torch.inference_mode():
                for _ in range(4):
                    tok = step(tok).argmax(-1).view(-1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.tokens):
                    tok = step(tok).argmax(-1).view(-1)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.tokens

        def device_loop():
            sampler = Sampler(n, cfg.vocab_size, DEV, max_tokens=a.tokens + 4)
            capture(fused_layers=True, sampler=sampler)
            with torch.inference_mode():
                model.graph_input.copy_(model.model.embed_tokens(tok0).view(n, 1, -1))
            for _ in range(4):
                model._graph.replay()
                ctl.prepare_metadata(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.tokens):
                model._graph.replay()
                ctl.prepare_metadata(1)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.tokens

        for rnd in range(a.rounds):
            for name, fn in (("A host loop (decode_graph_step + argmax)", host_loop), ("B in-graph greedy sampling", device_loop)):
                print(f"e2e llama-2-7b shapes ctx {a.ctx} budget 2048 fused layers, {n} sequence(s), round {rnd} {name}: "
                      f"{fn():.4f} ms per generated token ({a.tokens} tokens)", flush=True)
        del model, ctl, seqs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_sampling needs the GPU"
    print(f"# {torch.cuda.get_device_name(0)}; A B A B in one process, medians of 5 timings with (min max)")
    if a.launch or not a.e2e:
        launch_part(a)
    if a.e2e or not a.launch:
        e2e_part(a)


if __name__ == "__main__":
    main()
