"""quest_sample_tokens on the GPU against the float64 restatement of its contract (tests/_sampling_ref.py): greedy rows bit
for bit, kept sets and tokens under the decidability rule stated there, invariance (alone / any row of a batch / states or
positions / graph replays), stop handling, history bounds, the embedding copy and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

import _sampling_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TORCH_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _logits(bits: np.ndarray, dtype: str) -> torch.Tensor:
    """``[n, V]`` stored bits -> a device tensor of rows V elements apart (an odd V leaves rows 2-byte aligned only)."""
    return torch.from_numpy(bits.view(np.int16).copy()).to(DEV).view(TORCH_DTYPE[dtype])


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)


def _f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _seeds(a):
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).to(DEV)


def _sample(bits, dtype, temperature, top_k, top_p, seed, pos, **kw):
    from quest_amd import _kernels

    n = bits.shape[0]
    tokens, kept = torch.full((n,), -5, dtype=torch.int32, device=DEV), torch.full((n,), -5, dtype=torch.int32, device=DEV)
    if "states" not in kw:
        kw["positions"] = _i32(pos)
    _kernels.sample_tokens(_logits(bits, dtype), _f32(temperature), _i32(top_k), _f32(top_p), _seeds(seed), tokens,
                           kept=kept, **kw)
    torch.cuda.synchronize()
    return tokens.cpu().numpy(), kept.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in ref.gpu_cases()])
def test_tokens_and_kept_follow_the_restatement(name):
    c = {c.name: c for c in ref.gpu_cases()}[name]
    tokens, kept = _sample(c.bits, c.dtype, c.temperature, c.top_k, c.top_p, c.seed, c.pos)
    rows = ref.case_rows(name)
    assert ((tokens >= 0) & (tokens < c.V)).all()
    problems = [f"row {i} (T {c.temperature[i]}, top_k {c.top_k[i]}, top_p {c.top_p[i]}): {msg}"
                for i, r in enumerate(rows) if (msg := ref.check_row(r, int(tokens[i]), int(kept[i])))]
    assert not problems, "\n".join(problems[:10])


def _special(dtype):
    return {"fp16": (0x3C00, 0x7C00, 0x7E00), "bf16": (0x3F80, 0x7F80, 0x7FC0)}[dtype]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("V", [1001, 9000])  # 4-wave and 16-wave workgroups; 1001 leaves the rows misaligned
def test_greedy_rows_are_bit_exact(dtype, V):
    one, inf, nan = _special(dtype)
    neg = lambda b: b | 0x8000
    base = ref.make_logits(31, 1, V, dtype)[0]
    rows, temps = [], []

    def add(edit, T):
        r = base.copy()
        edit(r)
        rows.append(r)
        temps.append(T)

    top = ref.to_bits(np.array([45.0], np.float32), dtype)[0]  # above every logit of the row
    add(lambda r: None, 0.0)
    add(lambda r: r.__setitem__([0, V - 1], top), 0.0)            # a tie between the first and the last column
    add(lambda r: r.__setitem__([V - 1, V // 2, 7], top), 0.0)    # ties: the lowest index
    add(lambda r: r.__setitem__(slice(None), one), 0.0)           # every column equal
    add(lambda r: r.__setitem__(V // 3, nan), 1.0)                # a NaN makes the row greedy whatever T says
    add(lambda r: r.__setitem__([V - 2, 5], nan), 0.7)
    add(lambda r: r.__setitem__(V // 3, neg(nan)), 1.0)           # a NaN with the sign set: greedy, and it sorts last
    add(lambda r: r.__setitem__([V - 1, 3], inf), 1.0)            # +inf
    add(lambda r: r.__setitem__(slice(None), neg(inf)), 1.0)      # a row of -inf: token 0
    add(lambda r: r.__setitem__(slice(None), neg(inf)), 0.0)
    add(lambda r: (r.__setitem__(slice(None), neg(0)), r.__setitem__([V - 1, V // 2], 0)), 0.0)  # -0 < +0
    add(lambda r: (r.__setitem__(slice(None), neg(inf)), r.__setitem__(V - 1, neg(one))), 0.0)
    bits = np.stack(rows)
    n = len(rows)
    tokens, kept = _sample(bits, dtype, temps, [0] * n, [1.0] * n, np.arange(n) + 1, [9] * n)
    for i in range(n):
        want = ref.sample_row(bits[i], dtype, temps[i], 0, 1.0, i + 1, 9)
        assert want.greedy, i
        assert (int(tokens[i]), int(kept[i])) == (want.token, 1), (i, int(tokens[i]), want.token)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("V", [3000, 20000])
def test_cuts_inside_runs_of_equal_logits_keep_the_lowest_indices(dtype, V):
    """Rows of few distinct values: the top-k threshold and the top-p cut fall inside a run of equal keys, of which the
    lowest token indices stay (the draw then shows which ones were kept)."""
    rng = np.random.default_rng(V)
    levels = ref.to_bits(np.array([0.0, 1.0, 2.0], np.float32), dtype)
    flat = np.full(V, levels[1], np.uint16)
    three = levels[rng.integers(0, 3, V)]
    sparse_top = np.full(V, levels[0], np.uint16)
    sparse_top[rng.choice(V, 40, replace=False)] = levels[2]
    # (top_p values that put the target mass half a token away from the nearest prefix: the cut is decided)
    cases = [(flat, 50, 1.0), (flat, 50, 0.53), (flat, 200, 0.5025), (three, 50, 1.0), (three, 700, 0.5307),
             (sparse_top, 50, 1.0), (sparse_top, 50, 0.93), (sparse_top, 37, 0.53)]
    bits = np.stack([np.stack([b] * 8) for b, _, _ in cases]).reshape(-1, V)  # 8 draws (seeds) per case
    k = np.repeat([k for _, k, _ in cases], 8)
    p = np.repeat([p for _, _, p in cases], 8).astype(np.float32)
    n = bits.shape[0]
    seeds, pos = np.arange(n) * 7919 + 1, np.arange(n) + 100
    tokens, kept = _sample(bits, dtype, [1.0] * n, k, p, seeds, pos)
    for i in range(n):
        want = ref.sample_row(bits[i], dtype, 1.0, int(k[i]), p[i], int(seeds[i]), int(pos[i]))
        assert want.boundary_decided, (i, "the crafted cut must be decided")
        assert not ref.check_row(want, int(tokens[i]), int(kept[i])), (i, ref.check_row(want, int(tokens[i]), int(kept[i])))
    assert len(set(tokens[:8].tolist())) > 1  # the seeds do draw different tokens from the 50 kept of a flat row


def _one_row_case(dtype="fp16", V=32000, n_params=16):
    c = {c.name: c for c in ref.gpu_cases()}[f"{dtype}-V{V}-n16"]
    return c


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_a_row_samples_the_same_alone_and_at_every_row_of_a_batch(dtype):
    c = _one_row_case(dtype)
    alone_t, alone_k = [], []
    picks = [i for i in range(c.n) if not ref.case_rows(c.name)[i].greedy and ref.case_rows(c.name)[i].kept > 1][:3]
    assert picks
    for i in picks:
        one = lambda a: np.asarray(a)[i:i + 1]
        t1, k1 = _sample(one(c.bits), dtype, one(c.temperature), one(c.top_k), one(c.top_p), one(c.seed), one(c.pos))
        rep = lambda a: np.repeat(np.asarray(a)[i:i + 1], 16, axis=0)
        # the other rows of the batch hold other logits: only the row under test is replicated into each position in turn
        for at in range(16):
            bits = c.bits.copy()
            T, K, P, S, POS = (np.array(a).copy() for a in (c.temperature, c.top_k, c.top_p, c.seed, c.pos))
            bits[at], T[at], K[at], P[at], S[at], POS[at] = c.bits[i], c.temperature[i], c.top_k[i], c.top_p[i], c.seed[i], c.pos[i]
            t16, k16 = _sample(bits, dtype, T, K, P, S, POS)
            assert (t16[at], k16[at]) == (t1[0], k1[0]), (i, at)
        t16, k16 = _sample(rep(c.bits), dtype, rep(c.temperature), rep(c.top_k), rep(c.top_p), rep(c.seed), rep(c.pos))
        assert (t16 == t1[0]).all() and (k16 == k1[0]).all()


def test_states_form_equals_positions_form():
    c = _one_row_case("fp16")
    t_pos, k_pos = _sample(c.bits, c.dtype, c.temperature, c.top_k, c.top_p, c.seed, c.pos)
    states = np.full((c.n, 8), 12345, np.int32)
    states[:, 0] = c.pos  # seq_len
    t_st, k_st = _sample(c.bits, c.dtype, c.temperature, c.top_k, c.top_p, c.seed, None, states=_i32(states))
    assert np.array_equal(t_pos, t_st) and np.array_equal(k_pos, k_st)
    # ... and the position does enter the draw
    t_other, _ = _sample(c.bits, c.dtype, c.temperature, c.top_k, c.top_p, c.seed, c.pos + 1)
    assert not np.array_equal(t_pos, t_other)


def test_three_replays_of_a_captured_launch_are_bit_equal():
    from quest_amd import _kernels

    c = _one_row_case("bf16")
    hidden = 256
    logits = _logits(c.bits, c.dtype)
    args = (_f32(c.temperature), _i32(c.top_k), _f32(c.top_p), _seeds(c.seed))
    pos = _i32(c.pos)
    tokens, kept = torch.zeros(c.n, dtype=torch.int32, device=DEV), torch.zeros(c.n, dtype=torch.int32, device=DEV)
    embed = torch.randn(c.V, hidden, device=DEV).to(torch.bfloat16)
    nxt = torch.zeros(c.n, hidden, dtype=torch.bfloat16, device=DEV)
    eos = _i32([3])
    call = lambda: _kernels.sample_tokens(logits, *args, tokens, positions=pos, kept=kept, embed=embed, next_input=nxt,
                                          eos_ids=eos)
    call()  # eager
    torch.cuda.synchronize()
    eager = (tokens.clone(), kept.clone(), nxt.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        tokens.fill_(-1), kept.fill_(-1), nxt.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tokens, eager[0]) and torch.equal(kept, eager[1]) and torch.equal(nxt, eager[2])
    assert torch.equal(nxt, embed[tokens.long()])


def test_finished_rows_emit_pad_and_eos_sets_the_flag():
    V, n = 1001, 4
    bits = ref.make_logits(77, n, V, "fp16")
    greedy = [int(ref.token_order(b)[0]) for b in bits]
    eos = [greedy[1], 5] if greedy[1] != 5 else [greedy[1], 6]
    assert greedy[2] not in eos and greedy[3] not in eos
    pad = 9
    finished = _i32([1, 0, 0, 7])  # rows 0 and 3 are finished already (any non-zero flag)
    history = torch.full((n, 4), -3, dtype=torch.int32, device=DEV)
    history_len = _i32([2, 0, 1, 0])
    tokens, kept = _sample(bits, "fp16", [0.0] * n, [0] * n, [1.0] * n, [1] * n, [5] * n, eos_ids=_i32(eos), pad_id=pad,
                           finished=finished, history=history, history_len=history_len)
    assert tokens.tolist() == [pad, greedy[1], greedy[2], pad]
    assert kept.tolist() == [0, 1, 1, 0]
    assert finished.tolist() == [1, 1, 0, 7]            # unchanged where set, set by the eos, clear otherwise
    assert history_len.tolist() == [2, 1, 2, 0]         # a finished row appends nothing
    h = history.cpu().numpy()
    assert h[1, 0] == greedy[1] and h[2, 1] == greedy[2] and (h[0] == -3).all() and (h[3] == -3).all()
    # without a flag array the eos ids have nothing to set and no row is skipped
    tokens, _ = _sample(bits, "fp16", [0.0] * n, [0] * n, [1.0] * n, [1] * n, [5] * n, eos_ids=_i32(eos), pad_id=pad)
    assert tokens.tolist() == greedy


def test_history_fills_to_its_stride_and_no_further():
    from quest_amd import _kernels

    V, n, stride = 65, 3, 3
    bits = ref.make_logits(78, n, V, "bf16")
    greedy = [int(ref.token_order(b)[0]) for b in bits]
    backing = torch.full((n * stride + 16,), -9, dtype=torch.int32, device=DEV)
    history = backing[:n * stride].view(n, stride)
    history_len = _i32([0, 1, 3])
    tokens = torch.zeros(n, dtype=torch.int32, device=DEV)
    logits = _logits(bits, "bf16")
    z = _f32([0.0] * n)
    for _ in range(5):
        _kernels.sample_tokens(logits, z, _i32([0] * n), _f32([1.0] * n), _seeds([0] * n), tokens, positions=_i32([1] * n),
                               history=history, history_len=history_len)
    torch.cuda.synchronize()
    assert history_len.tolist() == [stride] * n
    h = history.cpu().numpy()
    assert h[0].tolist() == [greedy[0]] * 3 and h[1].tolist() == [-9, greedy[1], greedy[1]] and h[2].tolist() == [-9] * 3
    assert (backing[n * stride:] == -9).all()  # nothing past the last row either
    # a negative length is left alone, too
    history_len.fill_(-1)
    _kernels.sample_tokens(logits, z, _i32([0] * n), _f32([1.0] * n), _seeds([0] * n), tokens, positions=_i32([1] * n),
                           history=history, history_len=history_len)
    torch.cuda.synchronize()
    assert history_len.tolist() == [-1] * n and np.array_equal(history.cpu().numpy(), h)


@pytest.mark.parametrize("dtype,hidden,offset", [("fp16", 256, 0), ("bf16", 4096, 0), ("fp16", 100, 0), ("bf16", 264, 3)])
def test_next_input_is_the_embedding_row_bit_for_bit(dtype, hidden, offset):
    """16-byte copies where rows allow them, 2-byte copies otherwise (hidden not a multiple of 8, or a misaligned base)."""
    V, n = 1001, 5
    bits = ref.make_logits(79, n, V, dtype)
    td = TORCH_DTYPE[dtype]
    table = torch.randn(V * hidden + 8, device=DEV).to(td)
    embed = table[offset:offset + V * hidden].view(V, hidden)
    out = torch.full((n * hidden + 16,), 7.0, device=DEV).to(td)
    nxt = out[offset:offset + n * hidden].view(n, hidden)
    tokens, _ = _sample(bits, dtype, [0.0, 1.0, 0.7, 0.0, 2.0], [0, 5, 0, 1, 50], [1.0, 0.9, 0.5, 1.0, 1.0], np.arange(n), [3] * n,
                        embed=embed, next_input=nxt)
    assert torch.equal(nxt.view(torch.int16), embed[torch.from_numpy(tokens).long().to(DEV)].view(torch.int16))
    assert (out[:offset] == 7.0).all() and (out[offset + n * hidden:] == 7.0).all()


def test_every_refusal_leaves_the_outputs_untouched():
    from quest_amd._lib import lib

    EINVAL, EUNSUPPORTED = -1, -2
    V, n, hidden = 1001, 2, 64
    logits = _logits(ref.make_logits(80, n, V, "fp16"), "fp16")
    big = torch.zeros(1, (1 << 18) + 1, dtype=torch.float16, device=DEV)
    t = {"temperature": _f32([1.0] * n), "top_k": _i32([0] * n), "top_p": _f32([1.0] * n), "seed": _seeds([1] * n),
         "positions": _i32([4] * n), "states": _i32(np.zeros((n, 8))), "tokens": torch.full((n,), -77, dtype=torch.int32, device=DEV),
         "kept": torch.full((n,), -77, dtype=torch.int32, device=DEV), "eos": _i32([1, 2]), "eos_bad": _i32([1, V]),
         "eos_neg": _i32([-1]), "eos9": _i32(list(range(9))), "finished": _i32([0] * n),
         "history": torch.full((n, 4), -77, dtype=torch.int32, device=DEV), "history_len": _i32([0] * n),
         "embed": torch.zeros(V, hidden, dtype=torch.float16, device=DEV),
         "next_input": torch.full((n, hidden), -77.0, dtype=torch.float16, device=DEV)}
    good = dict(logits=logits, stride=V, vocab=V, n=n, dtype=0, temperature="temperature", top_k="top_k", top_p="top_p",
                seed="seed", states=None, positions="positions", tokens="tokens", kept="kept", eos="eos", n_eos=2, pad=0,
                finished="finished", history="history", hstride=4, history_len="history_len", embed="embed", hidden=hidden,
                next_input="next_input")

    def call(**change):
        a = {**good, **change}
        p = lambda key: None if a[key] is None else t[a[key]].data_ptr()
        lg = a["logits"]
        return lib.quest_sample_tokens(None if lg is None else lg.data_ptr() + a.get("byte_offset", 0), a["stride"], a["vocab"],
                                       a["n"], a["dtype"], p("temperature"), p("top_k"), p("top_p"), p("seed"), p("states"),
                                       p("positions"), p("tokens"), p("kept"), p("eos"), a["n_eos"], a["pad"], p("finished"),
                                       p("history"), a["hstride"], p("history_len"), p("embed"), a["hidden"], p("next_input"),
                                       torch.cuda.current_stream().cuda_stream)

    refusals = [
        (dict(logits=None), EINVAL), (dict(temperature=None), EINVAL), (dict(top_k=None), EINVAL), (dict(top_p=None), EINVAL),
        (dict(seed=None), EINVAL), (dict(tokens=None), EINVAL),
        (dict(states="states"), EINVAL), (dict(positions=None), EINVAL),                # both / neither
        (dict(pad=-1), EINVAL), (dict(pad=V), EINVAL),
        (dict(eos="eos_bad"), EINVAL), (dict(eos="eos_neg", n_eos=1), EINVAL), (dict(eos="eos9", n_eos=9), EINVAL),
        (dict(eos=None), EINVAL),                                                       # n_eos 2 without ids
        (dict(dtype=2), EINVAL), (dict(vocab=0), EINVAL), (dict(n=0), EINVAL), (dict(stride=V - 1), EINVAL),
        (dict(byte_offset=1), EINVAL),
        (dict(history_len=None), EINVAL), (dict(history=None), EINVAL), (dict(hstride=0), EINVAL),
        (dict(next_input=None), EINVAL), (dict(embed=None), EINVAL), (dict(hidden=0), EINVAL),
        (dict(logits=big, stride=(1 << 18) + 1, vocab=(1 << 18) + 1, n=1), EUNSUPPORTED),
    ]
    for change, code in refusals:
        assert call(**change) == code, change
        torch.cuda.synchronize()
        for name in ("tokens", "kept", "history"):
            assert (t[name] == -77).all(), (change, name)
        assert (t["next_input"] == -77.0).all() and t["finished"].tolist() == [0] * n and t["history_len"].tolist() == [0] * n
    # the same arguments unchanged are served (and 2^18 columns are the largest row)
    assert call() == 0
    torch.cuda.synchronize()
    assert ((t["tokens"] >= 0) & (t["tokens"] < V)).all() and t["history_len"].tolist() == [1] * n
    assert call(logits=big, stride=(1 << 18) + 1, vocab=1 << 18, n=1, embed=None, next_input=None, hidden=0) == 0
    torch.cuda.synchronize()
