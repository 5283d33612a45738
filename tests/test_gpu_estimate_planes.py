"""The sign-plane estimate on the GPU (csrc/estimate_planes.hip): the shadow store after the build, the
planes launch against the pool launch and the CPU oracle, a planes controller against a twin without planes over a run of
tokens (eager and as a replayed graph), appends that do not maintain the planes, resets, controllers that get none.

H = Hkv = 4 (one case with 32), D = 128, S = 16; scored pages 1, 7, 8, 9 (edges of a lane's 8 pages), 127, 128, 129 (edges of
a workgroup's 128 pages) and 255, 256, 257, 300 (edges of a 256-page block of the store), last-page fill 1, 15, 16 (the appended token opens a page, lands inside one, completes one).
No tolerance anywhere: comparisons are on bit patterns (NaN scores: NaN against NaN, payloads not compared -- as
tests/test_gpu_estimate_semantics.py does)."""
import numpy as np
import pytest
import torch

import _estimate_cells as E
import _harness
import oracle

pytestmark = pytest.mark.gpu
D, S, BUDGET = 128, 16, 4
N_OUTS = [1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 300]
SENTINEL = 0x5A5A
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same(got_bits, want_bits, what):
    """Equal bit patterns where the expected score is not a NaN, a NaN where it is."""
    nan = (want_bits & 0x7fff) > 0x7c00
    assert np.array_equal((got_bits & 0x7fff) > 0x7c00, nan), what + ": NaN pattern"
    assert np.array_equal(got_bits[~nan], want_bits[~nan]), what


def _inputs(seed, L, H):
    """q [1, H, D], k / v [L, H, D] fp16 N(0,1) (numpy's generator: the pools here are a few million elements)."""
    rng = np.random.default_rng(seed)
    draw = lambda *shape: rng.standard_normal(shape, dtype=np.float32).astype(np.float16)
    return draw(1, H, D), draw(L, H, D), draw(L, H, D)


def _scratch(ctl):
    from quest_amd import _kernels

    t = torch.empty((ctl.num_heads, _kernels.tiles_row_stride(ctl.max_pages - 1)), dtype=torch.float16, device=DEV)
    t.view(torch.int16).fill_(SENTINEL)
    return t


def _prefilled(L, H, layout, k, v, pattern=None, seed=5, layers=1, Hkv=None, D_=D, dtype=None, room=4 * S):
    """A controller holding the first L tokens of k / v in every layer (one prefill append), device state enabled."""
    import quest_amd.utils as qu

    ctl = _harness.make_controller(L, H, H if Hkv is None else Hkv, D_, S, BUDGET, layout=layout, shuffle_seed=seed,
                                   max_seq_len=L + room, num_layers=layers)
    if pattern is not None:
        _harness.poison_pools(ctl, pattern)
    ctl.prepare_metadata(L)
    ctl.begin_forward(L)
    for l in range(layers):
        qu.append_kv(_harness.cuda(k[:L]), _harness.cuda(v[:L]), ctl, l)
    ctl.end_forward()
    ctl.enable_device_state()
    return ctl


def _covered(ctl):
    return ctl._planes_covered.cpu().tolist()


def _planes_view(ctl, layer=0):
    """[kv head][page block][feature][sign][page in block] uint16 view of a layer's store."""
    blocks = ctl._planes_pages // 256
    return _bits(ctl._planes[layer]).reshape(ctl.num_kv_heads, blocks, D, 2, 256)


def _expected_planes(ctl, n, layer=0):
    """hi / lo [n, H, D] uint16 of the first n logical pages, from the metadata pool: max / min by the order-preserving
    key (the metadata append writes holds no NaN; -0 < +0)."""
    kslot, vslot = _harness.gather_entries(ctl.metadata_cache.buf_layer(layer).cpu().numpy(), ctl.metadata_cache.indicies, n,
                                           ctl.layout)
    kb, vb = _u16(kslot), _u16(vslot)
    k_ge = E.half_keys(kb) >= E.half_keys(vb)
    return np.where(k_ge, kb, vb), np.where(k_ge, vb, kb)


def _check_planes(ctl, n, what, layer=0):
    hi, lo = _expected_planes(ctl, n, layer)
    got = _planes_view(ctl, layer)  # [H, blocks, D, 2, 256] -> [pages, H, D, 2]
    got = got.transpose(1, 4, 0, 2, 3).reshape(-1, ctl.num_kv_heads, D, 2)[:n]
    assert np.array_equal(got[..., 0], hi), what + ": max plane"
    assert np.array_equal(got[..., 1], lo), what + ": min plane"


# ------------------------------------------------------------------------------------------------ build

@pytest.mark.parametrize("pattern", [0, 0x7fff])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("fill", [1, 15, 16])
def test_build_transposes_the_complete_pages(layout, fill, pattern):
    H, L = 4, 300 * S + fill
    _, k, v = _inputs(11 + fill, L, H)
    ctl = _prefilled(L, H, layout, k, v, pattern=pattern)
    ctl.begin_graph_decode()
    assert ctl.estimate_planes_eligible() and ctl._planes_pages == 512
    n_full = 300 + (1 if fill == 16 else 0)
    assert _covered(ctl) == [n_full]
    _check_planes(ctl, n_full, f"layout {layout} fill {fill} pattern {pattern:#x}")
    ctl.clean_states()
    assert _covered(ctl) == [0]


# ------------------------------------------------------------------------------------------------ scores

def _planes_launch(ctl, kd, vd, qd, token, scores, must_be_planes=True):
    from quest_amd import _kernels

    mb = ctl.metadata_layer(0)
    assert (_kernels.estimate_planes_for(mb, ctl.meta_table_full, ctl.step_state) is not None) == must_be_planes
    assert _kernels.append_estimate_dyn(kd[token:token + 1], vd[token:token + 1], ctl.kv_layer(0), ctl.kv_table_full, qd, scores,
                                        mb, ctl.meta_table_full, ctl.step_state, ctl.max_pages - 1, ctl.layout)


def _pool_launch(ctl, qd):
    """Today's launch over the same state: scores only."""
    from quest_amd import _kernels

    o = _scratch(ctl)
    _kernels.estimate_attn_score_batched(qd, o.unsqueeze(0), ctl.metadata_layer(0), ctl.meta_tables, ctl.step_states,
                                         ctl.max_pages - 1, ctl.layout)
    return _bits(o)


def _oracle_scores(ctl, q, n_pages):
    """The oracle over the device's metadata bytes as they are now: scores of pages 0 .. n_pages - 2."""
    mc = ctl.metadata_cache
    n_meta = -(-n_pages // S)
    meta = oracle.Paged(mc.buf_layer(0).cpu().numpy(), np.array(mc.indicies[:n_meta], np.int32), (n_pages - 1) % S + 1, ctl.layout)
    return _u16(oracle.estimate(q, meta))


def _rewound(ctl, n):
    """Step state of the same cache when it had n + 1 pages, the last one full: n pages are scored, the appending launch
    writes the last token of page n again (the token that is already there: the pools do not change)."""
    table, mtable = ctl.kv_cache.indicies, ctl.metadata_cache.indicies
    return torch.tensor([(n + 1) * S, n + 1, S, table[n], n // S + 1, n % S + 1, mtable[n // S], 0], dtype=torch.int32)


def _score_case(H, layout, fill, hand_written=False, odd_q=False):
    import quest_amd.utils as qu

    what = f"H {H} layout {layout} fill {fill}"
    L = 300 * S + fill
    q, k, v = _inputs(40 + fill + layout, L, H)
    if odd_q:  # one head takes the pool path's literal form, the others stay on the planes
        q = q.copy()
        q[0, 1, 5], q[0, 1, 64], q[0, 1, 127] = 0.0, np.inf, np.nan
    ctl = _prefilled(L - 1, H, layout, k, v)
    if hand_written:  # both slots N(0,1) (K slot below V slot half the time), +-inf and NaN entries
        buf = ctl.metadata_cache.pool.buf
        rng = np.random.default_rng(fill)
        raw = rng.standard_normal(tuple(buf.shape), dtype=np.float32).astype(np.float16)
        flat = raw.reshape(-1)
        for val, frac in ((np.inf, 0.004), (-np.inf, 0.004), (np.nan, 0.002)):
            flat[rng.integers(0, flat.size, int(flat.size * frac))] = np.float16(val)
        buf.copy_(_harness.cuda(raw))
    ctl.begin_graph_decode()
    n_full0 = (L - 1) // S
    assert _covered(ctl) == [n_full0], what
    qu.step_advance_dyn(ctl)
    kd, vd, qd = _harness.cuda(k), _harness.cuda(v), _harness.cuda(q)
    live = ctl.step_state.clone()
    n_pages = int(live[1])
    assert n_pages == 301
    scores = _scratch(ctl)
    _planes_launch(ctl, kd, vd, qd, L - 1, scores)
    ctl.prepare_metadata(1)
    got = _bits(scores)
    want = _oracle_scores(ctl, q, n_pages)
    assert want.shape == (H, 300)
    _same(got[:, :300], want, what + ": planes launch against the oracle")
    assert (got[:, 300:] == SENTINEL).all(), what + ": columns beyond the live length"
    _same(got[:, :300], _pool_launch(ctl, qd)[:, :300], what + ": planes launch against the pool launch")
    # the token that completes a page carries the page into the planes and moves the counter on
    assert _covered(ctl) == [n_full0 + (1 if fill == S else 0)], what
    if not hand_written:
        kv_o, meta_o = _harness.oracle_pools(ctl, k, v)
        assert _harness.pools_match(ctl, kv_o, meta_o, L), what + ": pools after the appending launch"
        if fill == S:
            _check_planes(ctl, 301, what + ": planes after the completing append")
    # every shorter length over the same cache
    for n in N_OUTS[:-1]:
        ctl.step_state.copy_(_rewound(ctl, n))
        s_n = _scratch(ctl)
        _planes_launch(ctl, kd, vd, qd, (n + 1) * S - 1, s_n)
        got_n = _bits(s_n)
        # (hand-written metadata: the append folds the page's last token into the entry of page n again, which changes it --
        # and carries it into the planes; append-built metadata stays as it was)
        want_n = _oracle_scores(ctl, q, n + 1) if hand_written else want[:, :n]
        _same(got_n[:, :n], want_n, f"{what}: n_out {n} against the oracle")
        assert (got_n[:, n:] == SENTINEL).all(), f"{what}: n_out {n}: columns beyond the live length"
        _same(got_n[:, :n], _pool_launch(ctl, qd)[:, :n], f"{what}: n_out {n} against the pool launch")
    ctl.step_state.copy_(live)
    if not hand_written:
        assert _harness.pools_match(ctl, kv_o, meta_o, L), what + ": pools after the rewound launches"


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("fill", [1, 15, 16])
def test_planes_scores_equal_the_pool_launch_and_the_oracle(layout, fill):
    _score_case(4, layout, fill)


def test_planes_scores_32_heads():
    _score_case(32, 2, 16)


@pytest.mark.parametrize("layout,fill", [(0, 16), (1, 1), (2, 15)])
def test_planes_scores_on_hand_written_metadata(layout, fill):
    _score_case(4, layout, fill, hand_written=True)


@pytest.mark.parametrize("layout,fill", [(0, 15), (1, 16), (2, 1)])
def test_planes_scores_with_zero_inf_nan_in_one_heads_query(layout, fill):
    _score_case(4, layout, fill, odd_q=True)


# ------------------------------------------------------------------------------------------------ runs of tokens

def _twin_run(layout, graph, steps=40, L0=16 * 17 + 9, H=4, layers=2):
    """`steps` tokens of decode_layer_dyn on a planes controller and on a twin with estimate_planes = False: scores, outputs
    and pools bit-identical at every token, `covered` follows n_pages (three pages complete on the way)."""
    import quest_amd.utils as qu

    dev = torch.device(DEV)
    _, k0, v0 = _inputs(90 + layout, L0, H)
    g = torch.Generator(device=dev).manual_seed(7)
    new = [torch.randn(steps, layers, 1, H, D, generator=g, device=dev, dtype=torch.float16) for _ in range(3)]
    runs = []
    for planes in (True, False):
        ctl = _prefilled(L0, H, layout, k0, v0, seed=21, layers=layers, room=steps + 40)
        ctl.estimate_planes = planes
        ctl.begin_graph_decode()
        assert ctl._planes_registered == planes
        bufs = [torch.empty(layers, 1, H, D, device=dev, dtype=torch.float16) for _ in range(3)]
        scores = [qu.score_scratch(ctl) for _ in range(layers)]
        for s in scores:
            s.view(torch.int16).fill_(SENTINEL)
        outs = [None] * layers

        def step(ctl=ctl, bufs=bufs, scores=scores, outs=outs):
            qu.step_advance_dyn(ctl)
            for l in range(layers):
                outs[l] = qu.decode_layer_dyn(bufs[0][l], bufs[1][l], bufs[2][l], ctl, l, scores[l], apply_rope=True)

        replay = step
        if graph:
            for b, n in zip(bufs, new):
                b.copy_(n[0])
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            ctl.sync_device_state()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                step()
            replay = cg.replay
        runs.append((ctl, bufs, scores, outs, replay))
    completed = 0
    for t in range(steps):
        seen = []
        for ctl, bufs, scores, outs, replay in runs:
            for b, n in zip(bufs, new):
                b.copy_(n[t])
            replay()
            ctl.prepare_metadata(1)
            seen.append(([o.clone() for o in outs], [s.clone() for s in scores]))
        for l in range(layers):
            assert torch.equal(seen[0][0][l], seen[1][0][l]), f"token {t} layer {l}: outputs"
            assert np.array_equal(_bits(seen[0][1][l]), _bits(seen[1][1][l])), f"token {t} layer {l}: scores"
        a, b = runs[0][0], runs[1][0]
        assert a.kv_cache.indicies == b.kv_cache.indicies and a.metadata_cache.indicies == b.metadata_cache.indicies
        masks = _harness.valid_mask(a, a.kv_cache.seqlen)  # what the sequence owns: the rest of a pool is torch.empty's
        for pa, pb, m in zip(_harness._pools(a), _harness._pools(b), masks):
            ba, bb = _harness.pool_bits(pa), _harness.pool_bits(pb)
            assert all(np.array_equal(ba[l][m], bb[l][m]) for l in range(layers)), f"token {t}: pools"
        kv = a.kv_cache
        n_full = len(kv.indicies) - 1 + (1 if kv.last_page_len == S else 0)
        assert _covered(a) == [n_full] * layers, f"token {t}: covered"
        completed += kv.last_page_len == S
    assert completed == 3
    for l in range(layers):
        _check_planes(runs[0][0], len(runs[0][0].kv_cache.indicies) - 1, f"layer {l} after the run", layer=l)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("layout", [0, 2])
def test_planes_on_equals_planes_off_over_40_tokens(layout, graph):
    _twin_run(layout, graph)


def test_an_append_that_does_not_maintain_the_planes_leaves_covered_behind():
    import quest_amd.utils as qu
    from quest_amd import _kernels

    H, L0, dev = 4, 16 * 20 + 14, torch.device(DEV)
    q, k, v = _inputs(123, L0 + 40, H)
    ctl = _prefilled(L0, H, 0, k, v, room=80)
    ctl.begin_graph_decode()
    assert _covered(ctl) == [20]
    kd, vd, qd = _harness.cuda(k), _harness.cuda(v), _harness.cuda(q)
    mb = ctl.metadata_layer(0)

    def check(t, covered, what):
        want = _oracle_scores(ctl, q, len(ctl.kv_cache.indicies))
        n = want.shape[1]
        got = _bits(scores)
        _same(got[:, :n], want, f"token {t}: {what}")
        assert (got[:, n:] == SENTINEL).all(), f"token {t}: columns beyond the live length"
        assert _covered(ctl) == [covered], f"token {t}: covered"

    # tokens L0, L0 + 1 go in through the plain batched append: the second one completes page 20 behind the planes' back
    for t in (L0, L0 + 1):
        qu.step_advance_dyn(ctl)
        _kernels.append_kv_cache_decode_batched(kd[t:t + 1], vd[t:t + 1], ctl.kv_layer(0), ctl.kv_tables, mb, ctl.meta_tables,
                                                ctl.step_states, ctl.layout)
        ctl.prepare_metadata(1)
    assert _covered(ctl) == [20]
    # the planes launch goes on: page 20 is scored from the pool, covered stays behind, also across the next completion
    for t in range(L0 + 2, L0 + 2 + 20):
        qu.step_advance_dyn(ctl)
        scores = _scratch(ctl)
        _planes_launch(ctl, kd, vd, qd, t, scores)
        ctl.prepare_metadata(1)
        check(t, 20, "behind a gap")
    # begin_graph_decode closes the gap
    ctl.begin_graph_decode()
    n_full = len(ctl.kv_cache.indicies) - 1 + (1 if ctl.kv_cache.last_page_len == S else 0)
    assert n_full >= 22 and _covered(ctl) == [n_full]
    _check_planes(ctl, n_full, "after the rebuild")
    t = L0 + 22
    qu.step_advance_dyn(ctl)
    scores = _scratch(ctl)
    _planes_launch(ctl, kd, vd, qd, t, scores)
    ctl.prepare_metadata(1)
    check(t, n_full, "after the rebuild")


def test_reset_zeroes_covered_and_drops_the_registration():
    from quest_amd import _kernels

    H, L = 4, 16 * 9 + 3
    _, k, v = _inputs(5, L, H)
    ctl = _prefilled(L, H, 0, k, v)
    ctl.begin_graph_decode()
    mb, table, state = ctl.metadata_layer(0), ctl.meta_table_full, ctl.step_state
    assert _covered(ctl) == [9] and _kernels.estimate_planes_for(mb, table, state) is not None
    ctl.clean_states()
    assert _covered(ctl) == [0] and _kernels.estimate_planes_for(mb, table, state) is None
    # the next request: a new state, a new build
    ctl.prepare_metadata(L)
    ctl.begin_forward(L)
    import quest_amd.utils as qu

    qu.append_kv(_harness.cuda(k), _harness.cuda(v), ctl, 0)
    ctl.end_forward()
    ctl.enable_device_state()
    assert _kernels.estimate_planes_for(ctl.metadata_layer(0), ctl.meta_table_full, ctl.step_state) is None
    ctl.begin_graph_decode()
    assert _covered(ctl) == [9]
    ctl.invalidate_device_state()
    assert _covered(ctl) == [0]


def test_switched_off_by_the_environment(monkeypatch):
    H, L = 4, 16 * 9 + 3
    _, k, v = _inputs(5, L, H)
    monkeypatch.setenv("QUEST_ESTIMATE_PLANES", "0")
    ctl = _prefilled(L, H, 0, k, v)
    ctl.begin_graph_decode()
    assert not ctl._planes_registered and ctl._planes is None


def test_ineligible_controllers_have_no_planes():
    import quest_amd.utils as qu
    from quest_amd import _kernels

    L = 16 * 9 + 3
    for what, kw in (("GQA", dict(H=8, Hkv=2)), ("head_dim 64", dict(H=4, D_=64)), ("bf16", dict(H=4, dtype=torch.bfloat16))):
        H, Hkv, D_ = kw["H"], kw.get("Hkv", kw["H"]), kw.get("D_", D)
        _, k, v = _harness.inputs(5, L, H, Hkv, D_)
        if "dtype" in kw:
            import _bf16

            ctl = _bf16.make_controller(L, H, Hkv, D_, S, BUDGET)
            _bf16.fill(ctl, k, v, [L])
            ctl.end_forward()
            ctl.enable_device_state()
        else:
            ctl = _prefilled(L, H, 0, k, v, Hkv=Hkv, D_=D_)
        ctl.begin_graph_decode()
        assert not ctl.estimate_planes_eligible() and not ctl._planes_registered and ctl._planes is None, what
        assert _kernels.estimate_planes_for(ctl.metadata_layer(0), ctl.meta_table_full, ctl.step_state) is None, what
    b = qu.BatchedInferenceController(2, 1, 4, D, S, BUDGET, L + 4 * S, torch.float16, torch.device(DEV))
    for c in b.seqs:
        c.prepare_metadata(L)
        c.begin_forward(L)
        qu.append_kv(_harness.cuda(k[:, :4]), _harness.cuda(v[:, :4]), c, 0)
        c.end_forward()
    b.enable_device_state()
    b.begin_graph_decode()
    assert _kernels.estimate_planes_for(b.metadata_layer(0), b.meta_tables, b.step_states) is None, "batched"


def test_planes_allocated_under_inference_mode_are_reset_outside_it():
    """A model plans its decode graph under torch.inference_mode() and is cleared outside it: the store and its counter must
    be ordinary tensors, and the in-place updates of a reset and of sync_device_state() must work from either side."""
    H, L = 4, 16 * 9 + 3
    _, k, v = _inputs(5, L, H)
    ctl = _prefilled(L, H, 0, k, v)
    with torch.inference_mode():
        ctl.begin_graph_decode()
    assert _covered(ctl) == [9]
    ctl.sync_device_state()
    assert _covered(ctl) == [9]
    ctl.clean_states()
    assert _covered(ctl) == [0]
    ctl = _prefilled(L, H, 0, k, v)
    ctl.begin_graph_decode()
    with torch.inference_mode():
        ctl.sync_device_state()
        ctl.clean_states()
    assert _covered(ctl) == [0]
