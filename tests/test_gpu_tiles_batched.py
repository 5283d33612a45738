"""The tiles launches for a BATCH (quest_append_estimate_batched + quest_decode_forward_fused_topk_batched with tile_max_offset != 0:
every row of the batched score scratch carries its own per-8-page maxima, csrc/decode_device.cuh sparse_decode_tiles_body
with blockIdx.z = sequence):

1. against the whole-row batched launches on the same caches, token after token: identical bits;
2. against the single-sequence tiles launches, per sequence;
3. against the oracle at cfg-4 row lengths (up to 8191 columns), four ragged sequences;
4. on crafted score rows with host-computed maxima, a different pattern and live length per sequence, tails poisoned;
5. the automatic policy of decode_layer_batched and its fall-backs;
6. a captured step replayed while the sequences grow, and a model generating with and without it."""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_long_rows import _half_keys, _row_patterns

pytestmark = pytest.mark.gpu
PAGE = 16
DEV = "cuda:0"
U16 = lambda a: np.ascontiguousarray(a).view(np.uint16)
# capacity of the small cases, in pages: beyond 1024 the whole-row launch gathers with 8-wave workgroups like the tiles
# launch (a head's pages are dealt over the waves: another wave count is another fp32 fold order)
CAP_PAGES = 1100


def _prefill(ctl, k, v, layers=1):
    import quest_amd.utils as qu

    L = k.shape[0]
    ctl.prepare_metadata(L)
    ctl.begin_forward(L)
    for l in range(layers):
        qu.append_kv(k, v, ctl, l)
    ctl.end_forward()


def _batch(lens, Hq, Hkv, D, B, layout, budgets=None, cap_tokens=PAGE * CAP_PAGES, seed=0, shuffle_seed=9, tiles_min_pages=1,
           keep_kv=False):
    """A one-layer BatchedInferenceController with ``lens[i]`` random tokens in sequence i, state on the device, planned."""
    import quest_amd.utils as qu

    dev = torch.device(DEV)
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    b = qu.BatchedInferenceController(len(lens), 1, Hq, D, PAGE, B, cap_tokens, torch.float16, dev, num_kv_heads=Hkv,
                                      layout=layout, shuffle_seed=shuffle_seed)
    if tiles_min_pages is not None:
        b.tiles_min_pages = tiles_min_pages
    kvs = []
    for i, L in enumerate(lens):
        k = torch.randn(L, Hkv, D, generator=g, device=dev, dtype=torch.float16)
        v = torch.randn(L, Hkv, D, generator=g, device=dev, dtype=torch.float16)
        _prefill(b.seqs[i], k, v)
        kvs.append((k, v) if keep_kv else None)
    if budgets is not None:
        b.set_page_budgets(budgets)
    b.enable_device_state()
    b.begin_graph_decode()
    return b, kvs


def _poisoned_scratch(b):
    """A score scratch whose every 16-bit word is 0xffff: as a tile key the largest there is, so a launch that read a
    maximum it had not been handed (a neighbour's row, a run beyond the live length) would select from it."""
    import quest_amd.utils as qu

    sc = qu.score_scratch(b)
    sc.view(torch.int16).fill_(-1)
    return sc


def _logical_pages(ctl, phys):
    if phys.numel() == 0:
        return torch.zeros(phys.shape, dtype=torch.int64)
    inv = {p: j for j, p in enumerate(ctl.kv_cache.indicies)}
    return torch.tensor([[inv[int(x)] for x in row] for row in phys.cpu().tolist()], dtype=torch.int64).reshape(phys.shape[0], -1)


RAGGED = [
    # Hq, Hkv, D, layout, starting lengths, planned budget (pages), per-sequence budgets
    # 2 sequences, HND, MHA
    (4, 4, 128, 1, (16 * 130 + 16, 16 * 30 + 5), 33, None),
    # 3 sequences, GQA: one 4.7 x another, one with fewer pages than the budget (it attends everything)
    (8, 2, 128, 0, (16 * 300 + 9, 16 * 64 + 1, 100), 20, None),
    # 5 sequences, row-rotated pool, head_dim 64, a budget per sequence (one above its sequence's page count); the third
    # sequence crosses a metadata-page boundary (256 tokens) mid-run, the fourth starts with ONE page (no row to select
    # from until its second page opens)
    (8, 8, 64, 2, (16 * 75 + 1, 16 * 16 + 3, 256 * 2 - 30, 5, 16 * 40 + 16), 9, (9, 4, 7, 9, 2)),
    # head_dim 256 (the estimate tile narrows to 4 kv heads so that it stays 8 pages wide)
    (8, 8, 256, 0, (16 * 90 + 5, 16 * 20 + 16, 256 - 20), 17, (17, 30, 5)),
    (16, 8, 256, 1, (16 * 70 + 16, 16 * 15 + 7), 12, None),
    (16, 16, 256, 2, (16 * 40 + 3, 16 * 9 + 9, 250), 7, (7, 3, 5)),
    # cfg-4 head shape, 200 selected pages; sequences below and above the budget, one 20 x another
    (32, 8, 128, 2, (16 * 260 + 1, 16 * 199 + 16, 16 * 50 + 3, 16 * 600 + 7, 30), 200, None),
    (32, 8, 128, 0, (16 * 260 + 1, 16 * 900 + 16, 16 * 50 + 3), 256, (256, 130, 256)),
]


@pytest.mark.parametrize("Hq,Hkv,D,layout,lens,B,budgets", RAGGED)
def test_batched_tiles_launches_equal_the_batched_whole_row_launches_while_the_sequences_grow(Hq, Hkv, D, layout, lens, B, budgets):
    """decode_layer_batched(one_launch=False, tiles=True) against tiles=False on the same caches (the append is
    idempotent), 70 tokens across KV-page and metadata-page boundaries: each sequence's live page scores, the selections
    and the outputs are identical bits -- both calls fold a head's pages in the same split (one plan, 8-wave gather)."""
    import quest_amd.utils as qu

    dev = torch.device(DEV)
    steps, n = 70, len(lens)
    if budgets is not None:
        B = max(B, max(budgets))
    b, _ = _batch(lens, Hq, Hkv, D, B, layout, budgets, seed=sum(lens) % 97)
    P = b.inference_page_budget
    h = b._decode_handler
    g = torch.Generator(device=dev).manual_seed(sum(lens) + B)
    sel = [(torch.zeros(n, Hq, P - 1, dtype=torch.float16, device=dev), torch.full((n, Hq, P - 1), -1, dtype=torch.int32, device=dev))
           for _ in range(2)]
    sc = [_poisoned_scratch(b), _poisoned_scratch(b)]
    assert sc[0].size(2) >= b.max_pages + (b.max_pages - 1 + 7) // 8
    for t in range(steps):
        q = torch.randn(n, Hq, D, generator=g, device=dev, dtype=torch.float16)
        k1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
        v1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
        qu.step_advance_batched(b)
        outs = []
        for i, tiles in enumerate((True, False)):
            h.set_selection_out(*sel[i])
            outs.append(qu.decode_layer_batched(q, k1, v1, b, 0, sc[i], one_launch=False, tiles=tiles))
            info = h.last_launch_info()
            assert (info["front_end_variant"] == 8) == tiles and info["n_seqs"] == n and info["waves"] == 8, (tiles, info)
            assert b.last_layer_launches == 2
        h.set_selection_out(None, None)
        b.prepare_metadata(1)
        for i, c in enumerate(b.seqs):
            n_live = len(c.kv_cache.indicies) - 1
            k_i = min((budgets[i] if budgets else P) - 1, n_live)
            assert torch.equal(sc[0][i, :, :n_live], sc[1][i, :, :n_live]), f"token {t} seq {i}: scores"
            assert torch.equal(sel[0][1][i, :, :k_i], sel[1][1][i, :, :k_i]), f"token {t} seq {i}: selected pages"
            assert torch.equal(sel[0][0][i, :, :k_i], sel[1][0][i, :, :k_i]), f"token {t} seq {i}: selected values"
            assert bool((sel[0][1][i, :, k_i:] == -1).all()), f"token {t} seq {i}: slots beyond the sequence's selection written"
        assert torch.equal(outs[0], outs[1]), f"token {t}: outputs"


@pytest.mark.parametrize("Hq,Hkv,D,layout,lens,B,budgets,ppc", [
    (8, 2, 128, 0, (16 * 300 + 9, 16 * 64 + 1, 100), 20, None, 4),
    (8, 8, 64, 2, (16 * 75 + 1, 16 * 16 + 3, 256 * 2 - 30, 5, 16 * 40 + 16), 9, (9, 4, 7, 9, 2), 0),
    (16, 8, 256, 1, (16 * 70 + 16, 16 * 15 + 7), 12, None, 0),    # ppc 0: each plan's own work split
    (32, 8, 128, 0, (16 * 260 + 1, 16 * 900 + 16, 16 * 50 + 3), 256, (256, 130, 256), 0),
])
def test_batched_tiles_launches_match_the_single_sequence_tiles_launches(Hq, Hkv, D, layout, lens, B, budgets, ppc):
    """Per sequence, the batched tiles launches against decode_layer_dyn(tiles=True) on that sequence alone (own pools,
    its own budget): page scores and selections bit for bit; outputs bit for bit where both plans put the same number of
    pages in a workgroup, else within 2e-3 (the bar include/quest_hip.h states for batched vs single)."""
    import quest_amd.utils as qu

    dev = torch.device(DEV)
    steps, n, cap = 12, len(lens), PAGE * CAP_PAGES
    g = torch.Generator(device=dev).manual_seed(77)
    ks = [torch.randn(L, Hkv, D, generator=g, device=dev, dtype=torch.float16) for L in lens]
    vs = [torch.randn(L, Hkv, D, generator=g, device=dev, dtype=torch.float16) for L in lens]
    b = qu.BatchedInferenceController(n, 1, Hq, D, PAGE, B, cap, torch.float16, dev, num_kv_heads=Hkv, layout=layout,
                                      shuffle_seed=9)
    b.tiles_min_pages = 1
    singles = []
    for i in range(n):
        _prefill(b.seqs[i], ks[i], vs[i])
        c = qu.InferenceController(1, Hq, D, PAGE, budgets[i] if budgets else B, cap, torch.float16, dev, num_kv_heads=Hkv,
                                   layout=layout, shuffle_seed=40 + i)
        _prefill(c, ks[i], vs[i])
        c.enable_device_state()
        if ppc:
            c._decode_handler.set_pages_per_chunk(ppc)
        c.begin_graph_decode()
        singles.append(c)
    if budgets is not None:
        b.set_page_budgets(budgets)
    b.enable_device_state()
    if ppc:
        b._decode_handler.set_pages_per_chunk(ppc)
    b.begin_graph_decode()
    P = b.inference_page_budget
    sel_b = torch.full((n, Hq, P - 1), -1, dtype=torch.int32, device=dev)
    sc_b = _poisoned_scratch(b)
    for t in range(steps):
        q = torch.randn(n, Hq, D, generator=g, device=dev, dtype=torch.float16)
        k1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
        v1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
        qu.step_advance_batched(b)
        b._decode_handler.set_selection_out(None, sel_b)
        o_b = qu.decode_layer_batched(q, k1, v1, b, 0, sc_b, one_launch=False, tiles=True)
        b._decode_handler.set_selection_out(None, None)
        assert b._decode_handler.last_launch_info()["front_end_variant"] == 8
        b.prepare_metadata(1)
        for i, c in enumerate(singles):
            P_i = c.inference_page_budget
            sel_s = torch.full((1, Hq, P_i - 1), -1, dtype=torch.int32, device=dev)
            sc_s = qu.score_scratch(c).zero_()
            qu.step_advance_dyn(c)
            c._decode_handler.set_selection_out(None, sel_s)
            o_s = qu.decode_layer_dyn(q[i:i + 1], k1[i:i + 1], v1[i:i + 1], c, 0, sc_s, tiles=True)
            c._decode_handler.set_selection_out(None, None)
            assert c._decode_handler.last_launch_info()["front_end_variant"] == 8
            c.prepare_metadata(1)
            n_live = len(c.kv_cache.indicies) - 1
            assert n_live == len(b.seqs[i].kv_cache.indicies) - 1
            k_i = min(P_i - 1, n_live)
            assert torch.equal(sc_b[i, :, :n_live], sc_s[:, :n_live]), f"token {t} seq {i}: scores"
            assert torch.equal(_logical_pages(b.seqs[i], sel_b[i, :, :k_i]), _logical_pages(c, sel_s[0, :, :k_i])), \
                f"token {t} seq {i}: selected pages"
            if ppc:
                assert torch.equal(o_b[i], o_s[0]), f"token {t} seq {i}: output bits"
            torch.testing.assert_close(o_b[i].float(), o_s[0].float(), rtol=2e-3, atol=2e-3)


def _gather_meta(buf_layer, indices, n_entries, layout):
    """Logical [n_entries, H, D] max / min rows of a metadata pool layer (device tensors)."""
    idx = torch.tensor(list(indices), device=buf_layer.device)
    pages = buf_layer[idx]
    if layout == 1:
        pages = pages.permute(0, 1, 3, 2, 4)
    if layout == 2:
        from quest_amd.utils.utils import TensorLayout

        pages = TensorLayout.to_logical(pages.view(torch.int16), 2).view(pages.dtype)
    m, _, S, H, D = pages.shape
    return pages[:, 0].reshape(m * S, H, D)[:n_entries], pages[:, 1].reshape(m * S, H, D)[:n_entries]


@pytest.mark.parametrize("layout", [0, 2])
def test_four_ragged_cfg4_sequences_against_the_oracle(layout):
    """4 sequences of BASELINE configs[3] head shape (Hq 32 / Hkv 8 / D 128) under one 8192-page capacity, 8192 / 8001 /
    6000 / 4100 pages long, budget 256 pages: one batched step through the tiles launches.  Metadata == per-page extrema;
    page scores and selected pages (values + ids) bit-exact against the oracle run on the device's metadata bytes;
    attention within 2e-3 of the oracle's fp64 attention over the selected pages."""
    import quest_amd.utils as qu

    Hq, Hkv, D, B = 32, 8, 128, 256
    pages = (8192, 8001, 6000, 4100)
    lens = tuple(p * PAGE - 6 for p in pages)  # the step's token is the 11th of each sequence's last page
    n = len(lens)
    dev = torch.device(DEV)
    b, kvs = _batch(lens, Hq, Hkv, D, B, layout, cap_tokens=8192 * PAGE + 64, seed=4, shuffle_seed=14, tiles_min_pages=None,
                    keep_kv=True)
    assert b.tiles_min_pages == 4097 and b.max_pages - 1 >= 4097 and not b.one_launch_layers
    g = torch.Generator(device=dev).manual_seed(5)
    q = torch.randn(n, Hq, D, generator=g, device=dev, dtype=torch.float16)
    k1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
    v1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
    sel_v = torch.zeros(n, Hq, B - 1, dtype=torch.float16, device=dev)
    sel_i = torch.full((n, Hq, B - 1), -1, dtype=torch.int32, device=dev)
    scores = _poisoned_scratch(b)
    h = b._decode_handler
    h.set_selection_out(sel_v, sel_i)
    qu.step_advance_batched(b)
    o = qu.decode_layer_batched(q, k1, v1, b, 0, scores)  # defaults: the policy picks the tiles launches at this capacity
    h.set_selection_out(None, None)
    b.prepare_metadata(1)
    info = h.last_launch_info()
    assert (info["keys_per_thread"], info["front_end_variant"], info["waves"], info["specialised"], info["n_seqs"]) == \
        (8, 8, 8, True, n), info
    meta_np = b.metadata_layer(0).cpu().numpy()
    kv_np = b.kv_layer(0).cpu().numpy()
    for i, c in enumerate(b.seqs):
        assert len(c.kv_cache.indicies) == pages[i] and c.kv_cache.seqlen == lens[i] + 1
        k_all = torch.cat([kvs[i][0], k1[i:i + 1]])
        full = (lens[i] + 1) // PAGE
        kp = k_all[:full * PAGE].view(full, PAGE, Hkv, D)
        mx, mn = _gather_meta(b.metadata_layer(0), c.metadata_cache.indicies, pages[i], layout)
        assert torch.equal(mx[:full], kp.amax(1)) and torch.equal(mn[:full], kp.amin(1)), f"seq {i}: metadata"
        assert torch.equal(mx[full], k_all[full * PAGE:].amax(0)) and torch.equal(mn[full], k_all[full * PAGE:].amin(0))
        meta = oracle.Paged(meta_np, np.asarray(c.metadata_cache.indicies, np.int32), c.metadata_cache.last_page_len, layout)
        q_np = q[i:i + 1].cpu().numpy()
        est = oracle.estimate(q_np, meta)
        table = np.asarray(c.kv_cache.indicies, np.int32)
        assert est.shape == (Hq, pages[i] - 1)
        assert np.array_equal(U16(scores[i, :, :pages[i] - 1].cpu().numpy()), U16(est)), f"seq {i}: page scores not bit-exact"
        ev, ei = oracle.topk(est, np.tile(table[:-1], (Hq, 1)), B - 1)
        assert np.array_equal(sel_i[i].cpu().numpy(), ei), f"seq {i}: selected pages differ from the oracle"
        assert np.array_equal(U16(sel_v[i].cpu().numpy()), U16(ev)), f"seq {i}: selected values"
        kv = oracle.Paged(kv_np, table, c.kv_cache.last_page_len, layout)
        eo, _ = oracle.sparse_attn(q_np, kv, ei, B - 1, int(table[-1]), c.kv_cache.last_page_len)
        np.testing.assert_allclose(o[i:i + 1].cpu().numpy().astype(np.float32), eo.astype(np.float32), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("with_budgets", [False, True])
def test_crafted_rows_per_sequence_select_the_oracles_pages(with_budgets):
    """Crafted score rows in a batched scratch with host-computed tile maxima: a different pattern (ties at the threshold,
    all-equal rows, a cluster of best pages, zeros of both signs and infinities) and a different live length per
    sequence, everything a launch must not read poisoned -- the columns and the maxima beyond each sequence's live
    length hold the largest key.  Per sequence the oracle's page list (values + ids, ascending column order)."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    Hq, Hkv, D, k = 4, 2, 64, 255
    cases = [(8192, "clustered"), (4100, "ties"), (6000, "equal"), (2041, "mixed"), (40, "normal"), (7001, "normal")]
    budgets = (256, 64, 256, 130, 256, 2) if with_budgets else None
    lens = tuple(p * PAGE - 5 for p, _ in cases)
    n = len(cases)
    dev = torch.device(DEV)
    b, _ = _batch(lens, Hq, Hkv, D, k + 1, 0, budgets, cap_tokens=8192 * PAGE + 64, seed=21, shuffle_seed=5)
    max_n = b.max_pages - 1
    off, stride = _kernels.tile_max_offset(max_n), _kernels.tiles_row_stride(max_n)
    rng = np.random.default_rng(91 + int(with_budgets))
    buf = np.full((n, Hq, stride), 0xffff, np.uint16)
    rows = []
    for i, (p, kind) in enumerate(cases):
        m = p - 1  # live columns: the cache already holds the "current" token
        r = np.stack([_row_patterns(rng, m, kind) for _ in range(Hq)])
        rows.append(r)
        buf[i, :, :m] = U16(r)
        n_tiles = (m + 7) // 8
        padded = np.zeros((Hq, n_tiles * 8), np.uint16)  # key 0 = below every real key: the invalid columns of the last tile
        padded[:, :m] = _half_keys(U16(r))
        buf[i, :, off:off + n_tiles] = padded.reshape(Hq, n_tiles, 8).max(axis=2)
    scores = torch.from_numpy(buf.view(np.float16)).to(dev)
    assert scores.size(2) == qu.score_scratch(b).size(2)
    g = torch.Generator(device=dev).manual_seed(3)
    q = torch.randn(n, Hq, D, generator=g, device=dev, dtype=torch.float16)
    h = b._decode_handler
    val = torch.zeros(n, Hq, k, dtype=torch.float16, device=dev)
    idx = torch.full((n, Hq, k), -1, dtype=torch.int32, device=dev)
    h.set_selection_out(val, idx)
    o = torch.empty_like(q)
    assert h.forward_fused_topk_batched(q, o, b.kv_layer(0), b.kv_tables, scores, b.step_states, max_n, b.page_budgets, tiles=True)
    h.set_selection_out(None, None)
    info = h.last_launch_info()
    assert info["front_end_variant"] == 8 and info["n_seqs"] == n and info["waves"] == 8, info
    for i, (p, kind) in enumerate(cases):
        table = np.array(b.seqs[i].kv_cache.indicies, np.int32)
        kk = min((budgets[i] if budgets else k + 1) - 1, p - 1)
        ev, ei = oracle.topk(rows[i], np.tile(table[:-1], (Hq, 1)), kk)
        assert np.array_equal(idx[i, :, :kk].cpu().numpy(), ei), f"seq {i} ({kind}): page ids"
        assert np.array_equal(U16(val[i, :, :kk].cpu().numpy()), U16(ev)), f"seq {i} ({kind}): values"
        assert bool((idx[i, :, kk:] == -1).all()), f"seq {i}: slots beyond the sequence's selection written"
    # the same rows through the whole-row launch (it ignores the maxima): identical slots -> identical bits
    o2 = torch.empty_like(q)
    h.forward_fused_topk_batched(q, o2, b.kv_layer(0), b.kv_tables, scores, b.step_states, max_n, b.page_budgets)
    info2 = h.last_launch_info()
    assert info2["front_end_variant"] != 8 and info2["waves"] == 8, info2
    assert torch.equal(o, o2)


def test_automatic_policy_and_fallbacks():
    """decode_layer_batched with defaults: tiles from ``tiles_min_pages`` pages up where the scratch has room and the
    largest budget selects at most 256 pages; otherwise the whole-row pair, with the same outputs; an ordinary small
    controller keeps its scratch shape and its launches."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    dev = torch.device(DEV)
    Hq, Hkv, D = 8, 2, 128
    lens = (16 * 300 + 9, 16 * 64 + 1, 100)
    n = len(lens)
    g = torch.Generator(device=dev).manual_seed(8)
    q = torch.randn(n, Hq, D, generator=g, device=dev, dtype=torch.float16)
    k1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
    v1 = torch.randn(n, Hkv, D, generator=g, device=dev, dtype=torch.float16)

    def step(b, scores, **kw):  # one token, decoded again by every call (the append is idempotent)
        m = b.n_seqs
        o = qu.decode_layer_batched(q[:m], k1[:m], v1[:m], b, 0, scores, one_launch=False, **kw)
        return o, b._decode_handler.last_launch_info()["front_end_variant"]

    # ordinary controller: default threshold 4097 pages, capacity 1100 -> nothing changes
    b, _ = _batch(lens, Hq, Hkv, D, 20, 0, tiles_min_pages=None)
    assert b.tiles_min_pages == 4097
    plain = qu.score_scratch(b)
    assert tuple(plain.shape) == (n, Hq, (b.max_pages + 7) // 8 * 8)
    qu.step_advance_batched(b)
    o_plain, variant = step(b, plain.zero_())
    assert variant != 8 and b.last_layer_launches == 2
    # threshold lowered: the scratch gets room and the default takes the tiles launches
    b.tiles_min_pages = 64
    roomy = qu.score_scratch(b)
    assert roomy.size(2) == _kernels.tiles_row_stride(b.max_pages - 1) > plain.size(2)
    o_tiles, variant = step(b, _poisoned_scratch(b))
    assert variant == 8 and torch.equal(o_tiles, o_plain)
    # ... a scratch allocated without room: the whole-row pair, same outputs (tiles=True cannot force it either)
    for kw in ({}, {"tiles": True}):
        o_fb, variant = step(b, plain.zero_(), **kw)
        assert variant != 8 and torch.equal(o_fb, o_plain)
    # ... tiles=False / a threshold above the capacity: the whole-row pair
    o_off, variant = step(b, roomy.zero_(), tiles=False)
    assert variant != 8 and torch.equal(o_off, o_plain)
    b.tiles_min_pages = b.max_pages
    o_off, variant = step(b, roomy.zero_())
    assert variant != 8 and torch.equal(o_off, o_plain)
    b.prepare_metadata(1)

    # a budget above 256 selected pages: outside the tiles launch -> the whole-row pair, default and forced
    lens2 = (16 * 700 + 3, 16 * 420 + 16)
    b2, _ = _batch(lens2, Hq, Hkv, D, 300, 0, tiles_min_pages=64, seed=2)
    assert b2.inference_page_budget - 1 > 256
    qu.step_advance_batched(b2)
    o_a, variant = step(b2, _poisoned_scratch(b2))
    assert variant != 8
    o_b, variant = step(b2, _poisoned_scratch(b2), tiles=True)
    assert variant != 8 and torch.equal(o_a, o_b)
    # the C entry itself refuses such a plan before anything is launched, and the wrapper reports it
    sc = _poisoned_scratch(b2)
    assert b2._decode_handler.forward_fused_topk_batched(q[:2], torch.empty_like(q[:2]), b2.kv_layer(0), b2.kv_tables, sc,
                                                         b2.step_states, b2.max_pages - 1, None, tiles=True) is False
    b2.prepare_metadata(1)


@pytest.mark.parametrize("Hq,Hkv,D,layout,lens,B,budgets", [RAGGED[1], RAGGED[2]])
def test_captured_batched_tiles_step_equals_eager_steps(Hq, Hkv, D, layout, lens, B, budgets):
    """A batched step through the tiles launches captured once and replayed while the sequences grow (KV pages and a
    metadata page open during the replay) equals the same steps issued eagerly on a twin batch: scores, outputs and step
    states bit for bit."""
    import quest_amd.utils as qu

    dev = torch.device(DEV)
    steps, n = 40, len(lens)
    if budgets is not None:
        B = max(B, max(budgets))
    seed = sum(lens) % 89
    bg, _ = _batch(lens, Hq, Hkv, D, B, layout, budgets, seed=seed, tiles_min_pages=64)
    be, _ = _batch(lens, Hq, Hkv, D, B, layout, budgets, seed=seed, tiles_min_pages=64)
    g = torch.Generator(device=dev).manual_seed(19)
    new_q = torch.randn(steps, n, Hq, D, generator=g, device=dev, dtype=torch.float16)
    new_k = torch.randn(steps, n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
    new_v = torch.randn(steps, n, Hkv, D, generator=g, device=dev, dtype=torch.float16)
    qb, kb, vb = torch.empty_like(new_q[0]), torch.empty_like(new_k[0]), torch.empty_like(new_v[0])
    ob = torch.empty_like(qb)
    sc_g, sc_e = _poisoned_scratch(bg), _poisoned_scratch(be)

    def step():
        qu.step_advance_batched(bg)
        qu.decode_layer_batched(qb, kb, vb, bg, 0, sc_g, one_launch=False, out=ob)

    qb.copy_(new_q[0]); kb.copy_(new_k[0]); vb.copy_(new_v[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up; the same token is folded again by the first replay (idempotent)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bg._decode_handler.last_launch_info()["front_end_variant"] == 8
    bg.sync_device_state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    bg.sync_device_state()
    for t in range(steps):
        qb.copy_(new_q[t]); kb.copy_(new_k[t]); vb.copy_(new_v[t])
        graph.replay()
        bg.prepare_metadata(1)
        qu.step_advance_batched(be)
        o_e = qu.decode_layer_batched(new_q[t], new_k[t], new_v[t], be, 0, sc_e, one_launch=False)
        assert be._decode_handler.last_launch_info()["front_end_variant"] == 8
        be.prepare_metadata(1)
        assert torch.equal(bg.step_states, be.step_states), f"token {t}: step states"
        for i, c in enumerate(be.seqs):
            n_live = len(c.kv_cache.indicies) - 1
            assert torch.equal(sc_g[i, :, :n_live], sc_e[i, :, :n_live]), f"token {t} seq {i}: scores"
        assert torch.equal(ob, o_e), f"token {t}: outputs"


def test_model_batched_generation_is_the_same_with_and_without_tiles(monkeypatch):
    """LlamaForCausalLM.quest_init_batched on a tiny random checkpoint reaches the tiles launches through score_scratch
    and decode_layer_batched alone (threshold lowered): same tokens and logits as the run with tiles off."""
    import quest_amd.utils as qu
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    dev = torch.device(DEV)
    cfg = LlamaConfig(vocab_size=256, hidden_size=512, intermediate_size=1024, num_hidden_layers=4,
                      num_attention_heads=4, num_key_value_heads=2)
    lens = (300, 215, 330)
    prompts = [((torch.arange(L, device=dev)[None] * (5 + 2 * i)) + i) % 256 for i, L in enumerate(lens)]
    n_new = 24

    def run(threshold):
        monkeypatch.setattr(qu.BatchedInferenceController, "tiles_min_pages", threshold, raising=False)
        torch.manual_seed(11)
        with torch.device(dev):
            m = LlamaForCausalLM(cfg).half()
        for p_ in m.parameters():
            p_.data.normal_(0, 0.05)
        # 1100 pages of capacity per sequence: the whole-row launch gathers with 8 waves like the tiles launch
        m.quest_init_batched(len(prompts), 16, PAGE * CAP_PAGES, token_budget=96)
        assert m.model.bController.tiles_min_pages == threshold
        with torch.inference_mode():
            ids = torch.tensor([int(m.prefill_sequence(i, pr).argmax(-1)) for i, pr in enumerate(prompts)], device=dev)
            m.capture_decode_graph_batched()
            toks, logits = [ids.tolist()], []
            for _ in range(n_new):
                out = m.decode_graph_step_batched(ids).float().clone()
                ids = out.argmax(-1).view(-1)
                toks.append(ids.tolist())
                logits.append(out)
        variant = m.model.bController._decode_handler.last_launch_info()["front_end_variant"]
        return toks, logits, variant

    toks_on, logits_on, v_on = run(8)
    toks_off, logits_off, v_off = run(1 << 30)
    assert v_on == 8 and v_off != 8
    assert toks_on == toks_off
    for a, c in zip(logits_on, logits_off):
        assert torch.equal(a, c)
