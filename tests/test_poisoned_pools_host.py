"""What the GPU tests of uninitialised pools compare against, fixed before any kernel is involved: the C oracle on numpy
pools pre-filled with a 16-bit pattern (a NaN, +inf of the element type) computes the bits it computes on zero pools and
writes only what ``valid_mask`` names; the mask helper itself; and the float64 restatement of the LSE against the C
oracle's.  The oracle is fp16: "bf16" here is fp16 data restricted to bf16 values (tests/_bf16.py) with bf16's patterns
(0x7f80, bf16's +inf, is one more NaN to the fp16 oracle)."""
import numpy as np
import pytest
import torch

import oracle
from oracle import synth, torch_ref
from _bf16 import mask3
from _harness import gather_entries, owned_mask, valid_mask

NAN16, INF_F16, INF_BF16 = 0x7FFF, 0x7C00, 0x7F80


def _controller(L, Hq, Hkv, D, S, layout, seed=3, extra_pages=3):
    import quest_amd.utils as qu

    ctl = qu.InferenceController(1, Hq, D, S, 4, L + extra_pages * S, torch.float16, "cpu", num_kv_heads=Hkv,
                                 layout=layout, shuffle_seed=seed)
    ctl.prepare_metadata(L)
    return ctl


def _paged(data, table, n_entries, S, layout):
    n = -(-n_entries // S)
    return oracle.Paged(data, np.array(table[:n], np.int32), (n_entries - 1) % S + 1, layout)


def _oracle_chain(ctl, pattern, q, k, v, chunks, budget):
    """Append k / v in ``chunks`` (pieces > 1 token: prefill append, 1 token: decode append) into pools pre-filled with
    ``pattern``, then estimate, top-k and sparse attention.  Returns every result and the two pools."""
    S, layout = ctl.page_size, ctl.layout
    kvd = np.full(tuple(ctl.kv_cache.buf_layer(0).shape), pattern, np.uint16).view(np.float16)
    md = np.full(tuple(ctl.metadata_cache.buf_layer(0).shape), pattern, np.uint16).view(np.float16)
    t = 0
    for n in chunks:
        t += n
        kv = _paged(kvd, ctl.kv_cache.indicies, t, S, layout)
        meta = _paged(md, ctl.metadata_cache.indicies, -(-t // S), S, layout)
        (oracle.append_prefill if n > 1 else oracle.append_decode)(kv, meta, k[t - n:t], v[t - n:t])
    assert t == k.shape[0]
    est = oracle.estimate(q, meta)
    table = np.asarray(kv.indices)
    sel_v, sel_i = oracle.topk(est, np.tile(table[:-1], (q.shape[1], 1)), budget - 1)
    o, lse = oracle.sparse_attn(q, kv, sel_i, sel_i.shape[1], int(table[-1]), kv.last_page_len)
    return {"est": est, "sel_v": sel_v, "sel_i": sel_i, "o": o, "lse": lse}, kvd, md


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else a.dtype)


# chunked prefill whose first chunk ends inside a page (the second reads the existing metadata entry), a decode append that
# continues a page and one that opens a page; page sizes 16 and 5; GQA and MHA
CASES = [
    # L, Hq, Hkv, D, S, chunks
    (16 * 6 + 2, 4, 2, 64, 16, (16 * 2 + 7, 16 * 4 - 7, 1, 1)),   # ... | to a page end | opens a page | continues it
    (5 * 9 + 1, 3, 3, 128, 5, (13, 31, 1, 1)),                    # page 5: 44 tokens, then one inside the page, one opening
    (16 * 5 + 16, 4, 2, 128, 16, (16 * 5 + 15, 1)),               # last page filled to its end by a decode append
]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("bf16,pattern", [(False, NAN16), (False, INF_F16), (True, NAN16), (True, INF_BF16)])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_oracle_ignores_and_keeps_stale_pool_bytes(case, bf16, pattern, layout):
    L, Hq, Hkv, D, S, chunks = CASES[case]
    assert sum(chunks) == L
    q, k, v = (synth.normal_f16(50 + case * 3 + i, shape) for i, shape in enumerate(((1, Hq, D), (L, Hkv, D), (L, Hkv, D))))
    if bf16:
        q, k, v = mask3(q), mask3(k), mask3(v)
    ctl = _controller(L, Hq, Hkv, D, S, layout)
    zero, kv0, m0 = _oracle_chain(ctl, 0, q, k, v, chunks, 4)
    pois, kv1, m1 = _oracle_chain(ctl, pattern, q, k, v, chunks, 4)
    for name in zero:
        assert np.array_equal(_bits(zero[name]), _bits(pois[name])), name
    assert np.isfinite(pois["est"].astype(np.float32)).all() and np.isfinite(pois["lse"]).all()
    kv_mask, meta_mask = valid_mask(ctl, L)
    for data, ref, mask in ((kv1, kv0, kv_mask), (m1, m0, meta_mask)):
        b = data.view(np.uint16)
        assert (b[~mask] == pattern).all(), "a byte outside the owned set was written"
        assert (b[mask] != pattern).all(), "an owned byte was not written"
        assert np.array_equal(b[mask], ref.view(np.uint16)[mask])
        assert (ref.view(np.uint16)[~mask] == 0).all()


@pytest.mark.parametrize("S,L", [(16, 1), (16, 16), (16, 17), (16, 16 * 17 + 3), (5, 23), (7, 7 * 8)])
def test_valid_mask_names_the_tokens_and_entries_of_the_sequence(S, L):
    Hq, Hkv, D = 4, 2, 64
    masks = {}
    for layout in (0, 1, 2):
        ctl = _controller(L, Hq, Hkv, D, S, layout)
        kvm, mm = masks[layout] = valid_mask(ctl, L)
        n_pages = -(-L // S)
        assert kvm.shape == tuple(ctl.kv_cache.buf_layer(0).shape) and mm.shape == tuple(ctl.metadata_cache.buf_layer(0).shape)
        assert kvm.sum() == L * 2 * Hkv * D and mm.sum() == n_pages * 2 * Hkv * D
        # the mask gathers exactly the logical rows gather_entries reads: mark them and read them back
        for mask, table, n in ((kvm, ctl.kv_cache.indicies, L), (mm, ctl.metadata_cache.indicies, n_pages)):
            marks = mask.astype(np.float16)
            kk, vv = gather_entries(marks, table, n, layout)
            assert kk.shape == (n, Hkv, D) and (kk == 1).all() and (vv == 1).all()
            used = sorted(set(np.nonzero(mask)[0].tolist()))
            assert used == sorted(table[:-(-n // S)])
    assert np.array_equal(masks[0][0], masks[2][0]) and np.array_equal(masks[0][1], masks[2][1])  # NHD_ROT == NHD
    assert np.array_equal(masks[0][0], masks[1][0].transpose(0, 1, 3, 2, 4))                      # HND: transposed
    # a shorter length of the same sequence owns a subset; the slots past it are outside
    kv_short, _ = valid_mask(_controller(L, Hq, Hkv, D, S, 0), max(1, L - 1))
    assert kv_short.sum() == max(1, L - 1) * 2 * Hkv * D and not (kv_short & ~masks[0][0]).any()


def test_valid_mask_of_a_shared_pool_is_the_union_of_disjoint_sequences():
    import quest_amd.utils as qu

    lens = (16 * 3 + 5, 7, 16 * 2 + 16)
    b = qu.BatchedInferenceController(len(lens), 1, 4, 64, 16, 4, 16 * 6, torch.float16, "cpu", num_kv_heads=2,
                                      shuffle_seed=2)
    for c, L in zip(b.seqs, lens):
        c.prepare_metadata(L)
    kvm, mm = valid_mask(b, lens)
    each = [valid_mask(c, L) for c, L in zip(b.seqs, lens)]
    assert kvm.sum() == sum(m[0].sum() for m in each) == sum(lens) * 2 * 2 * 64
    assert mm.sum() == sum(m[1].sum() for m in each) == sum(-(-L // 16) for L in lens) * 2 * 2 * 64
    assert owned_mask((4, 2, 16, 2, 8), 0, [3, 1], 17).sum() == 17 * 2 * 2 * 8


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("D,S,Hq,Hkv", [(64, 16, 4, 2), (128, 7, 3, 3), (256, 16, 4, 2)])
def test_lse_restatement_equals_the_c_oracle(D, S, Hq, Hkv, layout):
    """oracle/torch_ref.py lse_f64 (float64 numpy over the keys as stored in the pool) against the LSE the C oracle's sparse
    attention returns (accumulated in double, returned as float32): within one float32 rounding of the value."""
    L, budget = S * 9 + 3, 4
    q, k, v = (synth.normal_f16(80 + i, shape) for i, shape in enumerate(((1, Hq, D), (L, Hkv, D), (L, Hkv, D))))
    ctl = _controller(L, Hq, Hkv, D, S, layout)
    res, kvd, _ = _oracle_chain(ctl, NAN16, q, k, v, (L - 1, 1), budget)
    table = list(ctl.kv_cache.indicies)
    keys = []
    for h in range(Hq):
        pages = [int(p) for p in res["sel_i"][h]] + [table[-1]]
        rows = gather_entries(kvd, pages, (len(pages) - 1) * S + (L - 1) % S + 1, layout)[0]
        keys.append(rows[:, h // (Hq // Hkv)])
    want = torch_ref.lse_f64(q[0], np.stack(keys))
    assert np.isfinite(want).all()
    assert (np.abs(res["lse"].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    f32 = torch_ref.lse_f32(q[0], np.stack(keys).astype(np.float32)).numpy().astype(np.float64)
    assert np.abs(f32 - want).max() < 1e-4
