"""Group-shared page selection for GQA on the GPU (quest_decode_forward_group_topk, include/quest_hip.h): ONE selection per
kv head -- the key-max of its group's page scores, then the top-k contract -- attended by all heads of the group.

Selections are compared bit for bit with the numpy restatement (tests/_group_selection.py: ``oracle.half_key`` max over the
group, then ``oracle.topk``), read through ``quest_decode_set_selection_out``.  Outputs and ``lse`` are held to 2e-3 (the bar
include/quest_hip.h and tests/test_gpu_parity.py use against the fp64 oracle) against ``oracle.sparse_attn`` per head over the
selected pages and against ``quest_decode_forward`` fed the same pages as repeated per-head rows; bf16 outputs to the bar of
tests/test_gpu_bf16_kernels.py (atol 2e-3 + rtol 2^-8, one bf16 rounding of the output).  The score rows handed to the
eager entry are synthetic (``oracle/synth.py``) with crafted cross-head ties, signed zeros and NaN patterns: the entry takes
any 16-bit rows.  Pools are built by the project's own append through a controller and restated by the oracle."""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import synth

import _bf16
from _group_selection import expand, group_topk
from _harness import cuda, fill, inputs, make_controller, oracle_pools, poison_pools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAGE = 16
ATOL = 2e-3
BF_RTOL = 2.0 ** -8


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _craft(bits, group, hkv):
    """Synthetic score rows ``[Hq, n]`` (uint16 patterns) with, where the row is long enough: ties across the heads of kv
    head 0 on different columns, a kv head whose rows are one constant (the selection is its lowest columns) with signed
    zeros and NaN patterns among them."""
    hq, n = bits.shape
    if n < 8:
        return bits
    top = np.float16(6.5).view(np.uint16)
    bits[0, [1, 5]] = top                       # kv head 0: its first and last head tie on different pages
    bits[group - 1, [2, 5, 7]] = top
    if hkv > 1:
        rows = slice(group, 2 * group)          # kv head 1: everything ties at 1.0 ...
        bits[rows] = np.float16(1.0).view(np.uint16)
        bits[group, 0] = 0x8000                 # ... except -0 / +0 in one head (the others keep 1.0 there: the max wins)
        bits[group, 3] = 0x0000
        bits[rows, 4] = 0x8000                  # a column that is -0 in every head but one, +0 there
        bits[2 * group - 1, 4] = 0x0000
        bits[rows, 6] = 0xFE00                  # NaN, sign set, in every head: the smallest key of the row
        bits[2 * group - 1, n - 1] = 0x7E00     # NaN, sign clear, in one head: the largest key, at the last column
    return bits


@functools.lru_cache(maxsize=4)
def _sequence(L, hq, hkv, d, budget, layout=0, bf16=False, poison=None):
    """A controller filled with L tokens (left inside begin_forward of the last one: the handler is planned for the budget)
    and the oracle's restatement of its pools.  Cached: tests that share a shape share the pools and never write them."""
    q, k, v = (_bf16.inputs if bf16 else inputs)(L % 97 + 3, L, hq, hkv, d)
    if bf16:
        ctl = _bf16.make_controller(L, hq, hkv, d, PAGE, budget, layout=layout, shuffle_seed=3)
    else:
        ctl = make_controller(L, hq, hkv, d, PAGE, budget, layout=layout, shuffle_seed=3)
    if poison is not None:
        poison_pools(ctl, poison)
    if bf16:
        _bf16.fill(ctl, k, v, [L - 1, 1])
        kv_o, _ = _bf16.oracle_pools(ctl, k, v)
    else:
        fill(ctl, k, v)
        kv_o, _ = oracle_pools(ctl, k, v)
    return ctl, q, kv_o


def _score_rows(seed, hq, hkv, n, aligned, dtype):
    """(uint16 patterns ``[Hq, n]``, the device rows: a view of a buffer padded to 8 columns, or rows at an odd stride
    starting 2 bytes off an 8-byte boundary -- the scalar-load front end)."""
    bits = _craft(synth.normal_f16(seed, (hq, n)).view(np.uint16).copy(), hq // hkv, hkv)
    if dtype == torch.bfloat16:
        bits &= np.uint16(0xFFF8)  # (any patterns would do; these are bf16 values of the same order)
    stride = (n + 7) // 8 * 8 if aligned else n | 1
    buf = torch.zeros(hq * stride + 8, dtype=torch.int16, device=DEV)
    rows = buf[(0 if aligned else 1):][:hq * stride].view(hq, stride)[:, :n]
    rows.copy_(torch.from_numpy(bits.view(np.int16)).to(DEV))
    return bits, rows.view(dtype)


class _Run:
    """One eager launch on ``ctl`` and everything it wrote."""

    def __init__(self, ctl, q_np, score_rows, ppc=None, dtype=torch.float16):
        h = ctl._decode_handler
        self.hq, self.hkv = ctl.num_heads, ctl.num_kv_heads
        self.n = len(ctl.kv_cache.indicies) - 1
        self.k = ctl.inference_page_budget - 1
        if ppc is not None:  # re-plan with a forced split
            h.set_pages_per_chunk(ppc)
            h.begin_forward(torch.tensor([0, self.k], dtype=torch.int32), self.hq, self.hkv, ctl.head_dim, PAGE, dtype)
        self.q = _bf16.dev16(q_np) if dtype == torch.bfloat16 else cuda(q_np)
        # outputs inside guarded buffers: what lies around them must stay untouched
        self._o = torch.full((3, self.hq, ctl.head_dim), 77.0, dtype=dtype, device=DEV)
        self._lse = torch.full((3, self.hq), 77.0, dtype=torch.float32, device=DEV)
        self._idx = torch.full((3, self.hkv, self.k), -7, dtype=torch.int32, device=DEV)
        self._val = torch.full((3, self.hkv, self.k), 77.0, dtype=dtype, device=DEV)
        h.set_selection_out(self._val[1:2], self._idx[1:2])
        h.lse_out = self._lse[1]
        try:
            self.ok = h.forward_group_topk(self.q, self._o[1:2], ctl.kv_layer(0), ctl.kv_indices_with_last, score_rows, None,
                                           self.n, paged_kv_last_page_len=ctl.kv_cache.last_page_len,
                                           paged_kv_last_page_idx=ctl.kv_last_page_idx)
            self.info = h.last_launch_info()
        finally:
            h.set_selection_out(None, None)
            h.lse_out = None
            if ppc is not None:
                h.set_pages_per_chunk(0)
                h.begin_forward(torch.tensor([0, self.k], dtype=torch.int32), self.hq, self.hkv, ctl.head_dim, PAGE, dtype)
        torch.cuda.synchronize()
        self.o, self.lse, self.idx, self.val = self._o[1], self._lse[1], self._idx[1], self._val[1]

    def guards_intact(self):
        return all(bool((t[0] == fill).all()) and bool((t[2] == fill).all())
                   for t, fill in ((self._o, 77.0), (self._lse, 77.0), (self._idx, -7), (self._val, 77.0)))


def _check(ctl, q_np, kv_o, bits, run, dtype=torch.float16):
    """Selection bit-exact against the restatement; o / lse against the oracle per head and against quest_decode_forward
    fed the same pages as repeated per-head rows."""
    group = run.hq // run.hkv
    table = np.array(ctl.kv_cache.indicies, np.int32)
    assert run.ok and run.info["front_end_variant"] == 9 and run.info["n_seqs"] == 1
    assert run.guards_intact()
    want_v, want_i = group_topk(bits.view(np.float16), table, group, run.k)
    assert np.array_equal(run.idx.cpu().numpy(), want_i), "selected pages"
    assert np.array_equal(_bits(run.val), want_v.view(np.uint16)), "selected values"
    # the oracle, per head over the group's pages
    e_o, e_lse = oracle.sparse_attn(q_np, kv_o, expand(want_i, group), run.k, int(table[-1]), ctl.kv_cache.last_page_len)
    e_o = e_o[0].astype(np.float32)
    if dtype == torch.bfloat16:
        got = _bf16.bf16_bits_to_f32(_bits(run.o))
        err, bound = np.abs(got - e_o), ATOL + BF_RTOL * np.abs(e_o)
    else:
        err, bound = np.abs(run.o.cpu().numpy().astype(np.float32) - e_o), ATOL
    lse_err = np.abs(run.lse.cpu().numpy() - e_lse).max()
    print(f"group selection {dtype} Hq {run.hq} Hkv {run.hkv} D {ctl.head_dim} n {run.n} k {run.k} workgroups "
          f"{run.info['workgroups_per_head']}: o max abs err {err.max():.3e} lse max abs err {lse_err:.3e}")
    assert (err <= bound).all(), float(err.max())
    assert lse_err <= ATOL, lse_err
    # quest_decode_forward over the same pages as repeated per-head rows
    h = ctl._decode_handler
    o2 = torch.empty_like(run.q)
    lse2 = torch.empty(run.hq, dtype=torch.float32, device=DEV)
    rows = cuda(expand(want_i, group))
    h.lse_out = lse2
    try:
        h.forward(run.q, o2, ctl.kv_layer(0), rows, ctl.kv_indptr_for_approx_decode, ctl.kv_cache.last_page_len,
                  ctl.kv_last_page_idx)
    finally:
        h.lse_out = None
    d = (run.o.float() - o2[0].float()).abs()
    tol = ATOL + (BF_RTOL * o2[0].float().abs() if dtype == torch.bfloat16 else 0.0)
    assert bool((d <= tol).all()), float(d.max())
    assert float((run.lse - lse2).abs().max()) <= ATOL
    return want_i


# (pages of the sequence, page budget): k = min(budget - 1, pages - 1) selected pages + the current one.  (2, 4): budget >
# pages, everything is attended; (1000, 257): the envelope's 256 selected pages; (4097, 128): the row limit's last column
CASES = [(2, 4), (9, 4), (130, 33), (257, 128), (1000, 256), (1000, 257), (4096, 128), (4097, 128)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("group,hkv", [(1, 3), (2, 2), (4, 3), (8, 2)])
@pytest.mark.parametrize("pages,budget", CASES[:4])
def test_selection_and_outputs_small_rows(pages, budget, group, hkv, d):
    L = (pages - 1) * PAGE + 5
    ctl, q, kv_o = _sequence(L, group * hkv, hkv, d, budget)
    for aligned in (True, False):
        bits, rows = _score_rows(pages + group, group * hkv, hkv, pages - 1, aligned, torch.float16)
        _check(ctl, q, kv_o, bits, _Run(ctl, q, rows))


@pytest.mark.parametrize("pages,budget,group,hkv,d", [
    (1000, 256, 4, 2, 128), (1000, 257, 2, 2, 64), (4096, 128, 2, 2, 64), (4097, 128, 8, 2, 64), (4097, 128, 1, 2, 64)])
def test_selection_and_outputs_long_rows(pages, budget, group, hkv, d):
    L = (pages - 1) * PAGE + 16
    ctl, q, kv_o = _sequence(L, group * hkv, hkv, d, budget)
    for aligned in (True, False):
        bits, rows = _score_rows(pages, group * hkv, hkv, pages - 1, aligned, torch.float16)
        run = _Run(ctl, q, rows)
        _check(ctl, q, kv_o, bits, run)
        if budget == 257:
            assert run.info["workgroups_per_head"] >= 2  # 257 slots: more than one workgroup's LDS list


def test_work_splits_select_the_same_pages():
    """One workgroup per kv head, one page per workgroup (the generic merge: 33 partials), two workgroups (the fast merge)."""
    pages, budget, group, hkv, d = 130, 33, 4, 2, 128
    ctl, q, kv_o = _sequence((pages - 1) * PAGE + 5, group * hkv, hkv, d, budget)
    bits, rows = _score_rows(5, group * hkv, hkv, pages - 1, True, torch.float16)
    picked = []
    for ppc, chunks in ((budget, 1), (1, budget), (17, 2), (None, None)):
        run = _Run(ctl, q, rows, ppc=ppc)
        if chunks is not None:
            assert run.info["workgroups_per_head"] == chunks
        picked.append(_check(ctl, q, kv_o, bits, run))
    assert all(np.array_equal(p, picked[0]) for p in picked)


@pytest.mark.parametrize("fill_len", [1, 15, 16])
def test_last_page_fill(fill_len):
    pages, budget, group, hkv, d = 40, 9, 4, 2, 128
    ctl, q, kv_o = _sequence((pages - 1) * PAGE + fill_len, group * hkv, hkv, d, budget)
    assert ctl.kv_cache.last_page_len == fill_len
    bits, rows = _score_rows(fill_len, group * hkv, hkv, pages - 1, True, torch.float16)
    _check(ctl, q, kv_o, bits, _Run(ctl, q, rows))


@pytest.mark.parametrize("group,hkv,d", [(4, 4, 128), (2, 3, 64)])
def test_layouts_give_the_same_selection_and_the_same_bits(group, hkv, d):
    pages, budget = 70, 17
    got = []
    for layout in (0, 1, 2):  # NHD, HND, NHD_ROT: the same shuffle seed hands out the same physical pages
        ctl, q, kv_o = _sequence((pages - 1) * PAGE + 7, group * hkv, hkv, d, budget, layout=layout)
        bits, rows = _score_rows(9, group * hkv, hkv, pages - 1, True, torch.float16)
        run = _Run(ctl, q, rows, ppc=5)
        _check(ctl, q, kv_o, bits, run)
        got.append((run.idx.cpu(), _bits(run.o), run.lse.cpu()))
    for idx, o, lse in got[1:]:
        assert torch.equal(idx, got[0][0]) and np.array_equal(o, got[0][1]) and torch.equal(lse, got[0][2])


@pytest.mark.parametrize("group,hkv,d", [(1, 3, 128), (2, 2, 64), (4, 2, 128), (8, 2, 128)])
def test_bf16(group, hkv, d):
    pages, budget = 130, 33
    ctl, q, kv_o = _sequence((pages - 1) * PAGE + 5, group * hkv, hkv, d, budget, bf16=True)
    for aligned in (True, False):
        bits, rows = _score_rows(group, group * hkv, hkv, pages - 1, aligned, torch.bfloat16)
        _check(ctl, q, kv_o, bits, _Run(ctl, q, rows, dtype=torch.bfloat16), dtype=torch.bfloat16)


def test_nan_filled_pools_give_the_bits_of_zero_filled_pools_and_nothing_else_is_written():
    pages, budget, group, hkv, d = 70, 17, 4, 2, 128
    L = (pages - 1) * PAGE + 3  # 13 stale rows in the current page
    res = []
    for poison in (0x0000, 0x7FFF):
        ctl, q, kv_o = _sequence(L, group * hkv, hkv, d, budget, poison=poison)
        before = [p.buf.clone() for p in (ctl.kv_cache.pool, ctl.metadata_cache.pool)]
        bits, rows = _score_rows(21, group * hkv, hkv, pages - 1, True, torch.float16)
        rows_before = rows.clone()
        run = _Run(ctl, q, rows, ppc=5)
        _check(ctl, q, kv_o, bits, run)
        # only o / lse / the workspace (and the inspection rows) are written: pools and score rows keep their bits
        for p, b in zip((ctl.kv_cache.pool, ctl.metadata_cache.pool), before):
            assert torch.equal(p.buf.view(torch.int16), b.view(torch.int16))
        assert torch.equal(rows.view(torch.int16), rows_before.view(torch.int16))
        res.append((run.idx.cpu(), _bits(run.o), _bits(run.val), run.lse.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])


def test_refusals_leave_the_output_untouched():
    """On a real plan: 257 selected pages, and rows beyond the limit, are refused with nothing launched."""
    ctl, q, _ = _sequence(999 * PAGE + 16, 4, 2, 64, 257)
    h = ctl._decode_handler
    h.begin_forward(torch.tensor([0, 257], dtype=torch.int32), 4, 2, 64, PAGE, torch.float16)
    _, rows = _score_rows(1, 4, 2, 999, True, torch.float16)
    o = torch.full((1, 4, 64), 77.0, dtype=torch.float16, device=DEV)
    assert h.forward_group_topk(cuda(q), o, ctl.kv_layer(0), ctl.kv_indices_with_last, rows, None, 999,
                                paged_kv_last_page_len=16, paged_kv_last_page_idx=ctl.kv_last_page_idx) is False
    torch.cuda.synchronize()
    assert bool((o == 77.0).all())
    h.begin_forward(torch.tensor([0, 256], dtype=torch.int32), 4, 2, 64, PAGE, torch.float16)  # the plan _sequence left


# ---------------------------------------------------------------------------- state-driven: a batch, captured steps
def _prefill(ctl, k, v):
    import quest_amd.utils as qu

    L = k.shape[0]
    ctl.prepare_metadata(L)
    ctl.begin_forward(L)
    qu.append_kv(k, v, ctl, 0)
    ctl.end_forward()


def _logical(phys_rows, table):
    where = {int(p): j for j, p in enumerate(table)}
    return [[where[int(p)] for p in row] for row in phys_rows]


class _StateDriven:
    """``n`` sequences of a group-selection controller (one: InferenceController, more: BatchedInferenceController) after
    their prefill, planned for state-driven steps with a forced split, with the selection read back."""

    def __init__(self, lens, budgets, hq, hkv, d, cap, ppc, seed, data_seeds=None):
        import quest_amd.utils as qu

        dev = torch.device(DEV)
        self.n, self.hq, self.hkv, self.d, self.budgets = len(lens), hq, hkv, d, list(budgets)
        if self.n == 1:
            self.ctl = qu.InferenceController(1, hq, d, PAGE, budgets[0], cap, torch.float16, dev, num_kv_heads=hkv,
                                              shuffle_seed=seed, group_selection=True)
            self.seqs = [self.ctl]
        else:
            self.ctl = qu.BatchedInferenceController(self.n, 1, hq, d, PAGE, max(budgets), cap, torch.float16, dev,
                                                     num_kv_heads=hkv, shuffle_seed=seed, group_selection=True)
            self.seqs = self.ctl.seqs
        for i, (c, L) in enumerate(zip(self.seqs, lens)):
            _, k, v = inputs(data_seeds[i] if data_seeds else 300 + i + 7 * seed, L, hq, hkv, d)
            _prefill(c, cuda(k), cuda(v))
        self.ctl.enable_device_state()
        if self.n > 1 and len(set(budgets)) > 1:
            self.ctl.set_page_budgets(budgets)
        self.ctl._decode_handler.set_pages_per_chunk(ppc)
        self.ctl.begin_graph_decode()
        self.k_max = self.ctl.inference_page_budget - 1
        self.scores = qu.score_scratch(self.ctl).zero_()
        self.idx = torch.full((self.n, hkv, self.k_max), -1, dtype=torch.int32, device=DEV)
        self.val = torch.zeros((self.n, hkv, self.k_max), dtype=torch.float16, device=DEV)
        self.ctl._decode_handler.set_selection_out(self.val, self.idx)
        self.q = torch.empty(self.n, hq, d, dtype=torch.float16, device=DEV)
        self.kn = torch.empty(self.n, hkv, d, dtype=torch.float16, device=DEV)
        self.vn = torch.empty(self.n, hkv, d, dtype=torch.float16, device=DEV)
        self.o = torch.empty(self.n, hq, d, dtype=torch.float16, device=DEV)

    def layer(self, advance_after=False):
        import quest_amd.utils as qu

        qu._decode_layer(self.q, self.kn, self.vn, self.ctl, 0, self.scores, None, None, False, None, None, out=self.o,
                         advance_after=advance_after)
        assert self.ctl.last_layer_launches == 2

    def close(self):
        self.ctl._decode_handler.set_selection_out(None, None)

    def check_sequence(self, i, ppc):
        """Sequence i after a step (host mirror already advanced): its selection against the restatement on the step's own
        score rows, and against the EAGER entry at that length on a second handler with the same split (same bits)."""
        import quest_amd.utils as qu

        c = self.seqs[i]
        table = np.array(c.kv_cache.indicies, np.int32)
        n = len(table) - 1
        k = min(self.budgets[i] - 1, n)
        group = self.hq // self.hkv
        sc = self.scores.view(self.n, self.hq, -1)[i]
        bits = _bits(sc[:, :n]) if n else np.zeros((self.hq, 0), np.uint16)
        got = self.idx[i, :, :k].cpu().numpy()
        if k:
            _, want = group_topk(bits.view(np.float16), table, group, k)
            assert np.array_equal(got, want), f"sequence {i}: selection"
        if not k:
            return got
        h2 = qu.BatchDecodeWithPagedKVCacheWrapper("NHD")
        h2.set_pages_per_chunk(ppc)
        h2.begin_forward(torch.tensor([0, k], dtype=torch.int32), self.hq, self.hkv, self.d, PAGE, torch.float16)
        idx2 = torch.full((1, self.hkv, k), -1, dtype=torch.int32, device=DEV)
        h2.set_selection_out(None, idx2)
        o2 = torch.empty(1, self.hq, self.d, dtype=torch.float16, device=DEV)
        dev_table = torch.from_numpy(table).to(DEV)
        assert h2.forward_group_topk(self.q[i:i + 1], o2, self.ctl.kv_layer(0), dev_table, sc[:, :n], None, n,
                                     paged_kv_last_page_len=c.kv_cache.last_page_len,
                                     paged_kv_last_page_idx=int(table[-1]))
        h2.set_selection_out(None, None)
        assert np.array_equal(idx2[0].cpu().numpy(), got), f"sequence {i}: eager entry's selection"
        # the same slots per workgroup in both launches: a forced split, and the state-driven plan (k_max + 1 slots) cut like
        # the eager one (k + 1)
        same_split = ppc != 0 and k == self.k_max
        if same_split:
            assert torch.equal(o2[0], self.o[i]), f"sequence {i}: output bits of the eager entry"
        else:
            assert float((o2[0].float() - self.o[i].float()).abs().max()) <= ATOL
        return got


def test_batched_per_sequence_budgets_equal_each_sequence_alone():
    """3 sequences of 40, 700 and 2100 tokens with budgets 4, 16 and 33 pages (40 tokens = 3 pages: shorter than its budget,
    it attends everything).  Per sequence the selection is that of the sequence alone in its own pools, bit for bit (as
    logical pages: the pools hand out other physical ones), and the output within 2e-3."""
    lens, budgets, hq, hkv, d = (40, 700, 2100), (4, 16, 33), 8, 2, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    new = [torch.randn(3, h, d, generator=g, device=DEV, dtype=torch.float16) for h in (hq, hkv, hkv)]
    b = _StateDriven(lens, budgets, hq, hkv, d, 2100 + 64, 0, seed=1, data_seeds=(311, 312, 313))
    singles = [_StateDriven((L,), (B,), hq, hkv, d, 2100 + 64, 0, seed=2 + i, data_seeds=(311 + i,))  # its own pools, other pages
               for i, (L, B) in enumerate(zip(lens, budgets))]
    try:
        import quest_amd.utils as qu

        for s in [b] + singles:
            qu.step_advance_batched(s.ctl) if s.n > 1 else qu.step_advance_dyn(s.ctl)
        b.q.copy_(new[0]); b.kn.copy_(new[1]); b.vn.copy_(new[2])
        b.layer()
        assert b.ctl._decode_handler.last_launch_info()["front_end_variant"] == 9
        assert b.ctl._decode_handler.last_launch_info()["n_seqs"] == 3
        b.ctl.prepare_metadata(1)
        for i, s in enumerate(singles):
            s.q.copy_(new[0][i:i + 1]); s.kn.copy_(new[1][i:i + 1]); s.vn.copy_(new[2][i:i + 1])
            s.layer()
            s.ctl.prepare_metadata(1)
            got = b.check_sequence(i, 0)
            alone = s.check_sequence(0, 0)
            assert _logical(got, b.seqs[i].kv_cache.indicies) == _logical(alone, s.ctl.kv_cache.indicies), f"sequence {i}"
            n = len(s.ctl.kv_cache.indicies) - 1
            assert torch.equal(b.scores[i][:, :n], s.scores.view(hq, -1)[:, :n])
            err = float((b.o[i].float() - s.o[0].float()).abs().max())
            print(f"batched sequence {i} ({lens[i]} tokens, budget {budgets[i]}): |o - alone| <= {err:.3e}")
            assert err <= ATOL
    finally:
        for s in [b] + singles:
            s.close()


@pytest.mark.parametrize("lens", [(16 * 20 + 9,), (16 * 20 + 9, 16 * 9 + 15, 16 * 31 + 2)], ids=["one", "batch3"])
def test_captured_step_grows_across_a_page_boundary(lens):
    """A step captured once (append+estimate, group-selection launch with the armed advance in its merge launch) replayed
    for 20 tokens: every step's selection and output equal the eager entry's at that length, and the armed advance leaves
    the state quest_step_state_advance_batched leaves (the host mirror's, one reserved token ahead)."""
    import quest_amd.utils as qu

    hq, hkv, d, budget, steps, ppc = 8, 2, 128, 7, 20, 2
    s = _StateDriven(lens, (budget,) * len(lens), hq, hkv, d, max(lens) + steps + 40, ppc, seed=5)
    n = s.n
    g = torch.Generator(device=DEV).manual_seed(9)
    new = [torch.randn(steps, n, h, d, generator=g, device=DEV, dtype=torch.float16) for h in (hq, hkv, hkv)]
    try:
        qu.step_advance_batched(s.ctl) if n > 1 else qu.step_advance_dyn(s.ctl)  # the first token's reservation
        s.ctl.prepare_metadata(1)
        s.q.copy_(new[0][0]); s.kn.copy_(new[1][0]); s.vn.copy_(new[2][0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            s.layer(advance_after=True)  # warm-up; undone below
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        s.ctl.sync_device_state()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s.layer(advance_after=True)
        s.ctl.sync_device_state()  # (capture launches nothing; the state is the mirror's)
        assert s.ctl._decode_handler.last_launch_info()["workgroups_per_head"] == (budget + ppc - 1) // ppc
        for t in range(steps):
            s.q.copy_(new[0][t]); s.kn.copy_(new[1][t]); s.vn.copy_(new[2][t])
            s.idx.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            for i in range(n):  # the token is in the pools; the mirror still describes this length
                s.check_sequence(i, ppc)
            s.ctl.prepare_metadata(1)  # host mirror of the advance that rode in the merge launch
            st = s.ctl.step_states.cpu().tolist()
            for i, c in enumerate(s.seqs):
                kv, meta = c.kv_cache, c.metadata_cache
                assert st[i] == [kv.seqlen, len(kv.indicies), kv.last_page_len, kv.indicies[-1], len(meta.indicies),
                                 meta.last_page_len, meta.indicies[-1], 0], f"token {t} sequence {i}: state"
        assert all(len(c.kv_cache.indicies) > (L + 15) // 16 for c, L in zip(s.seqs, lens))  # a page was opened
    finally:
        s.close()


# ---------------------------------------------------------------------------- the model
def _model_bits():
    import test_gpu_model_sparse_reference as base

    return base


class _GroupSequence:
    """tests/test_gpu_model_sparse_reference.py's ``_Sequence`` with the selection check restated for one selection per kv
    head: the reference is forced to the device's group selection expanded to ``[Hq, B - 1]`` rows; the device's selection
    must be the key-max top-k of the float64 page scores wherever those separate the k-th and (k+1)-th page of the GROUP
    score by more than that file's guard band (3 delta, delta = max |yardstick - float64| over the layer's scores).  Logits
    and caches: that file's bars, through its own ``_check`` / ``finish``."""

    def __init__(self, *a):
        base = _model_bits()
        self.base, self.seq = base, base._Sequence(*a)
        self.rows = self.decided = 0

    def step(self, token, got, observed, table, t):
        base, s = self.base, self.seq
        B = base.BUDGET
        hkv = s.r64.hkv
        group = s.hq // hkv
        n_pages = -(-(s.r64.seqlen + 1) // base.PAGE)
        assert n_pages > B and sorted(observed) == list(range(2, s.layers))
        logical = {int(p): j for j, p in enumerate(table)}
        forced, picked = {}, {}
        for layer, phys in observed.items():
            assert tuple(phys.shape) == (hkv, B - 1)
            rows = [[logical.get(int(p), -1) for p in row] for row in phys.tolist()]
            for row in rows:
                assert len(set(row)) == B - 1 and min(row) >= 0 and max(row) <= n_pages - 2, rows
            picked[layer] = rows
            forced[layer] = torch.tensor(rows).repeat_interleave(group, dim=0)
        l64, i64 = s.r64.step(token, forced)
        ly, iy = s.yard.step(token, forced)
        assert sorted(i64) == sorted(iy) == sorted(forced)
        for layer in sorted(i64):
            s64, sy = i64[layer].scores, iy[layer].scores.double()
            delta = float((sy - s64).abs().max())
            g64 = s64.view(hkv, group, -1).amax(1)
            top = g64.sort(dim=1, descending=True)
            decided = (top.values[:, B - 2] - top.values[:, B - 1]) > 3 * delta
            for hk in range(hkv):
                self.rows += 1
                if bool(decided[hk]):
                    self.decided += 1
                    assert set(picked[layer][hk]) == set(top.indices[hk, :B - 1].tolist()), \
                        f"token {t} layer {layer} kv head {hk}: {picked[layer][hk]} vs float64's {top.indices[hk, :B - 1].tolist()}"
        s._check(got, ly, l64, f"token {t}")
        return int(l64.argmax())


STEPS = 12


def test_model_eager_module_path(monkeypatch):
    """4 layers (two dense, two sparse), 200-token prompt + 12 tokens (token 209 opens the 14th page): the eager module path
    with ``group_selection=True`` states the selection with the existing operators; ``decode_group_topk`` runs once per
    sparse layer and token, the per-head ``decode_topk`` never."""
    import quest_amd.utils as qutils

    base = _model_bits()
    dev = torch.device(DEV)
    m, cfg = base._model("llama", 4, torch.float16, fused=False)
    m.quest_init(base.PAGE, 512, token_budget=base.PAGE * base.BUDGET, group_selection=True)
    ctl = m.model.iController
    prompt = base._prompt(200)
    seq = _GroupSequence(m, cfg, "llama", torch.float16, prompt, "group eager")
    current, calls, real = {}, [], qutils.decode_group_topk
    for i, layer in enumerate(m.model.layers):
        layer.self_attn.register_forward_pre_hook(lambda mod, args, i=i: current.__setitem__("layer", i))

    def spy(scores, controller):
        out = real(scores, controller)
        hk = controller.num_kv_heads
        assert torch.equal(out, controller.topk_dindices_buffer[:hk].repeat_interleave(controller.num_heads // hk, dim=0))
        calls.append((current["layer"], controller.topk_dindices_buffer[:hk].cpu()))
        return out

    def never(*a, **k):
        raise AssertionError("per-head decode_topk called with group_selection=True")

    monkeypatch.setattr(qutils, "decode_group_topk", spy)
    monkeypatch.setattr(qutils, "decode_topk", never)
    with torch.inference_mode():
        tok = seq.seq.prefill(m(input_ids=prompt[None].to(dev))[0, -1])
        for t in range(STEPS):
            calls.clear()
            got = m(input_ids=torch.tensor([[tok]], device=dev))[0, -1]
            assert [c[0] for c in calls] == [2, 3]
            tok = seq.step(tok, got, {c[0]: c[1] for c in calls}, ctl.kv_cache.indicies, t)
    seq.seq.finish(ctl, ctl.kv_layer, 200 + STEPS)
    print(f"group eager: decided rows {seq.decided}/{seq.rows}")
    base._floor(seq.decided / seq.rows, torch.float16)


@pytest.mark.parametrize("fused_layers", [False, None], ids=["module_path", "fused_layers"])
def test_model_captured_steps(fused_layers):
    """3 layers (the last one sparse and observed through the handler's selection output, rows ``[1, Hkv, B - 1]``)."""
    base = _model_bits()
    dev = torch.device(DEV)
    m, cfg = base._model("llama", 3, torch.float16)
    m.quest_init(base.PAGE, 512, token_budget=base.PAGE * base.BUDGET, group_selection=True)
    ctl = m.model.iController
    prompt = base._prompt(200)
    seq = _GroupSequence(m, cfg, "llama", torch.float16, prompt, f"group captured fused_layers={fused_layers}")
    with torch.inference_mode():
        tok = seq.seq.prefill(m(input_ids=prompt[None].to(dev))[0, -1])
        out = base._SelectionOut(ctl._decode_handler, 1, cfg.num_key_value_heads, torch.float16)
        try:
            m.capture_decode_graph(fused_layers=fused_layers)
            assert m.fused_layers is (fused_layers is None)
            for t in range(STEPS):
                out.reset()
                got = m.decode_graph_step(input_ids=torch.tensor([[tok]], device=dev))[0, -1]
                tok = seq.step(tok, got, {2: out.read(0)[0]}, ctl.kv_cache.indicies, t)
            assert ctl._decode_handler.last_launch_info()["front_end_variant"] == 9
        finally:
            out.close()
    out.check_guard()
    seq.seq.finish(ctl, ctl.kv_layer, 200 + STEPS)
    print(f"group captured: decided rows {seq.decided}/{seq.rows}")
    base._floor(seq.decided / seq.rows, torch.float16)


def test_model_batched_of_two():
    base = _model_bits()
    dev = torch.device(DEV)
    lens = (200, 120)
    m, cfg = base._model("llama", 3, torch.float16)
    m.quest_init_batched(len(lens), base.PAGE, 512, token_budget=base.PAGE * base.BUDGET, group_selection=True)
    b = m.model.bController
    seqs = [_GroupSequence(m, cfg, "llama", torch.float16, base._prompt(L, i), f"group batched {i}") for i, L in enumerate(lens)]
    with torch.inference_mode():
        toks = [s.seq.prefill(m.prefill_sequence(i, base._prompt(L, i)[None].to(dev))[0, -1])
                for i, (s, L) in enumerate(zip(seqs, lens))]
        out = base._SelectionOut(b._decode_handler, len(lens), cfg.num_key_value_heads, torch.float16)
        try:
            m.capture_decode_graph_batched()
            for t in range(STEPS):
                out.reset()
                got = m.decode_graph_step_batched(torch.tensor(toks, device=dev))
                for i, (s, c) in enumerate(zip(seqs, b.seqs)):
                    toks[i] = s.step(toks[i], got[i, -1], {2: out.read(i)[0]}, c.kv_cache.indicies, t)
            assert b._decode_handler.last_launch_info()["front_end_variant"] == 9
        finally:
            out.close()
    out.check_guard()
    for s, c, L in zip(seqs, b.seqs, lens):
        s.seq.finish(c, b.kv_layer, L + STEPS)
    rows, decided = sum(s.rows for s in seqs), sum(s.decided for s in seqs)
    print(f"group batched: decided rows {decided}/{rows}")
    base._floor(decided / rows, torch.float16)


def test_model_default_flag_reproduces_the_per_head_tokens():
    """The default stays per-head selection: a model initialised without the argument and one with ``group_selection=False``
    produce the same logits bits over prompt + 12 captured tokens and never take the group-selection launch."""
    base = _model_bits()
    dev = torch.device(DEV)
    runs = []
    for kw in ({}, {"group_selection": False}):
        m, cfg = base._model("llama", 3, torch.float16)
        m.quest_init(base.PAGE, 512, token_budget=base.PAGE * base.BUDGET, **kw)
        assert m.model.iController.group_selection is False
        logits = []
        with torch.inference_mode():
            tok = int(m(input_ids=base._prompt(200)[None].to(dev))[0, -1].argmax())
            m.capture_decode_graph()
            for t in range(STEPS):
                got = m.decode_graph_step(input_ids=torch.tensor([[tok]], device=dev))[0, -1]
                logits.append(got.clone())
                tok = int(got.argmax())
        assert m.model.iController._decode_handler.last_launch_info()["front_end_variant"] != 9
        runs.append(torch.stack(logits))
    assert torch.equal(runs[0], runs[1])
