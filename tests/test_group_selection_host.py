"""Group-shared page selection for GQA (quest_decode_forward_group_topk, include/quest_hip.h), the parts that need no GPU:
the numpy restatement the GPU tests compare against (tests/_group_selection.py) does what the declared semantics say; the
C entry refuses before any launch; the controllers take the flag and refuse shapes outside the envelope at construction; the
built kernel has no scratch and no spills."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from _group_selection import expand, group_scores, group_topk, key_to_half

EINVAL, EUNSUPPORTED, ESTATE, ETOOLARGE = -1, -2, -3, -4


def _scores(seed, hq, n):
    from oracle import synth

    return synth.normal_f16(seed, (hq, n))


# ---------------------------------------------------------------------------------------------- the restatement
def test_key_round_trip_is_the_identity_on_every_pattern():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(key_to_half(oracle.half_key(bits.view(np.float16))).view(np.uint16), bits)


@pytest.mark.parametrize("n,k", [(1, 1), (9, 3), (130, 32), (1000, 255)])
def test_group_of_one_is_the_per_head_selection(n, k):
    s, table = _scores(n, 6, n), np.arange(100, 100 + n, dtype=np.int32)
    gv, gi = group_topk(s, table, 1, k)
    ov, oi = oracle.topk(s, np.tile(table, (6, 1)), k)
    assert np.array_equal(gi, oi) and np.array_equal(gv.view(np.uint16), ov.view(np.uint16))


@pytest.mark.parametrize("group", [2, 4, 8])
def test_heads_with_the_same_scores_select_what_each_selects_alone(group):
    """A group whose heads carry the same q scores every page alike: the group selects what each head alone selects."""
    hk, n, k = 3, 200, 17
    one = _scores(5, hk, n)
    s = np.repeat(one, group, axis=0)  # [hk * group, n], the heads of a group identical
    _, gi = group_topk(s, np.arange(n), group, k)
    _, oi = oracle.topk(s, np.tile(np.arange(n, dtype=np.int32), (hk * group, 1)), k)
    assert np.array_equal(expand(gi, group), oi)


def test_a_page_that_only_one_head_ranks_first_is_selected():
    group, n, k = 4, 64, 3
    s = np.full((group, n), -1.0, np.float16)
    s[:, :8] = np.float16(0.5)       # what most heads like: columns 0..7 tie at 0.5
    s[2, 41] = np.float16(3.0)       # one head's top page
    _, gi = group_topk(s, np.arange(n), group, k)
    assert 41 in gi[0].tolist()
    assert gi[0].tolist() == [0, 1, 41]  # the tie at 0.5 resolves to the lowest columns, output in column order


def test_ties_across_heads_resolve_to_the_lowest_column():
    group, n = 2, 12
    s = np.zeros((group, n), np.float16)
    s[0, [3, 7, 9]] = np.float16(2.0)   # head 0 and head 1 put the same value on different pages
    s[1, [1, 7, 11]] = np.float16(2.0)
    _, gi = group_topk(s, np.arange(n), group, 3)
    assert gi[0].tolist() == [1, 3, 7]  # five pages tie at 2.0 under the group score: columns 1, 3, 7, 9, 11
    _, gi = group_topk(s, np.arange(n), group, 6)
    assert gi[0].tolist() == [0, 1, 3, 7, 9, 11]  # then the zeros, lowest column first


def test_signed_zeros_and_nan_follow_the_key_order():
    """The maximum is taken on the keys: +0 beats -0, a NaN pattern with the sign clear beats +inf, one with the sign set
    loses to -inf -- whatever the other heads of the group hold."""
    pz, nz = np.float16(0.0), np.float16(-0.0)
    nan_pos = np.array([0x7E00], np.uint16).view(np.float16)[0]
    nan_neg = np.array([0xFE00], np.uint16).view(np.float16)[0]
    s = np.array([[nz, pz, nan_neg, np.float16(-np.inf), np.float16(np.inf), np.float16(1.0)],
                  [nz, nz, nan_neg, nan_neg, nan_pos, nan_neg]], np.float16)
    g = group_scores(s, 2).view(np.uint16)[0].tolist()
    assert g == [0x8000, 0x0000, 0xFE00, 0xFC00, 0x7E00, 0x3C00]
    _, gi = group_topk(s, np.arange(6), 2, 6)
    assert gi[0].tolist() == [0, 1, 2, 3, 4, 5]
    _, gi = group_topk(s, np.arange(6), 2, 3)
    assert gi[0].tolist() == [1, 4, 5]  # NaN(+), 1.0, +0
    _, gi = group_topk(s, np.arange(6), 2, 4)
    assert gi[0].tolist() == [0, 1, 4, 5]  # then -0, ahead of -inf and NaN(-)


def test_torch_restatement_of_the_eager_module_path_is_the_numpy_one():
    """``quest_amd.utils.group_max_scores`` (the eager module path's key-max) on every kind of pattern."""
    from quest_amd.utils import group_max_scores

    s = _scores(11, 8, 300)
    bits = s.view(np.uint16).copy()
    bits[0, :5] = [0x7E00, 0xFE00, 0x8000, 0x0000, 0x7C00]
    bits[3, :5] = [0xFC00, 0x7FFF, 0xFFFF, 0x8000, 0x8000]
    s = bits.view(np.float16)
    for group in (1, 2, 4, 8):
        got = group_max_scores(torch.from_numpy(s.copy()), group).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, group_scores(s, group).view(np.uint16)), group


# ---------------------------------------------------------------------------------------------- the entry's refusals
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced


def _kv(**kw):
    from quest_amd._lib import PagedKV

    f = dict(data=16, indices=16, indptr=16, num_heads=8, page_size=16, head_dim=128, page_budget=8, last_page_len=1,
             last_page_idx=0, layout=0)
    f.update(kw)
    return PagedKV(**f)


def _batch(n_seqs=1, kv_stride=0):
    from quest_amd._lib import Batch

    return Batch(n_seqs, kv_stride, 0, 0, None)


class _Handler:
    """A handler planned without a device: one workgroup per head, so that begin_forward allocates nothing (a plan for 64
    sequences, or a forced split that keeps every page in one workgroup)."""

    def __init__(self, n_sel=8, hq=32, hkv=8, d=128, ps=16, batch=64, ppc=0):
        from quest_amd._lib import lib

        self.lib, self.h = lib, ctypes.c_void_p()
        assert lib.quest_decode_handler_create(ctypes.byref(self.h), 0) == 0
        if n_sel is not None:
            assert lib.quest_decode_set_batch(self.h, batch) == 0
            assert lib.quest_decode_set_pages_per_chunk(self.h, ppc) == 0
            assert lib.quest_decode_begin_forward(self.h, n_sel, hq, hkv, d, ps, None) == 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.quest_decode_handler_destroy(self.h)

    def call(self, q=ONE, o=ONE, kv=None, hq=32, scores=ONE, stride=104, n=100, state=ONE, batch=None):
        return self.lib.quest_decode_forward_group_topk(self.h, q, o, kv if kv is not None else _kv(), hq, scores, stride, n,
                                                        state, batch if batch is not None else _batch(), None, None)


def test_entry_refuses_before_any_launch():
    with _Handler() as h:
        for null in ("q", "o", "scores"):
            assert h.call(**{null: None}) == EINVAL, null
        assert h.call(stride=99) == EINVAL                       # rows shorter than their columns
        assert h.call(state=None, batch=_batch(2, 104)) == EINVAL  # the eager form is one sequence
        assert h.call(batch=_batch(2, 100)) == EINVAL            # page tables shorter than the rows
        assert h.call(batch=_batch(0)) == EINVAL
        assert h.call(batch=_batch(65, 104)) == ESTATE           # the plan is for 64 sequences
        assert h.call(kv=_kv(num_heads=16)) == EINVAL            # not the plan's geometry
        assert h.call(n=4) == EINVAL                             # fewer columns than selected pages
        assert h.call(n=16385, stride=16392) == ETOOLARGE
        assert h.call(n=4097, stride=4104) == EUNSUPPORTED       # beyond the row limit of this launch
        assert h.call(state=None, kv=_kv(last_page_len=0)) == EINVAL
    with _Handler(n_sel=None) as h:
        assert h.call() == ESTATE                                # no plan
        assert h.call(q=None) == ESTATE                          # (the order of the sibling entries: plan before operands)
        assert h.call(scores=None) == EINVAL
    from quest_amd._lib import lib

    assert lib.quest_decode_forward_group_topk(None, ONE, ONE, _kv(), 32, ONE, 104, 100, ONE, _batch(), None, None) == EINVAL


@pytest.mark.parametrize("plan,kv,hq,n", [
    (dict(ps=8), dict(page_size=8), 32, 100),                        # page size 8
    (dict(d=256), dict(head_dim=256), 32, 100),                      # head_dim 256
    (dict(hq=6, hkv=2, ppc=9), dict(num_heads=2), 6, 100),           # 3 query heads per kv head (9 slots: one workgroup)
    (dict(n_sel=257, ppc=1000), dict(), 32, 300),                    # 257 selected pages
    (dict(hq=32, hkv=2, ppc=9), dict(num_heads=2), 32, 100),         # 16 query heads per kv head
])
def test_entry_returns_unsupported_outside_the_envelope(plan, kv, hq, n):
    with _Handler(**plan) as h:
        assert h.call(kv=_kv(**kv), hq=hq, n=n, stride=(n + 7) // 8 * 8) == EUNSUPPORTED
        assert h.call(kv=_kv(**kv), hq=hq, n=n, stride=(n + 7) // 8 * 8, state=None) == EUNSUPPORTED


def test_plan_info_answers_do_not_move_with_the_group_plan():
    """begin_forward plans the (kv head, chunk) split NEXT to the per-head one: quest_decode_plan_info answers as before."""
    with _Handler(n_sel=255, hq=32, hkv=8) as h:
        ppc, chunks = ctypes.c_uint32(), ctypes.c_uint32()
        assert h.lib.quest_decode_plan_info(h.h, ctypes.byref(ppc), ctypes.byref(chunks)) == 0
        assert (ppc.value, chunks.value) == (256, 1)


# ---------------------------------------------------------------------------------------------- controllers, model
def test_controller_flag_defaults_off_and_refuses_shapes_outside_the_envelope():
    from quest_amd.utils import BatchedInferenceController, InferenceController

    c = InferenceController(1, 8, 128, 16, 4, 1000, torch.float16, "cpu", num_kv_heads=2)
    assert c.group_selection is False
    c = InferenceController(1, 8, 128, 16, 4, 1000, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    assert c.group_selection is True
    b = BatchedInferenceController(2, 1, 8, 128, 16, 4, 400, torch.float16, "cpu", num_kv_heads=2)
    assert b.group_selection is False and not any(s.group_selection for s in b.seqs)
    b = BatchedInferenceController(2, 1, 8, 128, 16, 4, 400, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    assert b.group_selection is True and all(s.group_selection for s in b.seqs)
    with pytest.raises(ValueError, match="head_dim 256"):
        InferenceController(1, 8, 256, 16, 4, 1000, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    with pytest.raises(ValueError, match="4096 pages"):  # a pool beyond the row limit: 4098 pages -> rows of 4097
        InferenceController(1, 8, 128, 16, 4, 4098 * 16, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    InferenceController(1, 8, 128, 16, 4, 4097 * 16, torch.float16, "cpu", num_kv_heads=2, group_selection=True)  # the limit
    with pytest.raises(ValueError, match="page size 16"):
        InferenceController(1, 8, 128, 32, 4, 1000, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    with pytest.raises(ValueError, match="groups of 1, 2, 4 and 8"):
        InferenceController(1, 6, 128, 16, 4, 1000, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    with pytest.raises(ValueError, match="256 pages"):
        InferenceController(1, 8, 128, 16, 258, 8000, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    with pytest.raises(ValueError, match="head_dim 256"):
        BatchedInferenceController(2, 1, 8, 256, 16, 4, 400, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    with pytest.raises(ValueError, match="at most 64"):
        BatchedInferenceController(65, 1, 8, 128, 16, 4, 64, torch.float16, "cpu", num_kv_heads=2, group_selection=True)
    # the same shapes are served without the flag, as before
    InferenceController(1, 8, 256, 16, 4, 1000, torch.float16, "cpu", num_kv_heads=2)


def test_quest_init_passes_the_flag_through():
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=512)
    dev = torch.device("cpu")
    m = LlamaForCausalLM(cfg)
    m.quest_init(16, 256, token_budget=64, device=dev)
    assert m.model.iController.group_selection is False
    m = LlamaForCausalLM(cfg)
    m.quest_init(16, 256, token_budget=64, device=dev, group_selection=True)
    assert m.model.iController.group_selection is True
    m = LlamaForCausalLM(cfg)
    m.quest_init_batched(2, 16, 256, token_budget=64, device=dev, group_selection=True)
    assert m.model.bController.group_selection is True
    m = LlamaForCausalLM(cfg)
    with pytest.raises(ValueError, match="page size 16"):
        m.quest_init(32, 256, token_budget=64, device=dev, group_selection=True)


# ---------------------------------------------------------------------------------------------- the kernel as built
def test_group_selection_kernels_have_no_scratch_and_no_spills():
    from quest_amd.build import LIB, kernel_metadata

    llvm = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(llvm, "llvm-readelf")):
        pytest.skip("needs the built library and the ROCm LLVM tools (llvm-objcopy / llvm-readelf)")
    meta = kernel_metadata(LIB)
    hits = {k: v for k, v in meta.items() if "group_topk_attend_kernel" in k}
    # head_dim 64 / 128 x group 1 / 2 / 4 / 8 x fp16 / bf16
    assert len(hits) == 16, sorted(hits)
    assert sum("_bfloat16" in k for k in hits) == 8  # (the bf16 twins; not "_bf16": tests/test_bf16_host.py counts that suffix)
    for k, v in hits.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert v["vgpr"] <= 256, (k, v)          # built for two waves per SIMD: one 8-wave workgroup per CU at least
        assert v["lds"] <= 64 * 1024, (k, v)
    # and the fragments tests/test_build_metadata.py matches kernels by do not match this one
    for frag in ("sparse_decode_kernel", "shared_decode_kernel", "layer_decode_kernel"):
        assert not any(frag in k for k in hits)
