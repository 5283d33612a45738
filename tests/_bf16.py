"""Helpers of the bf16 tests: the fp16 oracle as referee of bf16 kernels.

An fp16 value whose low three mantissa bits are clear (``bits & 0xFFF8``) is exactly representable in bf16: fp16's
exponent range lies inside bf16's and 7 mantissa bits remain (subnormals included: they become bf16 normals).  So the
same real numbers can be handed to the device as bf16 and to ``oracle/`` as fp16.  numpy has no bf16: bf16 tensors
travel as uint16 bit patterns."""
import numpy as np
import torch

import oracle
from oracle import synth

BF16_MAX, BF16_NEG_MAX = 0x7F7F, 0xFF7F  # largest finite bf16, and its negative


def record(line: str) -> None:
    """A measured figure of the bf16 tests: printed (pytest -s) and, when QUEST_BF16_PARITY_FILE names a file, appended to it
    with the test case that measured it -- profiles/bf16_parity.txt is such a file, as the tests wrote it."""
    import os

    print(line)
    path = os.environ.get("QUEST_BF16_PARITY_FILE")
    if path:
        new = not os.path.exists(path)
        with open(path, "a") as f:
            if new:
                f.write("# written by tests/test_gpu_bf16_kernels.py and tests/test_gpu_bf16_model.py (tests/_bf16.py record()) with\n"
                        "# QUEST_BF16_PARITY_FILE=<this file> pytest tests/test_gpu_bf16_kernels.py tests/test_gpu_bf16_model.py -m gpu\n"
                        "# one line per measurement: <test case> | <figures>; the bars are in the tests' docstrings\n")
            case = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].replace("tests/", "")
            f.write(f"{case} | {line}\n")


def mask3(a: np.ndarray) -> np.ndarray:
    """fp16 array with the low three mantissa bits cleared: every value is a bf16 value."""
    return (np.ascontiguousarray(a, np.float16).view(np.uint16) & np.uint16(0xFFF8)).view(np.float16)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """Round to nearest even (NaN stays NaN)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.ascontiguousarray(x, np.float32))
    return np.where(nan, np.uint16(0x7FC0), r).astype(np.uint16)


def f16_to_bf16_bits(a: np.ndarray) -> np.ndarray:
    """fp16 -> bf16 bit patterns (exact for ``mask3`` data, round to nearest even otherwise)."""
    return f32_to_bf16_bits(np.ascontiguousarray(a, np.float16).astype(np.float32))


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_dev(bits: np.ndarray) -> torch.Tensor:
    """uint16 bf16 bit patterns -> a bf16 tensor on cuda:0."""
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to("cuda:0").view(torch.bfloat16)


def dev16(a_f16: np.ndarray) -> torch.Tensor:
    """``mask3`` fp16 data as the bf16 tensor of the same real numbers."""
    return to_dev(f16_to_bf16_bits(a_f16))


def bits(t: torch.Tensor) -> np.ndarray:
    """A bf16 (or fp16) tensor's bit patterns as uint16."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def inputs(seed, L, Hq, Hkv=None, D=128):
    """q ``[1, Hq, D]``, k / v ``[L, Hkv, D]``: N(0,1) fp16 data restricted to bf16 values."""
    Hkv = Hq if Hkv is None else Hkv
    return (mask3(synth.normal_f16(seed * 3, (1, Hq, D))), mask3(synth.normal_f16(seed * 3 + 1, (L, Hkv, D))),
            mask3(synth.normal_f16(seed * 3 + 2, (L, Hkv, D))))


def make_controller(L, Hq, Hkv, D, page_size, page_budget, layout=0, shuffle_seed=None, max_seq_len=None):
    import quest_amd.utils as qu

    return qu.InferenceController(1, Hq, D, page_size, page_budget, max_seq_len or (L + 4 * page_size), torch.bfloat16,
                                  torch.device("cuda:0"), num_kv_heads=Hkv, layout=layout, shuffle_seed=shuffle_seed)


def fill(ctl, k, v, chunks):
    """Append k / v ``[L, H, D]`` (fp16 data of bf16 values) in pieces of ``chunks`` tokens: pieces longer than one token take
    the prefill append, single tokens the decode append.  Left inside ``begin_forward`` of the last piece."""
    import quest_amd.utils as qu

    kc, vc = dev16(k), dev16(v)
    t = 0
    for i, n in enumerate(chunks):
        ctl.prepare_metadata(n)
        ctl.begin_forward(n)
        qu.append_kv(kc[t:t + n], vc[t:t + n], ctl, 0)
        t += n
        if i != len(chunks) - 1:
            ctl.end_forward()
    assert t == k.shape[0]


def oracle_pools(ctl, k, v):
    """The fp16 oracle's pools with the controller's physical page ids (tests/_harness.py)."""
    kvc, mc = ctl.kv_cache, ctl.metadata_cache
    kv = oracle.Paged(np.zeros(tuple(kvc.buf_layer(0).shape), np.float16), np.array(kvc.indicies, np.int32),
                      kvc.last_page_len, ctl.layout)
    meta = oracle.Paged(np.zeros(tuple(mc.buf_layer(0).shape), np.float16), np.array(mc.indicies, np.int32),
                        mc.last_page_len, ctl.layout)
    oracle.append_prefill(kv, meta, k, v)
    return kv, meta


def pools_equal_oracle(ctl, kv_o, meta_o, L):
    """Every valid KV token and metadata entry of the bf16 device pools == the oracle's fp16 pools converted to bf16."""
    from _harness import gather_entries

    n_pages = len(ctl.kv_cache.indicies)
    dk, dv = gather_entries(bits(ctl.kv_cache.buf_layer(0)), ctl.kv_cache.indicies, L, ctl.layout)
    ok_, ov_ = gather_entries(f16_to_bf16_bits(kv_o.data), kv_o.indices, L, ctl.layout)
    dmx, dmn = gather_entries(bits(ctl.metadata_cache.buf_layer(0)), ctl.metadata_cache.indicies, n_pages, ctl.layout)
    omx, omn = gather_entries(f16_to_bf16_bits(meta_o.data), meta_o.indices, n_pages, ctl.layout)
    return {"k": np.array_equal(dk, ok_), "v": np.array_equal(dv, ov_), "max": np.array_equal(dmx, omx),
            "min": np.array_equal(dmn, omn)}


def check_scores(dev_bits: np.ndarray, ora_f16: np.ndarray, max_undecided: float = 0.20):
    """The oracle returns fp16_rne(s), the device bf16_rne(s) of the same fp32 s.  Where the oracle's fp16 bits have
    ``bits & 7 != 4`` the bf16 rounding of s is decided by the oracle value: the device bits must equal the oracle value
    converted to bf16, exactly.  Elsewhere the oracle value sits on a bf16 midpoint: the device value must be one of its two
    bf16 neighbours.  The undecidable share is asserted to stay within ``max_undecided``.  Returns the share."""
    ob = np.ascontiguousarray(ora_f16, np.float16).view(np.uint16)
    assert dev_bits.shape == ob.shape
    f = ora_f16.astype(np.float32)
    mid = (ob & 7) == 4
    want = f32_to_bf16_bits(f)
    assert np.array_equal(dev_bits[~mid], want[~mid]), \
        f"{int((dev_bits[~mid] != want[~mid]).sum())} of {int((~mid).sum())} decided scores differ"
    u = f.view(np.uint32)
    lo = (u >> 16).astype(np.uint16)  # truncation: the neighbour towards zero; the other one is one bf16 ulp further out
    hi = (lo + 1).astype(np.uint16)
    ok = (dev_bits == lo) | (dev_bits == hi)
    assert ok[mid].all(), f"{int((~ok[mid]).sum())} midpoint scores are not a bf16 neighbour of the oracle value"
    share = float(mid.mean())
    record(f"estimate: undecidable share {share:.4f} of {mid.size} scores (bar 0.20), 0 decided scores differ, 0 others off a neighbour")
    assert share <= max_undecided, share
    return share
