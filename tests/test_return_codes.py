"""Return codes of the C entries whose host side is shared (attention launches, decode appends, estimate launches): one
table of calls with never-dereferenced operands, each with the code the library returned when the table was recorded
(``python tests/test_return_codes.py`` prints the codes of the library in use, in table order).  What the table pins is
the ORDER of the checks: an entry that is malformed in two ways at once keeps the code of the check that comes first.

No GPU is needed: every call is refused before a launch, except the well-formed ones (expected "> 0"), which get as far
as the launch and come back with a HIP error where there is no device.  On a machine WITH a device those calls would
launch kernels on the fake operands, so they are made only where no device is visible.

A handler can be planned without a device where ``begin_forward`` allocates nothing: one workgroup per head, i.e. a plan
for 64 sequences of 32 heads with at most 255 selected pages.

An operator has ONE entry; the table calls it in each of its FORMS (``"<entry>, <form>"``: one sequence = the batch
``{1, 0, 0, 0, NULL}``, contiguous rows = stride 0, whole rows = ``tile_max_offset`` 0), with the arguments that make the form
held fixed (``"=name"``: never varied).  Two forms that come to the same call are made once.

The one-sequence tiles form of ``quest_append_estimate_batched`` makes the checks of the batched tiles form (``tile_max_offset``
is exactly the row capacity rounded up to 8, rows 16-byte aligned), which a single sequence was once spared: its cases
``n = 4`` (offset 104 is not 8), ``off = 112`` with stride 136, and ``o`` at addresses 24 and 18 are EINVAL, where the table
first recorded a launch.  Rows like these could never be read back: the attention launch has always refused them."""
import ctypes

EINVAL, EUNSUPPORTED, ESTATE, ETOOLARGE = -1, -2, -3, -4
CODES = {0: "0", EINVAL: "I", EUNSUPPORTED: "U", ESTATE: "S", ETOOLARGE: "T"}  # the letters of EXPECTED
LAUNCHED = "L"  # "> 0": a HIP error from the launch itself

ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned
MAX_N = 100                # columns of a score row
OFF, TSTRIDE = 104, 120    # tile_max_offset(100), tiles_row_stride(100)


def _kv(**kw):
    from quest_amd._lib import PagedKV

    f = dict(data=16, indices=16, indptr=16, num_heads=32, page_size=16, head_dim=128, page_budget=8, last_page_len=1,
             last_page_idx=0, layout=0)
    f.update(kw)
    return PagedKV(**f)


def _b(n_seqs=2, kv_stride=104, meta_stride=8):
    from quest_amd._lib import Batch

    return Batch(n_seqs, kv_stride, meta_stride, 0, None)


# "<entry>[, <form>]" -> ordered (argument, well-formed value); "h" = the handler, filled in per case; "=name" = an argument
# the form fixes (no case replaces it)
def _entries():
    kv, b = _kv(), _b()
    one, whole, contiguous = ("=batch", _b(1, 0, 0)), ("=off", 0), ("=stride", 0)
    att = [("h", None), ("q", ONE), ("o", ONE), ("kv", kv), ("hq", 32)]
    app = [("h", None), ("k", ONE), ("v", ONE), ("metadata", kv), ("q", ONE), ("o", ONE), ("kv", kv), ("hq", 32)]
    est = [("k", ONE), ("v", ONE), ("kv", kv), ("q", ONE), ("o", ONE), ("hq", 32)]
    tail = [("lse", None), ("stream", None)]
    return {
        "quest_decode_forward": att + tail,
        "quest_decode_forward_shared": att + tail,
        "quest_decode_forward_shared_batched, one sequence": att + [("state", ONE), one] + tail,
        "quest_decode_forward_shared_batched": att + [("state", ONE), ("batch", b)] + tail,
        "quest_decode_append_forward_shared_batched, one sequence": app + [("state", ONE), one] + tail,
        "quest_decode_append_forward_shared_batched": app + [("state", ONE), ("batch", b)] + tail,
        "quest_decode_forward_fused_topk, contiguous rows": att + [("scores", ONE), ("n", MAX_N), contiguous, ("val_out", None),
                                                                   ("idx_out", None)] + tail,
        "quest_decode_forward_fused_topk": att + [("scores", ONE), ("n", MAX_N), ("stride", 104), ("val_out", None),
                                                  ("idx_out", None)] + tail,
        "quest_decode_forward_fused_topk_batched, one sequence": att + [("scores", ONE), ("stride", 104), ("n", MAX_N), whole,
                                                                        ("state", ONE), one] + tail,
        "quest_decode_forward_fused_topk_batched, one sequence, tiles": att + [("scores", ONE), ("stride", TSTRIDE), ("n", MAX_N),
                                                                               ("off", OFF), ("state", ONE), one] + tail,
        "quest_decode_forward_fused_topk_batched": att + [("scores", ONE), ("stride", 104), ("n", MAX_N), whole, ("state", ONE),
                                                          ("batch", b)] + tail,
        "quest_decode_forward_fused_topk_batched, tiles": att + [("scores", ONE), ("stride", TSTRIDE), ("n", MAX_N),
                                                                 ("off", OFF), ("state", ONE), ("batch", b)] + tail,
        "quest_decode_forward_batched": att + [("indices", ONE), ("idx_stride", 8), ("state", ONE), ("batch", b)] + tail,
        "quest_decode_layer_fused_batched": app + [("n", MAX_N), ("state", ONE), ("batch", b), ("scores_out", None),
                                                   ("stride", 0)] + tail,
        "quest_append_kv_cache_decode": [("k", ONE), ("v", ONE), ("kv", kv), ("metadata", kv), ("stream", None)],
        "quest_append_kv_cache_decode_batched, one sequence": [("k", ONE), ("v", ONE), ("kv", kv), ("metadata", kv),
                                                               ("state", ONE), one, ("stream", None)],
        "quest_append_kv_cache_decode_batched": [("k", ONE), ("v", ONE), ("kv", kv), ("metadata", kv), ("state", ONE),
                                                 ("batch", b), ("stream", None)],
        "quest_append_kv_cache_prefill": [("k", ONE), ("v", ONE), ("append_len", 20), ("n_pages", 4), ("kv", kv),
                                          ("metadata", kv), ("stream", None)],
        # (this entry checks the strides for every n_seqs: one sequence passes its capacities)
        "quest_step_state_advance_batched, one sequence": [("state", ONE), ("kv_table", ONE), ("meta_table", ONE),
                                                           ("page_size", 16), ("max_kv", 104), ("max_meta", 8),
                                                           ("=batch", _b(1, 104, 8)), ("stream", None)],
        "quest_step_state_advance_batched": [("state", ONE), ("kv_table", ONE), ("meta_table", ONE), ("page_size", 16),
                                             ("max_kv", 104), ("max_meta", 8), ("batch", b), ("stream", None)],
        "quest_estimate_attn_score": [("q", ONE), ("o", ONE), ("hq", 32), ("n", MAX_N), ("metadata", kv), ("stream", None)],
        "quest_estimate_attn_score_batched": [("q", ONE), ("o", ONE), ("hq", 32), ("stride", 104), ("n", MAX_N),
                                              ("metadata", kv), ("state", ONE), ("batch", b), ("stream", None)],
        "quest_append_estimate, contiguous rows": est + [("n", MAX_N), contiguous, ("metadata", kv), ("stream", None)],
        "quest_append_estimate": est + [("n", MAX_N), ("stride", 104), ("metadata", kv), ("stream", None)],
        "quest_append_estimate_batched, one sequence": est + [("stride", 104), ("n", MAX_N), whole, ("metadata", kv),
                                                              ("state", ONE), one, ("stream", None)],
        "quest_append_estimate_batched, one sequence, tiles": est + [("stride", TSTRIDE), ("n", MAX_N), ("off", OFF),
                                                                     ("metadata", kv), ("state", ONE), one, ("stream", None)],
        "quest_append_estimate_batched": est + [("stride", 104), ("n", MAX_N), whole, ("metadata", kv), ("state", ONE),
                                                ("batch", b), ("stream", None)],
        "quest_append_estimate_batched, tiles": est + [("stride", TSTRIDE), ("n", MAX_N), ("off", OFF), ("metadata", kv),
                                                       ("state", ONE), ("batch", b), ("stream", None)],
    }


def _call(ent, name, rep):
    """(C entry, its arguments in order) of a case; the handler still as the "h" placeholder."""
    args = dict(ent[name])
    args.update(rep)
    return name.split(",")[0], args


def _key(v):
    if isinstance(v, ctypes.Structure):
        return tuple(_key(getattr(v, f)) for f, _ in v._fields_)
    return v.value if isinstance(v, ctypes.c_void_p) else v


# handler states: None = NULL handler, "new" = created, never planned, a dict = planned with these values
PLAN = dict(n_sel=8, hq=32, hkv=32, d=128, ps=16, batch=64)


def _plan(**kw):
    p = dict(PLAN)
    p.update(kw)
    return p


def _cases():
    """(entry, handler state, {argument: value} replacing the well-formed ones)."""
    ent = _entries()
    out = []
    pools = dict(layout=1, head_dim=64, page_size=32, num_heads=16)  # each differs from the plan / the other pool
    for name, args in ent.items():
        names = [a for a, _ in args]
        has_h = "h" in names
        states = [PLAN] if has_h else [None]
        if has_h:
            out.append((name, None, {}))
            out.append((name, "new", {}))
            out.append((name, None, {"q": None}))
        out.append((name, states[0], {}))  # well-formed
        for st in (["new", PLAN] if has_h else [None]):
            for a, v in args:  # each operand NULL (lse and the optional outputs may be NULL: stay well-formed)
                if v is ONE:
                    out.append((name, st, {a: None}))
        st = states[0]
        if "batch" in names:
            out.append((name, st, {"batch": _b(0)}))
            out.append((name, st, {"batch": _b(65)}))   # the plan is for 64 sequences
            out.append((name, st, {"batch": _b(1, 0, 0)}))
            out.append((name, st, {"batch": _b(2, 8, 8)}))    # page tables shorter than the rows
            out.append((name, st, {"batch": _b(2, 104, 6)}))  # 6 metadata pages x 16 entries < 100
        if "hq" in names:
            out.append((name, st, {"hq": 64}))
            out.append((name, st, {"hq": 48}))
            out.append((name, st, {"hq": 0}))
        for pool in ("kv", "metadata"):
            if pool not in names:
                continue
            for f, v in pools.items():
                out.append((name, st, {pool: _kv(**{f: v})}))
                if has_h:
                    out.append((name, "new", {pool: _kv(**{f: v})}))
            if "kv" in names and "metadata" in names:  # both pools changed alike: the plan (if any) is what differs
                for f, v in pools.items():
                    out.append((name, st, {"kv": _kv(**{f: v}), "metadata": _kv(**{f: v})}))
            for kw in (dict(data=0), dict(indices=0), dict(indptr=0), dict(layout=3), dict(head_dim=96), dict(num_heads=0),
                       dict(page_size=0), dict(last_page_len=0), dict(last_page_len=17), dict(page_budget=4)):
                out.append((name, st, {pool: _kv(**kw)}))
            if has_h:
                out.append((name, "new", {pool: _kv(data=0)}))
                out.append((name, "new", {pool: _kv(head_dim=96)}))
        if "n" in names:
            for n in (0, 4, 105, 4097, 16384, 16385):
                out.append((name, st, {"n": n}))
                out.append((name, st, {"n": n, "stride": (n + 7) // 8 * 8 + 8 * ((n + 63) // 64)}))
            if has_h:
                out.append((name, "new", {"n": 105}))
                out.append((name, "new", {"n": 16385, "stride": 20000}))
        if "stride" in names:
            for s in (0, 99, 100, 101, 102, 103, 107, 108, 112, 116):
                out.append((name, st, {"stride": s}))
            if has_h:
                out.append((name, "new", {"stride": 99}))
        if "off" in names:
            for o in (0, 100, 96, 112):
                out.append((name, st, {"off": o}))
            out.append((name, st, {"off": 112, "stride": 136}))
            if has_h:
                out.append((name, "new", {"off": 0}))
        for a in ("scores", "o"):
            if a in names and ("off" in names or a == "scores"):
                out.append((name, st, {a: ctypes.c_void_p(24)}))  # 8-byte aligned only
                out.append((name, st, {a: ctypes.c_void_p(18)}))
        if has_h:  # plans the entry does not serve, or serves by another route
            for p in (_plan(d=256), _plan(d=64), _plan(ps=32), _plan(hkv=8), _plan(hkv=16), _plan(n_sel=0), _plan(n_sel=255),
                      _plan(n_sel=200, ppc=1000), _plan(front_end=1), _plan(front_end=2), _plan(layout=1), _plan(layout=2)):
                kv = _kv(head_dim=p["d"], page_size=p["ps"], num_heads=p["hkv"], layout=p.get("layout", 0))
                rep = {"kv": kv}
                if "metadata" in names:
                    rep["metadata"] = kv
                out.append((name, p, rep))
                if "n" in names:
                    out.append((name, p, dict(rep, n=300, stride=304 if "off" not in names else 328, off=304)))
                    out.append((name, p, dict(rep, n=5000, stride=5001, off=5000)))
                    out.append((name, p, dict(rep, n=5000, stride=5008 + 640, off=5000)))
    # named rules of single entries
    n = "quest_decode_forward_batched"
    out += [(n, PLAN, {"idx_stride": 7}), (n, "new", {"idx_stride": 7}), (n, PLAN, {"idx_stride": 0}),
            (n, _plan(n_sel=0), {"idx_stride": 0})]
    n = "quest_decode_forward"
    out += [(n, PLAN, {"kv": _kv(page_budget=7)}), (n, _plan(n_sel=0), {"kv": _kv(indices=0)})]
    n = "quest_decode_layer_fused_batched"
    out += [(n, PLAN, {"scores_out": ONE, "stride": 99}), (n, PLAN, {"scores_out": ONE, "stride": 100}),
            (n, "new", {"scores_out": ONE, "stride": 99}), (n, PLAN, {"n": 4097, "batch": _b(2, 5000, 500)}),
            (n, PLAN, {"n": 4096, "batch": _b(2, 5000, 500)})]
    n = "quest_append_kv_cache_prefill"
    out += [(n, None, {"append_len": 0}), (n, None, {"n_pages": 0}), (n, None, {"append_len": 50}),
            (n, None, {"append_len": 49})]
    for n in ("quest_step_state_advance_batched, one sequence", "quest_step_state_advance_batched"):
        out += [(n, None, {a: 0}) for a in ("page_size", "max_kv", "max_meta")]
    n = "quest_step_state_advance_batched"
    out += [(n, None, {"max_kv": 105}), (n, None, {"max_meta": 9})]
    out = [(name, st, rep) for name, st, rep in out if all(k in dict(ent[name]) for k in rep)]
    seen, once = set(), []
    for name, st, rep in out:  # two forms that come to the same call of the same entry: made once
        entry, args = _call(ent, name, rep)
        k = (entry, "new" if st == "new" else st and tuple(sorted(st.items())), tuple(_key(v) for v in args.values()))
        if k not in seen:
            seen.add(k)
            once.append((name, st, rep))
    return once


def _run(lib, cases):
    """The code each case returns, as one letter of CODES."""
    ent = _entries()
    handlers, codes = {}, []

    def handler(st):
        if st is None:
            return None
        key = "new" if st == "new" else tuple(sorted(st.items()))
        if key not in handlers:
            h = ctypes.c_void_p()
            assert lib.quest_decode_handler_create(ctypes.byref(h), 0 if st == "new" else st.get("layout", 0)) == 0
            handlers[key] = h
            if st != "new":
                assert lib.quest_decode_set_batch(h, st["batch"]) == 0
                assert lib.quest_decode_set_pages_per_chunk(h, st.get("ppc", 0)) == 0
                assert lib.quest_decode_set_front_end(h, st.get("front_end", 0)) == 0
                assert lib.quest_decode_begin_forward(h, st["n_sel"], st["hq"], st["hkv"], st["d"], st["ps"], None) == 0, st
                chunks = ctypes.c_uint32()
                assert lib.quest_decode_plan_info(h, None, ctypes.byref(chunks)) == 0 and chunks.value == 1
        return handlers[key]

    try:
        for name, st, rep in cases:
            entry, args = _call(ent, name, rep)
            if "h" in args:
                args["h"] = handler(st)
            code = getattr(lib, entry)(*args.values())
            codes.append(LAUNCHED if code > 0 else CODES[code])
    finally:
        for h in handlers.values():
            lib.quest_decode_handler_destroy(h)
    return "".join(codes)


def _device_visible():
    import torch

    return torch.cuda.is_available()


def test_entry_return_codes_match_the_recorded_table():
    from quest_amd._lib import lib

    cases, want = _cases(), "".join(EXPECTED.split())
    assert len(cases) == len(want) and len(cases) > 1500
    for name in _entries():  # every entry: refused for an argument, (handler entries) for the plan, and launched when well-formed
        seen = {w for (n, _, _), w in zip(cases, want) if n == name}
        assert CODES[EINVAL] in seen and LAUNCHED in seen, name
        assert CODES[ESTATE] in seen or not name.startswith("quest_decode_"), name
    if _device_visible():  # calls that reach a launch are not made where a device would run them on the fake operands
        cases, want = zip(*[(c, w) for c, w in zip(cases, want) if w != LAUNCHED])
    got = _run(lib, cases)
    bad = [(i, c[0], c[1] if not isinstance(c[1], dict) else {k: v for k, v in c[1].items() if PLAN.get(k) != v}, w, g)
           for i, (c, w, g) in enumerate(zip(cases, want, got)) if g != w]
    assert not bad, f"{len(bad)} of {len(cases)} differ (case, entry, handler, recorded, got): {bad[:12]}"


# one letter per case of _cases(), in order
EXPECTED = """
ISILSSIIIIIISISISISIILIIIIIIISSLLLLLLIILLLLISILSSIIIIIISISISISIILIIIIIILSSULULLLLLLLLLISILSSIIIIIIIISISISISIILIIIILLLSSL
LLLLLLLLLLLISILSSIIIIISILIIIISISISISIILIIIILLLSSLLLLLLIILLLLISILIISSIIIIIIIIIISISISISIIIIIILIIIILLLSSISISISISILLIIIILLLS
SULULLLLLLLLLISILIISSIIIIIIISILIIIISISISISIIIIIILIIIILLLSSISISISISILLIIIILLLSSULULLLIILLLLISILSSIIIIIIIISISISISIILIIIIII
LSSIILLLTSLLLLLLLIIILLLLISILSSIIIIIIIISISISISIILIIIIIILSSIIIILILILITISILLLLLLLLILLLLLLLIIILLLLISILSSIIIIIIIIIISISISISIIL
IIIILLLSSIIIIILILILITISIILLLLLLLLILLLLLLLIIILLLLISILSSIIIIIIIIIISISISISIILIIIILLLSSIIIIIIIIIIITSSIIIIIIIIIIILIIIISIILLLI
ILLIILUIIULIILLIILIIIIIIILIUUULIILLIILLIILLIILISILSSIIIIIIISILIIIISISISISIILIIIILLLSSIIIIIIIIIIIIIIIILLLLLLLLILLLLLLLIII
LLLLISILSSIIIIIIISILIIIISISISISIILIIIILLLSSIIIIIIIIIIIIIIIIIIIIIIIIILIIIISIILLLIIILIIIUIIILIIILIIIIIIIIIIIIIIILIIILIIILI
IILIIIISILSSIIIIIIISLLLIIIISISISISILLIIIILLLSSLLLLLLIILLLLISILIIIIIIIIIIISLIIIIIISISISISIIIIIILIUIILLLSSISISISISIILIUIIL
LLSSILLIIIIIIIISSLLLLLLLLLSULULLULLLLLLLIILILILLLLIILIUIIIILLILIIILIUIIIILLIIILILILLLLIILIUIILLLLILIIILIUIILLLLIIIILLLLI
LILLLLIILIUIILLLLILIIILIUIILLLLIILILILLLLIIIIUIIIILLILIIIIIUIIIILLIIILIIIILIIILIILIILLLLIILIUIILLL0LLLLLLIIIILLLILIILLLL
IILIUIILLLIILLILIIIIIIIILLLLLLLLLIIIILIILILILLLLIILIUIIIILLILIIILIUIIIILLLLLLLLIIIILIILILILLLLIILIUIIIILLILIIILIUIIIILLL
LILILILILILLLLLLLLLIIIIILIILILILLLLIILIUIILLLLILIIILIUIILLLIILLILILILILIILLLLLLLLLIIIIILIILILILLLLIILIUIILLLLILIIILIUIIL
LLIIIIIIIIIIIIIIIIIIIIIILIIIIIILIIIIIILLILIILILILLLLIILIUIILLLLILIIILIUIILLLIILLILIIIIIIIILLLLLLLLLIIIIIILLILIILILILLLLI
ILIUIILLLLILIIILIUIILLLIIIIIIIIIIIIIIIIIIIIIILIIIIIIISILILILSULIIILIIIIIIII
"""


if __name__ == "__main__":
    import os
    import sys
    import textwrap

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from quest_amd._lib import lib as _lib

    assert not _device_visible(), "record on a machine without a device (the well-formed calls go as far as the launch)"
    print("\n".join(textwrap.wrap(_run(_lib, _cases()), 120)))
