"""CPU checks of the sampling contract's float64 restatement (tests/_sampling_ref.py): the Philox generator against the
published Random123 vectors, the uniforms, the kept set against transformers' warpers, the draw's distribution, and -- from
the restatement alone -- that the GPU tests' inputs are decidable within the cap and what EPS_Z they yield."""
import numpy as np
import pytest

import _sampling_ref as ref


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("key,counter,want", [
    ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_reproduces_the_random123_vectors(key, counter, want):
    got = ref.philox4x32_10(np.array(counter, np.uint32), np.array(key, np.uint32))
    assert _hex(got) == want


def test_draw_words_follow_the_counter_layout():
    seed, pos = 0x299F31D0A4093822, 0x85A308D3
    words = ref.draw_words(seed, pos, 11)
    for j in (0, 3, 4, 10):
        one = ref.philox4x32_10(np.array([j >> 2, pos, ref.DRAW_TAG, 0], np.uint32),
                                np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))
        assert words[j] == one[j & 3]


def test_uniform_is_exact_in_float32_and_inside_the_open_interval():
    words = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], np.uint32)
    words = np.concatenate([words, np.random.default_rng(5).integers(0, 2 ** 32, 100000).astype(np.uint32)])
    u = ref.uniforms(words)
    assert u.dtype == np.float32
    exact = ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u.astype(np.float64), exact)
    assert u.min() > 0 and u.max() < 1
    assert np.isfinite(np.log(-np.log(u))).all()


def test_greedy_rule_and_the_order_of_special_values():
    for dtype, one, inf, nan in (("fp16", 0x3C00, 0x7C00, 0x7E00), ("bf16", 0x3F80, 0x7F80, 0x7FC0)):
        neg = lambda b: b | 0x8000
        row = lambda *b: np.array(b, np.uint16)
        s = lambda bits, T=1.0: ref.sample_row(bits, dtype, T, 0, 1.0, 1, 1)
        assert s(row(0, one, one, 0), 0.0).token == 1                      # ties: the lowest index
        assert s(row(one, 0, 0, one), 0.0).token == 0                      # first and last column tie
        assert s(row(neg(0), 0, neg(0)), 0.0).token == 1                   # -0 < +0
        assert s(row(neg(inf), neg(inf), neg(inf))).greedy and s(row(neg(inf),) * 3).token == 0
        r = s(row(one, nan, one))
        assert r.greedy and r.token == 1 and r.kept == 1
        r = s(row(one, inf, inf))
        assert r.greedy and r.token == 1
        r = s(row(one, neg(nan), 0))                                       # a NaN with the sign set sorts last; still greedy
        assert r.greedy and r.token == 0
        assert not s(row(one, neg(inf), 0)).greedy                         # -inf entries alone do not make a row greedy


def test_kept_set_equals_transformers_warpers_on_decided_rows():
    torch = pytest.importorskip("torch")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    V, checked = 1000, 0
    bits = ref.make_logits(4242, 96, V, "fp16")
    combos = [(t, k, p) for t in ref.TEMPERATURES for k in (0, 1, 5, 50, V) for p in (0.0, 0.5, 0.9, 1.0)]
    for i in range(bits.shape[0]):
        T, k, p = combos[i % len(combos)]
        row = ref.sample_row(bits[i], "fp16", T, k, p, 3, 5)
        keys = np.sort(ref.half_key(bits[i]))[::-1]
        k1 = V if k <= 0 else min(k, V)
        tied = lambda n: n < V and keys[n - 1] == keys[n]
        if not row.boundary_decided or tied(k1) or tied(row.kept):
            # transformers' top-k keeps every token that ties with the k-th, the contract exactly k; and at a top-p cut
            # inside a run of equal logits transformers' (unstable) sort decides which of them stay, here the index does
            continue
        scores = torch.from_numpy(ref.to_f64(bits[i], "fp16").astype(np.float32))[None]
        scores = TemperatureLogitsWarper(float(T))(None, scores)
        if k > 0:
            scores = TopKLogitsWarper(int(k))(None, scores)
        if p < 1:
            scores = TopPLogitsWarper(float(p))(None, scores)
        hf_kept = set(np.nonzero(np.isfinite(scores[0].numpy()))[0].tolist())
        ours = set(ref.token_order(bits[i])[:row.kept].tolist())
        assert ours == hf_kept, (i, T, k, p, len(ours), len(hf_kept))
        checked += 1
    assert checked >= 80, checked


def _chi2_critical(df: int, z: float = 3.719) -> float:
    """Upper critical value of chi-square with `df` degrees of freedom at p = 1e-4 (z = its normal quantile), by the
    Wilson-Hilferty cube: df (1 - 2/(9 df) + z sqrt(2/(9 df)))^3; within 2 % of the exact value for df >= 2 at this
    level, and the test adds that 2 %."""
    a = 2.0 / (9.0 * df)
    return 1.02 * df * (1.0 - a + z * np.sqrt(a)) ** 3


@pytest.mark.parametrize("T,top_k,top_p,seed", [(1.0, 0, 1.0, 11), (0.7, 5, 1.0, 12), (1.5, 0, 0.9, 13), (0.8, 6, 0.8, 14)])
def test_draw_frequencies_follow_the_filtered_softmax(T, top_k, top_p, seed):
    V, P = 8, 20000
    bits = ref.to_bits(np.array([1.5, -0.25, 0.75, 1.5, -2.0, 0.0, 2.25, 0.5], np.float32), "fp16")
    first = ref.sample_row(bits, "fp16", T, top_k, top_p, seed, 0)
    assert first.boundary_decided
    order = ref.token_order(bits)
    keep = order[:first.kept]
    s = ref.to_f64(bits, "fp16")
    x = (s - s.max()) / float(np.float32(T))
    prob = np.zeros(V)
    prob[keep] = np.exp(x[keep]) / np.exp(x[keep]).sum()
    # all positions at once: counter (group, pos, tag, 0) for the two groups of a row of 8
    counter = np.zeros((P, 2, 4), np.uint32)
    counter[:, :, 0] = np.arange(2, dtype=np.uint32)[None]
    counter[:, :, 1] = np.arange(P, dtype=np.uint32)[:, None]
    counter[:, :, 2] = ref.DRAW_TAG
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
    u = ref.uniforms(ref.philox4x32_10(counter, key).reshape(P, V)).astype(np.float64)
    z = np.full((P, V), -np.inf)
    z[:, keep] = x[keep][None] - np.log(-np.log(u[:, keep]))
    # ties to the earlier token of the order: argmax over the columns taken in that order
    tokens = order[np.argmax(z[:, order], axis=1)]
    for pos in range(0, 200):  # the vectorised draw is the restatement's
        assert tokens[pos] == ref.sample_row(bits, "fp16", T, top_k, top_p, seed, pos).token
    counts = np.bincount(tokens, minlength=V)
    assert counts[prob == 0].sum() == 0
    expected = prob[keep] * P
    chi2 = float(((counts[keep] - expected) ** 2 / expected).sum())
    bound = _chi2_critical(len(keep) - 1)
    print(f"chi-square {chi2:.2f} over {len(keep)} kept tokens, bound {bound:.2f}")
    assert chi2 < bound


def test_gpu_inputs_are_decidable():
    """From the restatement alone: at most 1 % of the GPU tests' draws are undecided, per case of 16 rows or more and over
    all of them; and EPS_Z is at least 32 x the largest fp32-vs-float64 difference of z over these inputs."""
    rows = undecided = 0
    z_err = 0.0
    seen = set()
    for c in ref.gpu_cases():
        r = ref.case_rows(c.name)
        bad = sum(ref.is_undecided(x) for x in r)
        if c.n >= 16:
            assert bad <= max(1, int(ref.MAX_UNDECIDED * c.n)), (c.name, bad)
        rows += c.n
        undecided += bad
        z_err = max(z_err, max(x.z32_err for x in r))
        seen |= {(float(t), int(k) if k <= c.V else -1, float(p)) for t, k, p in zip(c.temperature, c.top_k, c.top_p)}
    print(f"{rows} rows, {undecided} undecided, max |z_fp32 - z_fp64| = {z_err:.3g}, 32 x = {32 * z_err:.3g}, "
          f"EPS_Z = {ref.EPS_Z:.3g}")
    assert undecided <= ref.MAX_UNDECIDED * rows
    assert 32 * z_err <= ref.EPS_Z
    assert len({(t, p) for t, _, p in seen}) == len(ref.TEMPERATURES) * len(ref.TOP_PS)
