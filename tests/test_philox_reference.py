"""The host reference of the random streams (philox_reference.py) against published known answers and against itself.  No GPU."""
import numpy as np

import philox_reference as ref

# counter, key -> output.  The first and the third are Random123's published vectors (kat_vectors: philox4x32 10); the second is the
# all-ones case of the same file.
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        assert ref.philox4x32_10(*counter, *key) == want
        got = ref.philox4x32_10_array(*(np.array([c]) for c in counter), *key)
        assert tuple(int(word[0]) for word in got) == want


def test_scalar_form_matches_vectorised_form():
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, size=(6, 3000), dtype=np.uint64)
    words[:, 0] = 0
    words[:, 1] = 0xFFFFFFFF
    words[0, 2:66] = np.arange(64)                    # consecutive counters, as the kernels use them
    got = np.stack(ref.philox4x32_10_array(*words))
    assert got.dtype == np.uint64 and int(got.max()) <= ref.MASK32
    for n in range(words.shape[1]):
        assert ref.philox4x32_10(*(int(v) for v in words[:, n])) == tuple(int(v) for v in got[:, n])
    # broadcasting: scalars against an array
    x = ref.philox4x32_10_array(np.arange(64), 1, 2, 3, 0xdeadbeef, 0x12345678)[0]
    assert [int(v) for v in x] == [ref.philox4x32_10(lane, 1, 2, 3, 0xdeadbeef, 0x12345678)[0] for lane in range(64)]


def test_uniform_keeps_the_top_24_bits():
    assert ref.uniform(0) == 0.0 and ref.uniform(0xFF) == 0.0 and ref.uniform(0x100) == 2.0 ** -24
    assert ref.uniform(0xFFFFFFFF) == 1.0 - 2.0 ** -24
    bits = np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
    assert ref.uniform(bits).tolist() == [ref.uniform(int(b)) for b in bits]
    assert np.array_equal(ref.uniform(bits).astype(np.float32).astype(np.float64), ref.uniform(bits))      # exact in float32


def _picks_by_hand(cdf, seed, step, count):
    """Candidate j's pick from the scalar Philox and a linear walk over the prefix sums."""
    total, picks = int(cdf[-1]), []
    for j in range(count):
        x, y, _, _ = ref.philox4x32_10(j, 0, step & ref.MASK32, (step >> 32) ^ ref.TABLE_TAG, seed & ref.MASK32, seed >> 32)
        target = (((x << 32) | y) * total) >> 64
        picks.append(next(i for i, c in enumerate(cdf) if int(c) > target))
    return picks


def test_table_emulation_on_cases_small_enough_to_enumerate():
    seed, step = (1 << 40) + 11, (1 << 33) + 4
    # three weights 1 : 2 : 3, k = 3: the first three distinct picks, in candidate order
    cdf = np.array([1, 3, 6], dtype=np.uint64)
    picks = _picks_by_hand(cdf, seed, step, 64)
    assert set(picks) == {0, 1, 2}
    order = list(dict.fromkeys(picks))
    draw = ref.table_draw(cdf, 3, seed, step)
    assert draw.out.tolist() == order and draw.candidates == 2048 and draw.accepted == 3 and not draw.incomplete
    assert ref.table_picks(cdf, 0, 64, seed, step).tolist() == picks
    assert ref.table_draw(cdf, 2, seed, step).out.tolist() == order[:2]
    assert ref.table_draw(cdf, 3, seed, step, remap=[10, 20, 30]).out.tolist() == [10 * (i + 1) for i in order]
    assert ref.table_draw(cdf, 3, seed, step + 1).out.tolist() == list(dict.fromkeys(_picks_by_hand(cdf, seed, step + 1, 64)))
    # a zero weight in the middle is never picked; asking for more than the positives leaves -1 in the tail
    cdf = np.array([5, 5, 9], dtype=np.uint64)
    draw = ref.table_draw(cdf, 4, seed, step)
    assert sorted(draw.out[:2].tolist()) == [0, 2] and draw.out[2:].tolist() == [-1, -1] and draw.accepted == 2 and not draw.incomplete
    assert draw.out[:2].tolist() == list(dict.fromkeys(_picks_by_hand(cdf, seed, step, 64)))
    # one entry with 2^-63 of the mass is not met in 32768 candidates: the draw ends short and repeats its first picks
    cdf = np.array([1, 1 << 62, 1 << 63], dtype=np.uint64)
    draw = ref.table_draw(cdf, 5, seed, step)
    first = list(dict.fromkeys(_picks_by_hand(cdf, seed, step, 64)))
    assert sorted(first) == [1, 2]
    assert draw.incomplete and draw.candidates == 32768 and draw.accepted == 2 and draw.out.tolist() == first + first[:1] + [-1, -1]


def test_table_prefix_sums_and_race_keys_on_small_inputs():
    weights = np.array([0.5, 0.0, 2.0, 1.0e-30, -1.0], dtype=np.float32)
    cdf = ref.table_prefix_sums(weights)                          # 5 weights: b = 52 (capped), scale = 2^52 / 2
    assert cdf.tolist() == [1 << 50, 1 << 50, (1 << 50) + (1 << 52), (1 << 50) + (1 << 52) + 1, (1 << 50) + (1 << 52) + 1]
    seed, step = 7, (1 << 33) + 4
    keys = ref.race_keys(weights, seed, step)
    for i, w in enumerate(weights.tolist()):
        x = ref.philox4x32_10(i, 0, step & ref.MASK32, (step >> 32) ^ ref.RACE_TAG, seed, 0)[0]
        want = w / (-np.log1p(-ref.uniform(x)) + 1.0e-30) if w > 0 else 0.0
        assert keys[i] == want


def test_render_uniforms_follow_the_formula():
    seed, offset, R, S = (3 << 32) + 7, (5 << 32) + 3, 3, 5
    uc, uf = ref.render_uniforms(R, S, seed, offset)
    for ray in range(R):
        words = [ref.philox4x32_10(ray, s, 3, 5, 7, 3) for s in range(S)]
        assert uc[ray].tolist() == [ref.uniform(w[0]) for w in words]
        e = [-np.log1p(-ref.uniform(w[1])) for w in words]
        total = sum(e) + -np.log1p(-ref.uniform(words[0][2]))
        assert np.allclose(uf[ray], np.cumsum(e) / total, rtol=1e-15, atol=0)
    assert np.all(np.diff(uf, axis=1) > 0) and uf.max() < 1.0
