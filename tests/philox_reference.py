"""Host reference of the library's random streams (test_philox_reference.py on the host, test_hip_random_streams.py on the GPU).

Philox4x32-10 written from its specification (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
known answers are in test_philox_reference.py), once on Python ints and once vectorised over numpy uint64, and on top of it the three
consumers of the library, keyed as INTEGRATION.md ("Random streams") says:

    render / step samples   counter (ray, sample, lo32(stream_offset), hi32(stream_offset))            x: coarse u, y: fine spacing,
                                                                                                       z of sample 0: (S+1)-th spacing
    race sampler            counter (lo32(i), hi32(i), lo32(step), hi32(step) ^ 0x52415953)            x
    table sampler           counter (candidate number, 0, lo32(step), hi32(step) ^ 0x52415954)         (x << 32) | y

all with key (lo32(seed), hi32(seed)).  Everything here is integers, or float64 formulas over exact integers: no statistics."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # multipliers of counter words 0 and 2
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments (golden ratio, sqrt(3) - 1)
MASK32 = 0xFFFFFFFF
RACE_TAG, TABLE_TAG = 0x52415953, 0x52415954          # "RAYS", "RAYT": xor-ed into the fourth counter word

TABLE_BLOCK = 2048                         # candidates per round of the table draw
TABLE_BLOCKS = 16                          # rounds before a draw gives up
FINE_CLAMP = 0.99999994                    # the largest float32 below 1 (the fine uniforms are clamped to it)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Python ints (each < 2^32) -> the four output words."""
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox4x32_10_array(c0, c1, c2, c3, k0, k1):
    """The same over numpy arrays (anything that broadcasts; values < 2^32) -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1)))
    mask, shift = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2           # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> shift) ^ c1 ^ k0, p1 & mask, (p0 >> shift) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c0, c1, c2, c3


def uniform(bits):
    """32 random bits -> [0, 1): the top 24 bits times 2^-24 (exact in float32 and in float64)."""
    if isinstance(bits, np.ndarray):
        return (bits >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return (int(bits) >> 8) * 2.0 ** -24


def _halves(value):
    value = int(value) & 0xFFFFFFFFFFFFFFFF
    return value & MASK32, value >> 32


# ---- render / step samples ------------------------------------------------------------------------------------------------------------

def render_uniforms(num_rays, num_samples, seed, stream_offset):
    """-> (u_coarse [R,S], u_fine [R,S]) in float64.  u_coarse is exact (24-bit values); u_fine is the float64 value of the kernels'
    formula: partial sums of the S exponential spacings -log1p(-uniform(y)) over their sum plus the (S+1)-th spacing (z of sample 0),
    clamped to the largest float32 below 1."""
    (o0, o1), (k0, k1) = _halves(stream_offset), _halves(seed)
    ray, sample = np.meshgrid(np.arange(num_rays), np.arange(num_samples), indexing="ij")
    x, y, z, _ = philox4x32_10_array(ray, sample, o0, o1, k0, k1)
    spacing = -np.log1p(-uniform(y))
    extra = -np.log1p(-uniform(z[:, 0]))
    fine = np.cumsum(spacing, axis=1) / (spacing.sum(axis=1) + extra)[:, None]
    return uniform(x), np.minimum(fine, FINE_CLAMP)


# ---- race sampler ---------------------------------------------------------------------------------------------------------------------

def race_uniforms(count, seed, step):
    (s0, s1), (k0, k1) = _halves(step), _halves(seed)
    index = np.arange(count, dtype=np.uint64)
    x, _, _, _ = philox4x32_10_array(index & np.uint64(MASK32), index >> np.uint64(32), s0, s1 ^ RACE_TAG, k0, k1)
    return uniform(x)


def race_keys(weights, seed, step):
    """float64 keys of the exponential race: w / (Exp(1) + 1e-30) for w > 0, else 0.  `weights`: the float32 values the device reads."""
    w = np.asarray(weights, dtype=np.float64)
    e = -np.log1p(-race_uniforms(w.size, seed, step)) + 1.0e-30
    return np.where(w > 0, w / e, 0.0)


# ---- table sampler --------------------------------------------------------------------------------------------------------------------

def table_prefix_sums(weights):
    """The table's inclusive prefix sums (uint64) of float32 `weights`: fixed-point weights max(1, floor(w 2^b / max w)) for w > 0,
    b = min(62 - ceil(log2 count), 52)."""
    w32 = np.asarray(weights, dtype=np.float32)
    w = w32.astype(np.float64)
    count = w.size
    bits = min(62 - (int(np.ceil(np.log2(count))) if count > 1 else 0), 52)
    scale = np.ldexp(1.0, bits) / float(w32.max())
    fixed = np.where(w > 0, np.maximum((np.maximum(w, 0.0) * scale).astype(np.uint64), 1), 0).astype(np.uint64)
    return np.cumsum(fixed, dtype=np.uint64)


def table_picks(cdf, first, count, seed, step):
    """The picks of candidates first .. first + count - 1: searchsorted(cdf, (bits * total) >> 64, side="right")."""
    (s0, s1), (k0, k1) = _halves(step), _halves(seed)
    x, y, _, _ = philox4x32_10_array(np.arange(first, first + count), 0, s0, s1 ^ TABLE_TAG, k0, k1)
    total = int(cdf[-1])
    targets = [(((int(a) << 32) | int(b)) * total) >> 64 for a, b in zip(x, y)]           # 128-bit products: Python ints
    return np.searchsorted(cdf, np.array(targets, dtype=np.uint64), side="right")


class TableDraw:
    """What one draw did: `out` int64 [k], `candidates` drawn (a multiple of 2048), `accepted` distinct picks among them, `incomplete`
    (the sixteen blocks ended short and the tail repeats the first picks)."""

    def __init__(self, out, candidates, accepted, incomplete):
        self.out, self.candidates, self.accepted, self.incomplete = out, candidates, accepted, incomplete


def table_draw(cdf, k, seed, step, remap=None):
    """Emulation of one draw of k indices from the table with inclusive prefix sums `cdf` (uint64, total > 0)."""
    cdf = np.asarray(cdf, dtype=np.uint64)
    positives = int(np.count_nonzero(np.diff(cdf, prepend=np.uint64(0))))
    need = min(int(k), positives)
    seen, kept, blocks = set(), [], 0
    while blocks < TABLE_BLOCKS and len(kept) < need:
        for pick in table_picks(cdf, blocks * TABLE_BLOCK, TABLE_BLOCK, seed, step).tolist():      # the whole block, in candidate order
            if pick not in seen:
                seen.add(pick)
                kept.append(pick)
        blocks += 1
    accepted = len(kept)
    out = np.full(int(k), -1, dtype=np.int64)
    head = np.array(kept[:k], dtype=np.int64)
    out[:head.size] = head if remap is None else np.asarray(remap, dtype=np.int64)[head]
    incomplete = accepted < need
    if incomplete:
        for i in range(accepted, need):
            out[i] = out[(i - accepted) % accepted]
    return TableDraw(out, blocks * TABLE_BLOCK, accepted, incomplete)
