"""The library's random streams against an exact host reference (philox_reference.py): the table sampler's draw bit for bit, the race
sampler's own keys, candidates and order, and the render kernels' exported uniforms element by element.  Needs a real MI355X: run
with ``-m gpu``.

Two tolerances here depend on the hardware's log and reciprocal instructions; both were measured on the MI355X over every case of
this module against the float64 host formulas, and are asserted at four times the worst value seen, rounded up to one significant
digit (docs/OPTLOG.md, "Random streams pinned to a host reference"):

    RACE_KEY_RTOL       relative error of a race key  w / (-log(1 - u) + 1e-30)                 worst seen 1.816e-07, asserted at 8e-7
    FINE_UNIFORM_ATOL   absolute error of a fine uniform  cumsum(e)[s] / (sum(e) + e_extra)     worst seen 2.002e-07, asserted at 9e-7

Both are of float32 rounding size: three units in the last place of a key, and 3.4 x 2^-24 for a uniform below 1 that is a sum of up
to 128 rounded terms times a rounded reciprocal.
"""
import numpy as np
import pytest
import torch

import philox_reference as ref
from conftest import margin

pytestmark = pytest.mark.gpu

RACE_KEY_RTOL = 8.0e-7              # 4 x 1.816e-07 (3.05 x 2^-24: the log, its scaling by ln 2 and the division), rounded up
FINE_UNIFORM_ATOL = 9.0e-7          # 4 x 2.002e-07 (3.4 x 2^-24), rounded up

SEED, STEP = (1 << 40) + 11, (1 << 33) + 4          # both 32-bit words of both are non-zero


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


# ---- the table sampler --------------------------------------------------------------------------------------------------------------

def sized_table_weights(M, seed=3):
    """The weights of test_ray_table_is_exact_and_bounded: rand^4 * 3, 40 % zeros, one entry of 2.5."""
    gen = torch.Generator().manual_seed(seed + M)
    weights = torch.rand(M, generator=gen) ** 4 * 3.0
    weights[torch.rand(M, generator=gen) < 0.4] = 0.0
    weights[M // 2] = 2.5
    return weights


def sparse_weights(M, power, seed):
    gen = torch.Generator().manual_seed(seed)
    weights = torch.rand(M, generator=gen) ** power
    weights[torch.rand(M, generator=gen) < 0.4] = 0.0
    return weights


def check_table_draw(dev, weights, k, seed, step, remap=None, table=None):
    """One device draw against the emulation over the numpy prefix sums; -> (the emulation's record, the table)."""
    from vsrd_amd import rendering
    M = weights.numel()
    cdf = ref.table_prefix_sums(weights.numpy())
    if table is None:
        table = rendering.RayTable(weights.to(dev))
        assert np.array_equal(table.table.cpu().numpy()[64:64 + 8 * M].view(np.uint64), cdf)
    draw = ref.table_draw(cdf, k, seed, step, remap=None if remap is None else remap.numpy())
    got = table.sample(k, seed=seed, stream_offset=step, remap=None if remap is None else remap.to(dev))
    assert torch.equal(got.cpu(), torch.from_numpy(draw.out)), f"M={M} k={k}: first difference at {int((got.cpu() != torch.from_numpy(draw.out)).nonzero()[0])}"
    return draw, table


@pytest.mark.parametrize("M", [1, 17, 4096, 4097, 70001])
def test_table_draw_matches_emulation_at_the_table_sizes(dev, M):
    """RayTable.sample == the host emulation (Philox bits -> umul64hi -> searchsorted -> keep the first k distinct), bit for bit, at
    the table sizes of test_ray_table_is_exact_and_bounded (one entry, a partial chunk, one chunk, one chunk and one entry, 18 chunks)
    and k = 1, 64, 1000 where that many weights are positive."""
    weights = sized_table_weights(M)
    positives = int((weights > 0).sum())
    table, ran = None, 0
    for k in (1, 64, 1000):
        if k > positives:
            continue
        draw, table = check_table_draw(dev, weights, k, seed=11, step=4, table=table)
        assert draw.accepted >= k and bool((weights[torch.from_numpy(draw.out)] > 0).all()) and np.unique(draw.out).size == k
        assert table.incomplete() == draw.incomplete
        ran += 1
    assert ran >= (3 if M >= 4096 else 1)


@pytest.mark.parametrize("case", ["equal_3000", "rand_5000"])
def test_table_draw_of_several_blocks(dev, case):
    """k = 2048 needs more than one block of 2048 candidates (repeats are skipped): the accepted count carries over from block to
    block and the draw stops after the block that completes it.  Candidates used by the emulation: 4096 for 3000 equal weights, 6144
    for rand weights over 5000 entries with 40 % zeros."""
    weights = torch.ones(3000) if case == "equal_3000" else sparse_weights(5000, 1, seed=21)
    draw, table = check_table_draw(dev, weights, 2048, SEED, STEP)
    assert 2048 < draw.candidates < 32768 and not draw.incomplete and not table.incomplete()
    assert draw.candidates == (4096 if case == "equal_3000" else 6144)
    assert np.unique(draw.out).size == 2048


def test_table_draw_that_exhausts_its_candidates(dev):
    """rand^4 weights over 5000 entries (40 % zeros) at k = 2048: all sixteen blocks run, about 2000 distinct picks arrive, the rest of
    the output repeats the first picks in order and the table's sticky flag is raised -- without and with a remap (the repeats are
    copies of the remapped entries)."""
    weights = sparse_weights(5000, 4, seed=22)
    draw, table = check_table_draw(dev, weights, 2048, SEED, STEP)
    assert draw.candidates == 32768 and draw.incomplete and 1024 < draw.accepted < 2048
    assert table.incomplete()
    assert np.array_equal(draw.out[draw.accepted:], draw.out[:2048 - draw.accepted])
    remap = torch.randperm(5000, generator=torch.Generator().manual_seed(5)) + 100000
    mapped, table = check_table_draw(dev, weights, 2048, SEED, STEP, remap=remap)
    assert np.array_equal(mapped.out, remap.numpy()[draw.out]) and table.incomplete()


def test_table_draw_with_fewer_positive_weights_than_samples(dev):
    """100 weights, about 40 of them positive, k = 64: the draw goes on (three blocks in the emulation) until every positive entry has
    been met, the output holds them in the order they were met and -1 behind them."""
    gen = torch.Generator().manual_seed(23)
    weights = torch.rand(100, generator=gen) ** 2.5
    weights[torch.rand(100, generator=gen) < 0.6] = 0.0
    positives = int((weights > 0).sum())
    draw, table = check_table_draw(dev, weights, 64, SEED, STEP)
    assert 30 <= positives < 64 and draw.accepted == positives and not draw.incomplete and not table.incomplete()
    assert draw.candidates == 6144
    assert sorted(draw.out[:positives].tolist()) == torch.nonzero(weights > 0).flatten().tolist() and bool((draw.out[positives:] == -1).all())


def test_table_draw_with_wide_seed_and_step(dev):
    """Seed and step above 2^32 in both words: the high words reach the key and the fourth counter word.  The step as a host integer
    and as a device int64 tensor give the same draw, and neighbouring seeds and steps (in either word) give other draws."""
    weights = sized_table_weights(4097)
    draw, table = check_table_draw(dev, weights, 64, SEED, STEP)
    on_device = table.sample(64, seed=SEED, stream_offset=torch.tensor([STEP], dtype=torch.int64, device=dev))
    assert torch.equal(on_device.cpu(), torch.from_numpy(draw.out))
    for seed, step in ((SEED & 0xFFFFFFFF, STEP), (SEED, STEP & 0xFFFFFFFF), (SEED + (1 << 32), STEP), (SEED, STEP + (1 << 32))):
        other, _ = check_table_draw(dev, weights, 64, seed, step, table=table)
        assert not np.array_equal(other.out, draw.out)


# ---- the race sampler ---------------------------------------------------------------------------------------------------------------

BINS = CANDIDATES = 4096


def run_race(dev, weights, k, seed, step):
    """vsrd_sample_rays with a workspace of the test's own -> (indices [k], the workspace read back as SampleScratch)."""
    from vsrd_amd import _lib
    lib = _lib.load()
    nbytes = int(lib.vsrd_sample_rays_workspace_bytes())
    assert nbytes == 4 * BINS + 16 + 4 * CANDIDATES + 8 * CANDIDATES
    workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    w = weights.to(dev)
    out = torch.full((k,), -7, dtype=torch.int64, device=dev)
    _lib.check(lib.vsrd_sample_rays(_lib.ptr(w), w.numel(), k, seed, step, None, workspace.data_ptr(), nbytes, out.data_ptr(), _lib.stream()))
    raw = workspace.cpu().numpy()
    words = raw[4 * BINS:4 * BINS + 16].view(np.uint32)
    scratch = dict(histogram=raw[:4 * BINS].view(np.uint32).astype(np.int64), threshold_bin=int(words[0]), num_candidates=int(words[1]),
                   overflow=int(words[2]), keys=raw[4 * BINS + 16:8 * BINS + 16].view(np.float32),
                   indices=raw[8 * BINS + 16:].view(np.int64))
    return out.cpu().numpy(), scratch


def check_race(tag, dev, weights, k, seed, step):
    """Every exact property of one call on the device's own numbers, then the candidate set against the float64 host keys.
    -> (output, candidate indices, candidate keys, host keys)."""
    out, s = run_race(dev, weights, k, seed, step)
    w = weights.numpy()
    positives = int((w > 0).sum())
    hist, b, n = s["histogram"], s["threshold_bin"], s["num_candidates"]
    assert int(hist.sum()) == positives
    if positives < k:
        assert b == 0
    else:
        assert int(hist[b + 1:].sum()) < k <= int(hist[b:].sum())
    assert n == int(hist[b:].sum()) and s["overflow"] == 0 and n <= CANDIDATES
    keys, idx = s["keys"][:n], s["indices"][:n]
    assert bool(((keys.view(np.uint32) >> 20) >= b).all()) and bool((keys > 0).all())
    assert np.unique(idx).size == n and bool(((idx >= 0) & (idx < w.size)).all()) and bool((w[idx] > 0).all())
    order = np.lexsort((idx, -keys.astype(np.float64)))                      # key descending, then index ascending
    expected = np.full(k, -1, dtype=np.int64)
    expected[:min(n, k)] = idx[order][:k]
    assert np.array_equal(out, expected)
    # the float64 host keys: how far the device's keys are from them, and that the candidates are the keys above the bin's lower edge
    host = ref.race_keys(w, seed, step)
    if n:
        error = float((np.abs(keys.astype(np.float64) - host[idx]) / host[idx]).max())
        print(f"[{tag}] candidates {n}, threshold bin {b}, worst relative key error {error:.3e} = {error * 2 ** 24:.2f} x 2^-24")
        assert margin(tag, "race key rel error", error, RACE_KEY_RTOL) <= RACE_KEY_RTOL
    edge = float(np.array([b << 20], dtype=np.uint32).view(np.float32)[0])
    is_candidate = np.zeros(w.size, dtype=bool)
    is_candidate[idx] = True
    assert bool(is_candidate[host > edge * (1.0 + RACE_KEY_RTOL)].all())
    assert bool((host[idx] >= edge * (1.0 - RACE_KEY_RTOL)).all())
    near = int(((host > 0) & (host >= edge * (1.0 - RACE_KEY_RTOL)) & (host <= edge * (1.0 + RACE_KEY_RTOL))).sum())
    assert near <= 0.01 * n, f"{near} host keys within the key tolerance of the threshold edge"
    return out, idx, keys, host


def race_weights(count, seed=1):
    gen = torch.Generator().manual_seed(seed + count)
    weights = torch.rand(count, generator=gen) ** 3
    weights[torch.rand(count, generator=gen) < 0.3] = 0.0
    return weights


@pytest.mark.parametrize("k", [1, 64, 2048])
@pytest.mark.parametrize("count", [1, 255, 256, 257, 70001])
def test_race_sampler_is_the_k_largest_keys(dev, count, k):
    """vsrd_sample_rays on its own workspace: the histogram counts every positive weight once, the threshold bin satisfies its
    definition, the candidate list is exactly the keys in or above that bin, and the output is the first k candidates by (key
    descending, index ascending), -1 behind them.  Against the float64 host keys (Philox u exact, w / (-log1p(-u) + 1e-30)): every
    index whose host key is above the bin's lower edge by more than the key tolerance is a candidate, none lies below it.
    Measured on the MI355X over all cases of this module (these, 200 000 weights, 1.2 M equal weights, ten positive weights): worst
    relative key error 1.816e-07 = 3.05 x 2^-24 (1.2 M equal weights; 1.812e-07 at 256 weights), asserted at 8e-7."""
    weights = race_weights(count)
    out, idx, keys, host = check_race(f"test_race_sampler_is_the_k_largest_keys[{count}-{k}]", dev, weights, k, SEED, STEP)
    positives = int((weights > 0).sum())
    assert int((out >= 0).sum()) == min(k, positives)
    if positives < k:                                                         # everything positive, best key first, then -1
        assert sorted(out[:positives].tolist()) == torch.nonzero(weights > 0).flatten().tolist()


def test_race_sampler_grid_stride_of_the_histogram(dev):
    """200 000 weights: more than the histogram kernel's 512 x 256 threads, so its grid-stride loop runs twice for some threads."""
    weights = race_weights(200000)
    out, idx, keys, host = check_race("test_race_sampler_grid_stride_of_the_histogram", dev, weights, 1000, SEED, STEP)
    assert int((out >= 131072).sum()) > 100 and int((out < 131072).sum()) > 100 and np.unique(out).size == 1000


def test_race_sampler_breaks_ties_by_index(dev):
    """1.2 M equal weights, k = 2048: more than the collect kernel's 4096 x 256 threads (its loop runs twice), and with 24-bit
    uniforms exact key ties occur among the best 2048 -- asserted on the host keys -- so the order by index within a tie decides
    output positions."""
    count, k = 1200000, 2048
    weights = torch.ones(count)
    top = np.sort(ref.race_keys(weights.numpy(), SEED, STEP))[-k:]
    ties = int((top[1:] == top[:-1]).sum())
    assert ties >= 1 and top[0] > 0
    out, idx, keys, host = check_race("test_race_sampler_breaks_ties_by_index", dev, weights, k, SEED, STEP)
    assert int((idx >= 4096 * 256).sum()) > 0
    chosen = host[out]
    tied = np.nonzero(chosen[1:] == chosen[:-1])[0]
    assert tied.size >= ties and bool((out[tied] < out[tied + 1]).all())     # equal u -> equal device keys: the smaller index first
    print(f"[test_race_sampler_breaks_ties_by_index] {ties} tied neighbours among the best {k} host keys")


def test_race_sampler_with_ten_positive_weights(dev):
    """1000 weights of which 10 are positive, k = 32: threshold bin 0, the ten indices best key first, then -1."""
    weights = torch.zeros(1000)
    weights[torch.randperm(1000, generator=torch.Generator().manual_seed(9))[:10]] = torch.rand(10, generator=torch.Generator().manual_seed(10)) + 0.1
    out, idx, keys, host = check_race("test_race_sampler_with_ten_positive_weights", dev, weights, 32, SEED, STEP)
    assert sorted(out[:10].tolist()) == torch.nonzero(weights > 0).flatten().tolist() and bool((out[10:] == -1).all())
    assert np.array_equal(out[:10], np.argsort(-host, kind="stable")[:10])   # ten keys far apart: the host order is the device order


def test_race_sampler_reads_the_step_on_the_device(dev):
    """A wide step read from device memory keys the same stream as the same step passed by value."""
    from vsrd_amd import rendering
    weights = race_weights(70001).to(dev)
    by_value = rendering.sample_rays(weights, 64, seed=SEED, stream_offset=STEP)
    on_device = rendering.sample_rays(weights, 64, seed=SEED, stream_offset=torch.tensor([STEP], dtype=torch.int64, device=dev))
    assert torch.equal(by_value, on_device)
    host = ref.race_keys(weights.cpu().numpy(), SEED, STEP)
    best = np.argsort(-host, kind="stable")[:64]
    gaps = host[best][:-1] / host[best][1:] - 1.0
    if gaps.min() > 2.0 * RACE_KEY_RTOL:                                      # (no two of the best keys within the key tolerance: one order)
        assert np.array_equal(by_value.cpu().numpy(), best)


# ---- the render kernels' uniforms -----------------------------------------------------------------------------------------------------

SAMPLE_COUNTS = [2, 15, 16, 17, 63, 64, 65, 100, 128]
RAY_COUNTS = [1, 5, 37]


def scene(N, R, seed=0):
    """Boxes rotated about y in front of a camera at the origin, rays aimed near them."""
    g = torch.Generator().manual_seed(1000 * N + R + seed)
    loc = torch.stack([torch.empty(N).uniform_(-6, 6, generator=g), torch.empty(N).uniform_(-1.0, 1.5, generator=g),
                       torch.empty(N).uniform_(8, 30, generator=g)], -1)
    dim = torch.stack([torch.empty(N).uniform_(0.75, 1.0, generator=g), torch.empty(N).uniform_(0.75, 1.0, generator=g),
                       torch.empty(N).uniform_(1.5, 2.5, generator=g)], -1)
    yaw = torch.empty(N).uniform_(-3.1, 3.1, generator=g)
    rot = torch.stack([torch.stack([torch.cos(yaw), torch.zeros(N), torch.sin(yaw)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                       torch.stack([-torch.sin(yaw), torch.zeros(N), torch.cos(yaw)], -1)], -2)
    target = loc[torch.randint(0, N, (R,), generator=g)] + torch.randn(R, 3, generator=g) * 0.7
    return dict(loc=loc, dim=dim, rot=rot, origins=torch.zeros(R, 3), directions=torch.nn.functional.normalize(target, dim=-1),
                targets=torch.rand(R, N, generator=g), mlp=torch.randn(N, 1617, generator=g) * 0.3)


_REFERENCE_UNIFORMS = {}


def reference_uniforms(R, S):
    """(u_coarse float32 [R,S], u_fine float64 [R,S]) of (SEED, STEP), computed once per shape and shared."""
    if (R, S) not in _REFERENCE_UNIFORMS:
        coarse, fine = ref.render_uniforms(R, S, SEED, STEP)
        _REFERENCE_UNIFORMS[(R, S)] = (torch.from_numpy(coarse.astype(np.float32)), torch.from_numpy(fine))
    return _REFERENCE_UNIFORMS[(R, S)]


def exported_uniforms(dev, how, N, S, R):
    """The uniforms one launch says it used, keyed by (SEED, STEP)."""
    from vsrd_amd import fields, rendering
    from vsrd_amd.rendering import renderers
    sc = scene(N, R)
    inst = fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev)
    block = fields.FieldBlock(inst, 0.4, sc["mlp"].to(dev) if how == "residual_step" else None, None)
    origins, directions = sc["origins"].to(dev), sc["directions"].to(dev)
    if how == "render_hierarchical":
        out = rendering.render_hierarchical(block, origins, directions, (0.0, 100.0), S, 0.4, 0.4, seed=SEED, stream_offset=STEP, return_uniforms=True)
        return out["u_coarse"], out["u_fine"]
    renderers.STEP_WAVE_PER_RAY = how == "step_wave_per_ray"
    try:
        with torch.no_grad():
            samples = rendering.silhouette_step(block, origins, directions, sc["targets"].to(dev), (0.0, 100.0), S, 0.4, 0.4, seed=SEED,
                                                stream_offset=STEP, return_samples=True, skip_exact_misses=False)[-1]
    finally:
        renderers.STEP_WAVE_PER_RAY = False
    return samples["u_coarse"], samples["u_fine"]


def check_uniforms(tag, u_coarse, u_fine, R, S):
    coarse, fine = reference_uniforms(R, S)
    assert u_coarse.shape == (R, S) and u_fine.shape == (R, S)
    assert torch.equal(u_coarse.cpu(), coarse), f"{tag}: u_coarse differs from uniform(x) of philox(ray, sample, offset; seed)"
    got = u_fine.cpu()
    error = float((got.double() - fine).abs().max())
    print(f"[{tag}] worst |u_fine - float64| {error:.3e} = {error * 2 ** 24 / S:.3f} x S x 2^-24")
    assert margin(tag, "fine uniform abs error", error, FINE_UNIFORM_ATOL) <= FINE_UNIFORM_ATOL
    assert bool((got[:, 1:] >= got[:, :-1]).all()) and float(got.max()) < 1.0 and float(got.min()) >= 0.0


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
@pytest.mark.parametrize("how", ["render_hierarchical", "step_wave_per_ray", "step_multi_ray"])
def test_render_uniforms_match_the_philox_streams(dev, how, S):
    """The uniforms a launch exports are those of the stream keyed (ray, sample, stream_offset; seed): u_coarse == uniform(x) exactly;
    u_fine == min(cumsum(e)[s] / (sum(e) + e_extra), 0.99999994) with e = -log1p(-uniform(y)) over the ray's S samples and e_extra from
    z of sample 0, to the rounding of the float32 evaluation; every row non-decreasing and below 1.  N = 4, R = 1, 5, 37 rays (a lone
    ray, a partial group of the four- and two-ray mappings, more rays than a workgroup has waves), S on both sides of 16, 64 and at 128:
    render_hierarchical_kernel, the fused step with one ray per wave, and with four (S <= 64) or two rays per wave.
    Measured on the MI355X over all cases of this module: worst absolute error of a fine uniform 2.002e-07 (3.4 x 2^-24, at S = 17;
    0.2 x S x 2^-24 there and less at every larger S), asserted at 9e-7."""
    for R in RAY_COUNTS:
        u_coarse, u_fine = exported_uniforms(dev, how, 4, S, R)
        check_uniforms(f"test_render_uniforms_match_the_philox_streams[{how}-{S}]", u_coarse, u_fine, R, S)


def test_render_uniforms_of_the_two_rays_per_wave_kernel(dev):
    """N = 33, S = 128: more instances than the four-ray mapping takes, so the default mapping is two rays per wave, 32 lanes each."""
    for R in RAY_COUNTS:
        u_coarse, u_fine = exported_uniforms(dev, "step_multi_ray", 33, 128, R)
        check_uniforms("test_render_uniforms_of_the_two_rays_per_wave_kernel", u_coarse, u_fine, R, 128)


def step_on_both_uniforms(dev, N, S, R, residual):
    """One fused step twice -- with in-kernel Philox keyed (SEED, STEP), then on the host reference's uniforms of the same key (u_coarse
    exact, u_fine rounded to float32, sorted) -> ((loss, labels), (loss, labels)) on the host."""
    from vsrd_amd import fields, rendering
    sc = scene(N, R)
    coarse, fine = reference_uniforms(R, S)
    results = []
    for uniforms in ({}, dict(u_coarse=coarse.to(dev), u_fine=fine.float().to(dev))):
        block = fields.FieldBlock(fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev), 0.4, sc["mlp"].to(dev) if residual else None, None)
        with torch.no_grad():
            loss, labels = rendering.silhouette_step(block, sc["origins"].to(dev), sc["directions"].to(dev), sc["targets"].to(dev), (0.0, 100.0), S,
                                                     0.4, 0.4, seed=SEED, stream_offset=STEP, return_labels=True, skip_exact_misses=False, **uniforms)
        results.append((loss.cpu(), labels.cpu()))
    return results


def check_same_step(tag, results):
    """The project's bound for two evaluations of a step on the same Philox stream: labels 2e-4 (test_split_step_matches_wave_per_ray),
    loss 1e-3."""
    (loss_a, labels_a), (loss_b, labels_b) = results
    assert float(labels_b.max()) > 0.05                                       # the scene is seen
    assert margin(tag, "labels", (labels_a - labels_b).abs().max(), 2e-4) < 2e-4
    torch.testing.assert_close(loss_a, loss_b, rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("N,S,R", [(8, 100, 130), (4, 64, 37)])
def test_split_ray_step_draws_the_reference_uniforms(dev, N, S, R):
    """The split-ray mapping (VSRD_FLAG_STEP_SPLIT_RAY; four and two rounds) exports no samples, so its stream is pinned through its
    results: the step with in-kernel Philox against the same step on the host reference's uniforms."""
    from vsrd_amd.rendering import renderers
    renderers.STEP_SPLIT_RAY = True
    try:
        results = step_on_both_uniforms(dev, N, S, R, residual=False)
    finally:
        renderers.STEP_SPLIT_RAY = False
    check_same_step(f"test_split_ray_step_draws_the_reference_uniforms[{N}-{S}-{R}]", results)


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_residual_step_draws_the_reference_uniforms(dev, S):
    """The residual step writes its samples out for 32 < S <= 64 only (csrc/launch.h: residual_step_front_kernel<2, true>); there the
    exported uniforms are held to the host reference like every other kernel's, and any other S is refused, not served by another
    kernel.  At every S the step's own kernels (one round per pass, the ray split over a pair of waves at two and four rounds) are pinned
    through their results: in-kernel Philox against the host reference's uniforms supplied."""
    from vsrd_amd import _lib
    for R in RAY_COUNTS:
        if 32 < S <= 64:
            u_coarse, u_fine = exported_uniforms(dev, "residual_step", 4, S, R)
            check_uniforms(f"test_residual_step_draws_the_reference_uniforms[{S}]", u_coarse, u_fine, R, S)
        else:
            with pytest.raises(_lib.VsrdHipError, match="unsupported configuration"):
                exported_uniforms(dev, "residual_step", 4, S, R)
    check_same_step(f"test_residual_step_draws_the_reference_uniforms[{S}]", step_on_both_uniforms(dev, 4, S, 37, residual=True))
