"""The several-rays-per-wave step kernels (csrc/quad_step.h) with VSRD_FLAG_YAW_GRADIENTS: at the full shapes (S = 64 with 9..16 instances,
S = 128 with 33..64) the hot kernel has an instantiation with the flag compiled in, which the host picks by the flag; every other launch
tests it at run time.  Both must compute what one ray per wave computes.  And their importance merge (quad_importance_merge), which takes
the merge ranks from the inverse-CDF brackets where every fine sample of the wave's live rays stayed in its bracket and from two searches
otherwise: both must give the stable sorted union.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

from conftest import margin

pytestmark = pytest.mark.gpu

CONSTANT = [4, 6, 7, 8, 10]                  # r01, r10, r11, r12, r21 of the packed block: what rotation_matrix_y keeps constant
KEPT = [c for c in range(16) if c not in CONSTANT]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def scene(seed, N, R, S, general_rotations=False):
    """Boxes 8 to 30 m in front of a camera at the origin, rays aimed near them (the scenes of test_hip_render.py)."""
    g = torch.Generator().manual_seed(seed)
    loc = torch.stack([torch.empty(N).uniform_(-6, 6, generator=g), torch.empty(N).uniform_(-1.0, 1.5, generator=g),
                       torch.empty(N).uniform_(8, 30, generator=g)], -1)
    dim = torch.stack([torch.empty(N).uniform_(0.75, 1.0, generator=g), torch.empty(N).uniform_(0.75, 1.0, generator=g),
                       torch.empty(N).uniform_(1.5, 2.5, generator=g)], -1)
    if general_rotations:
        q, r = torch.linalg.qr(torch.randn(N, 3, 3, generator=g, dtype=torch.float64))
        q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2)
        q[:, :, 0] *= torch.sign(torch.linalg.det(q)).unsqueeze(-1)
        rot = q.float()
    else:
        yaw = torch.empty(N).uniform_(-3.1, 3.1, generator=g)
        rot = torch.stack([torch.stack([torch.cos(yaw), torch.zeros(N), torch.sin(yaw)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                           torch.stack([-torch.sin(yaw), torch.zeros(N), torch.cos(yaw)], -1)], -2)
    target = loc[torch.randint(0, N, (R,), generator=g)] + torch.randn(R, 3, generator=g) * 0.7
    return dict(loc=loc, dim=dim, rot=rot, origins=torch.zeros(R, 3), directions=torch.nn.functional.normalize(target, dim=-1),
                u_coarse=torch.rand(R, S, generator=g), u_fine=torch.rand(R, S, generator=g), targets=torch.rand(R, N, generator=g))


def run_step(dev, sc, S, mode, yaw_gradients, distance_range=(0.0, 100.0), T=0.4, std=0.4, ratio=0.4):
    """One fused step: `mode` = "rows" (what a dense launch takes by itself: four or two rays per wave), "wave" (one ray per wave) or
    "general" (rows, every rotation treated as a general one).  Returns (loss, labels, gradient of the packed block)."""
    from vsrd_amd import fields, rendering
    from vsrd_amd.rendering import renderers
    renderers.STEP_WAVE_PER_RAY, renderers.GENERAL_ROTATIONS = mode == "wave", mode == "general"
    try:
        inst = fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev).requires_grad_(True)
        block = fields.FieldBlock(inst, T, None, None, yaw_gradients=yaw_gradients)
        loss, labels = rendering.silhouette_step(block, sc["origins"].to(dev), sc["directions"].to(dev), sc["targets"].to(dev), distance_range, S, std, ratio,
                                                 u_coarse=sc["u_coarse"].to(dev), u_fine=sc["u_fine"].to(dev), return_labels=True)
        return loss.detach().clone(), labels.clone(), torch.autograd.grad(loss, inst)[0].clone()
    finally:
        renderers.STEP_WAVE_PER_RAY = renderers.GENERAL_ROTATIONS = False


def check_against_one_ray_per_wave(tag, rows, wave, S, columns):
    """The tolerances of test_split_step_matches_wave_per_ray (scenes with explicit uniforms and no forced misses)."""
    assert torch.isfinite(rows[2]).all() and float(wave[1].max()) > 0.05                   # the scene is seen
    label_error = margin(tag, "labels vs one ray per wave", (rows[1] - wave[1]).abs().max(), 2e-5)
    gradient_tolerance = 1e-3 if S <= 20 else 2e-4
    gradient_error = margin(tag, "gradient vs one ray per wave", (rows[2][:, columns] - wave[2][:, columns]).abs().max() / max(float(wave[2].abs().max()), 1e-6),
                            gradient_tolerance)
    print(f"{tag}: loss {float(rows[0]):.9g} vs {float(wave[0]):.9g}, labels {label_error:.3e}, gradient {gradient_error:.3e}")
    assert label_error < 2e-5
    torch.testing.assert_close(rows[0], wave[0], rtol=1e-5, atol=1e-7)
    assert gradient_error <= gradient_tolerance


# full-shape four-ray kernel (also: groups with dead rows), run-time S with padding lanes in both quad round counts, full-shape two-ray kernel
SHAPES = [(16, 64, 203), (16, 64, 6), (16, 64, 7), (3, 33, 61), (3, 20, 61), (33, 128, 37)]


@pytest.mark.parametrize("N,S,R", SHAPES)
def test_step_with_yaw_gradients_matches_one_ray_per_wave(dev, N, S, R):
    """Rotations about y with VSRD_FLAG_YAW_GRADIENTS -- at S = 64 / 128 the hot kernels that have the flag compiled in, at the other shapes
    the run-time test -- against one ray per wave: loss, labels and the gradient entries the flag keeps; the entries it drops are exact
    zeros; a second launch repeats the first bit for bit.  (The far plane is 100 m and the boxes end at 30 m: the last pass-2 rounds of
    these rays see nothing, so the label mix of the last round with a weight re-evaluates its soft-min terms or reads them from the wave's
    distance cache, whichever round that cache still holds.)"""
    sc = scene(300 + N + S, N, R, S)
    rows = run_step(dev, sc, S, "rows", True)
    again = run_step(dev, sc, S, "rows", True)
    wave = run_step(dev, sc, S, "wave", True)
    assert all(torch.equal(a, b) for a, b in zip(rows, again))
    assert float(rows[2][:, CONSTANT].abs().max()) == 0.0 and float(rows[2][:, KEPT].abs().max()) > 0
    check_against_one_ray_per_wave(f"test_step_with_yaw_gradients_matches_one_ray_per_wave[{N}-{S}-{R}]", rows, wave, S, KEPT)


def test_full_shape_step_without_the_yaw_flag_takes_the_run_time_path(dev):
    """yaw_gradients=False on the full shape: the hot kernel WITHOUT the compiled-in flag, which accumulates all nine rotation adjoints.
    Its gradient agrees with the general-rotation kernels' to 1e-4 of the largest entry, the five entries included, and with the flag's
    kernel bit for bit on the entries that one keeps."""
    N, S, R = 16, 64, 203
    sc = scene(300 + N + S, N, R, S)
    plain = run_step(dev, sc, S, "rows", False)
    again = run_step(dev, sc, S, "rows", False)
    general = run_step(dev, sc, S, "general", False)
    flagged = run_step(dev, sc, S, "rows", True)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert float(plain[2][:, CONSTANT].abs().max()) > 0
    error = margin("test_full_shape_step_without_the_yaw_flag_takes_the_run_time_path", "gradient vs general rotations",
                   (plain[2] - general[2]).abs().max() / max(float(general[2].abs().max()), 1e-6), 1e-4)
    print(f"gradient vs general rotations {error:.3e}, labels {float((plain[1] - general[1]).abs().max()):.3e}")
    assert error <= 1e-4 and (plain[1] - general[1]).abs().max() < 1e-4
    assert torch.equal(plain[0], flagged[0]) and torch.equal(plain[1], flagged[1]) and torch.equal(plain[2][:, KEPT], flagged[2][:, KEPT])


# ---- the importance merge (quad_importance_merge): ranks from the inverse-CDF brackets, the two searches where a bracket does not hold --------------
MERGE_SHAPES = [(16, 64, 64), (16, 64, 6), (16, 64, 7), (3, 33, 30), (3, 20, 30), (33, 128, 14)]
MERGE_CASES = ["ordinary", "cdf_entries", "one_bin"]


def step_samples(dev, sc, S, directions, u_fine, std, running_minimum=False):
    """The fused step's own sorted pass-2 distances [R, 2S] and coarse weights [R, S - 1] (dense launch: four or two rays per wave)."""
    from vsrd_amd import fields, rendering
    from vsrd_amd.rendering import renderers
    renderers.RUNNING_MINIMUM = running_minimum
    try:
        inst = fields.pack_instances(sc["loc"], sc["rot"], sc["dim"]).to(dev)
        out = rendering.silhouette_step(fields.FieldBlock(inst, 0.4, None, None), sc["origins"].to(dev), directions.to(dev), sc["targets"].to(dev), (0.0, 100.0), S, std,
                                        0.4, u_coarse=sc["u_coarse"].to(dev), u_fine=u_fine.to(dev), skip_exact_misses=False, return_samples=True)
        return out[-1]["distances"].cpu(), out[-1]["coarse_weights"].cpu()
    finally:
        renderers.RUNNING_MINIMUM = False


def merge_inputs(dev, sc, S, case):
    """(sorted fine uniforms, sigma) of a case.  cdf_entries: each ray's fine uniforms are the entries of its own coarse cdf as float32 sums on the
    host (most of them equal to the device's entries, the others an ulp away: either side of a bracket's end).  one_bin: a sharp surface
    (sigma = 0.03: the coarse weight sits in one or two bins, the cdf is flat elsewhere) and ONE uniform repeated S times."""
    if case == "ordinary":
        return torch.sort(sc["u_fine"], dim=-1).values, 0.4
    if case == "one_bin":
        return sc["u_fine"][:, :1].expand(-1, S).contiguous(), 0.03
    _, weights = step_samples(dev, sc, S, sc["directions"], torch.sort(sc["u_fine"], dim=-1).values, 0.4)
    weights = weights.abs()
    cdf = torch.cumsum(weights / weights.sum(-1, keepdim=True).clamp_min(1e-12), dim=-1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], dim=-1).clamp(0.0, 0.99999994)
    return torch.sort(cdf, dim=-1).values, 0.4


def host_coarse(u_coarse, S, near=0.0, far=100.0):
    """The stratified coarse distances in float64 (the device rounds them to float32 its own way: matched to the nearest entry below)."""
    edges = torch.linspace(near, far, S + 1, dtype=torch.float64)
    return edges[:-1] + (edges[1:] - edges[:-1]) * u_coarse.double()


@pytest.mark.parametrize("case", MERGE_CASES)
@pytest.mark.parametrize("N,S,R", MERGE_SHAPES)
def test_merged_distances_are_the_stable_union(dev, N, S, R, case):
    """The sorted pass-2 distances of every ray equal, bit for bit, the stable merge (a coarse distance before an equal fine one) of the device's
    own coarse distances -- the S entries nearest the host's float64 values, each within 1e-5 m -- and its own fine distances -- the other S.
    A wrong rank leaves a slot of the row unwritten or writes one twice, so the row is no longer sorted or loses a coarse distance."""
    sc = scene(500 + N + S, N, R, S)
    u_fine, std = merge_inputs(dev, sc, S, case)
    merged, _ = step_samples(dev, sc, S, sc["directions"], u_fine, std)
    again, _ = step_samples(dev, sc, S, sc["directions"], u_fine, std)
    assert torch.equal(merged, again) and torch.isfinite(merged).all()
    want = host_coarse(sc["u_coarse"], S)
    for ray in range(R):
        row = merged[ray].numpy()
        position = np.searchsorted(row.astype(np.float64), want[ray].numpy())
        lower, upper = np.clip(position - 1, 0, 2 * S - 1), np.clip(position, 0, 2 * S - 1)
        nearest = np.where(np.abs(row[lower] - want[ray].numpy()) <= np.abs(row[upper] - want[ray].numpy()), lower, upper)
        assert len(set(nearest.tolist())) == S and np.abs(row[nearest] - want[ray].numpy()).max() < 1e-5, ray
        is_coarse = np.zeros(2 * S, dtype=bool)
        is_coarse[nearest] = True
        coarse, fine = row[is_coarse], row[~is_coarse]
        keys = np.concatenate([coarse, fine])
        order = np.lexsort((np.concatenate([np.zeros(S), np.ones(S)]), keys))          # by value, coarse before fine on equal values
        assert np.array_equal(keys[order].view(np.uint32), row.view(np.uint32)), ray
        assert np.all(np.diff(fine) >= 0)


@pytest.mark.parametrize("case", MERGE_CASES)
@pytest.mark.parametrize("N,S,R", MERGE_SHAPES)
def test_bracket_ranks_equal_search_ranks(dev, N, S, R, case):
    """The same rays merged by both paths of one library.  The second launch turns the last ray of every wave's group (four rays at N <= 16 and
    S <= 64, else two) away from the scene: a ray of (next to) no weight, whose fine samples are extrapolated far beyond their bracket, so its vote
    sends the whole group to the two searches.  (Running minimum in both launches, so that both run the same body of the same kernel.)  The
    other rays' sorted distances must be bit-equal in the two launches."""
    sc = scene(500 + N + S, N, R, S)
    u_fine, std = merge_inputs(dev, sc, S, case)
    rays_per_group = 4 if (N <= 16 and S <= 64) else 2
    away = torch.zeros(R, dtype=torch.bool)
    away[rays_per_group - 1::rays_per_group] = True
    directions = sc["directions"].clone()
    directions[away] = torch.nn.functional.normalize(torch.tensor([[0.3, -0.9, -0.4]]), dim=-1)
    bracketed, _ = step_samples(dev, sc, S, sc["directions"], u_fine, std, running_minimum=True)
    searched, weights = step_samples(dev, sc, S, directions, u_fine, std, running_minimum=True)
    assert float(weights[away].abs().max()) < 1e-3 and float(searched[away].max()) > 1.0e4           # (next to) no weight, extrapolated
    assert torch.isfinite(searched).all() and (searched[away].diff(dim=-1) >= 0).all()
    assert torch.equal(bracketed[~away], searched[~away])
