"""vsrd_sphere_trace (csrc/aux_kernels.h) on the GPU against oracle.tracing in float64 -- the reference's loop without its batch-wide exit --
and, on G19 (rays that graze a rim), against the reference's own output.

Every comparison follows one rule (`compare`): masks are equal on every ray that is not borderline (a decision along the float64 path within
1e-4 relative of its threshold; at most 1 % of a case), and the positions of the rays converged in both -- and of the rays that never were
foreground, which keep their origin or entry point -- are within 3 x the largest distance between the float32 and the float64 oracle on those
rays, with a floor of 4 float32 ulps of the largest coordinate under that distance.  What a ray that is still in flight after the last
iteration holds is not compared: no test of the reference's looks at it either.

Measured (MI355X; the oracle-to-oracle distance, the bound and what the device showed, in metres) are in DESIGN.md, "Sphere tracing"."""
import ctypes
import functools
import operator

import numpy as np
import pytest
import torch

from conftest import load_golden, margin
from oracle import fields as ofields, tracing as otracing

pytestmark = pytest.mark.gpu

T = 0.3
TRACE = (64, 0.01, 100.0)          # iterations, convergence criterion, bounding radius
R_SMALL = 257
SENTINEL = 0xA5
FIELDS = ("T0.3", "T0.05", "hard")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def pointer(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boxes(N=3):
    """G19's three boxes (N <= 3), or N boxes of the same sizes spread over 30 x 2 x 52 m in front of the camera."""
    g = load_golden("g19_sphere_tracing_grazing")
    if N <= 3:
        return g["locations"][:N].clone(), g["orientations"][:N].clone(), g["dimensions"][:N].clone()
    gen = torch.Generator().manual_seed(64)
    loc = torch.stack([torch.empty(N).uniform_(-15.0, 15.0, generator=gen), torch.empty(N).uniform_(-1.0, 1.0, generator=gen),
                       torch.empty(N).uniform_(8.0, 60.0, generator=gen)], -1)
    dim = g["dimensions"][torch.arange(N) % 3] * torch.empty(N, 1).uniform_(0.8, 1.2, generator=gen)
    yaw = torch.empty(N).uniform_(-3.1, 3.1, generator=gen)
    rot = torch.stack([torch.stack([torch.cos(yaw), torch.zeros(N), torch.sin(yaw)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                       torch.stack([-torch.sin(yaw), torch.zeros(N), torch.cos(yaw)], -1)], -2)
    return loc, rot, dim


@functools.lru_cache(maxsize=None)
def small_rays(N=3, origin=(0.0, 0.0, 0.0), R=R_SMALL):
    """Unit directions from `origin`: two in three aimed at points around the boxes (hits, grazes, near misses), the others over a wide fan."""
    loc, _, _ = boxes(N)
    gen = torch.Generator().manual_seed(7)
    aimed = loc[torch.randint(0, loc.shape[0], (R,), generator=gen)] + torch.randn(R, 3, generator=gen) * 0.9
    fan = torch.stack([torch.empty(R).uniform_(-25.0, 25.0, generator=gen), torch.empty(R).uniform_(-8.0, 8.0, generator=gen), torch.full((R,), 20.0)], -1)
    target = torch.where((torch.arange(R) % 3 < 2)[:, None], aimed, fan)
    return torch.nn.functional.normalize(target - torch.tensor(origin), dim=-1)


def oracle_field(N, dtype, temperature=T, hard=False, mlp=None):
    loc, rot, dim = (t.to(dtype) for t in boxes(N))
    union = ofields.InstanceUnion(loc, rot, dim, temperature, None if mlp is None else mlp.to(dtype))
    return functools.partial(union.union_distance, hard=hard)


def device_trace(dev, N, origins, directions, iterations=TRACE[0], criteria=TRACE[1], radius=TRACE[2], initialise=False, hard=False, foreground=None,
                 temperature=T, mlp=None, tail=0):
    """One vsrd_sphere_trace call -> positions [R + tail, 3] and converged [R + tail] on the host, the tails sentinel-filled before the call.
    origins [3] (stride 0) or [R,3]."""
    from vsrd_amd import _lib, fields
    lib = _lib.load()
    loc, rot, dim = boxes(N)
    instances = fields.pack_instances(loc, rot, dim).to(dev)
    weights = None if mlp is None else mlp.to(dev).contiguous()
    field = _lib.Field(N, temperature, instances.data_ptr(), None if weights is None else weights.data_ptr())
    R = directions.shape[0]
    o, d = origins.to(dev).contiguous(), directions.to(dev).contiguous()
    fg = None if foreground is None else foreground.to(torch.uint8).to(dev).contiguous()
    positions = torch.full(((R + tail) * 12,), SENTINEL, dtype=torch.uint8, device=dev).view(torch.float32).view(R + tail, 3)
    converged = torch.full((R + tail,), SENTINEL, dtype=torch.uint8, device=dev)
    _lib.check(lib.vsrd_sphere_trace(field, pointer(o), 0 if o.dim() == 1 else 3, pointer(d), pointer(fg), R, iterations, criteria, float(radius or 0.0),
                                     1 if initialise else 0, 1 if hard else 0, pointer(positions), pointer(converged), _lib.stream()))
    torch.cuda.synchronize()
    return positions.cpu(), converged.cpu()


def oracles(N, origins, directions, iterations=TRACE[0], criteria=TRACE[1], radius=TRACE[2], initialise=False, hard=False, foreground=None,
            temperature=T, mlp=None):
    """(float64 oracle, float32 oracle, borderline from the float64 one), all without the batch-wide exit."""
    outs = []
    for dtype in (torch.float64, torch.float32):
        outs.append(otracing.trace(oracle_field(N, dtype, temperature, hard, mlp), origins.to(dtype), directions.to(dtype), iterations, criteria,
                                   foreground=foreground, bounding_radius=radius, initialise=initialise, early_exit=False))
    return outs[0], outs[1], otracing.borderline(outs[0], criteria, radius)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def compare(name, positions, converged, double, single, borderline, also=None, least_converged=32, least_missing=32):
    """The rule of the module docstring; `also`: rays whose positions are compared although they did not converge (they never moved, or
    moved once).  Returns (oracle-to-oracle distance, bound, observed)."""
    R = len(borderline)
    got = converged.bool()
    assert set(converged.tolist()) <= {0, 1}
    keep = ~borderline
    assert int(borderline.sum()) <= 0.01 * R, f"{name}: {int(borderline.sum())} borderline rays of {R}"
    assert int(double.converged.sum()) >= least_converged and int((~double.converged).sum()) >= least_missing
    wrong = (got != double.converged) & keep
    assert not wrong.any(), f"{name}: masks differ on rays {torch.nonzero(wrong)[:, 0].tolist()}"
    both = keep & got & double.converged
    held = (both if also is None else both | (also & keep)) & torch.isfinite(double.positions).all(-1)
    scale = float(double.positions[held].abs().max()) if held.any() else 1.0
    floor = 4.0 * float(np.spacing(np.float32(scale)))
    settled = held & (single.converged == double.converged)
    reference_error = float((single.positions.double() - double.positions)[settled].norm(dim=-1).max()) if settled.any() else 0.0
    bound = 3.0 * max(reference_error, floor)
    observed = float((positions.double() - double.positions)[held].norm(dim=-1).max()) if held.any() else 0.0
    print(f"{name}: {int(double.converged.sum())} of {R} converged, {int(borderline.sum())} borderline, {double.live_iterations.double().mean():.2f} iterations per ray; "
          f"float32-to-float64 oracle {reference_error:.3e} m, floor {floor:.3e}, bound {bound:.3e}, device {observed:.3e}")
    margin(name, "|position - float64| m", observed, bound)
    assert observed <= bound, f"{name}: {observed:.3e} m from the float64 oracle, bound {bound:.3e}"
    return reference_error, bound, observed


# ---- G19 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3), ids=FIELDS)
def test_g19_grazing_rays_through_the_drop_in(dev, k):
    """rendering.sphere_tracing as main.py:1028-1041 drives it (compose(field, itemgetter(0)), a [3] camera position, initialization=False)
    on the rays that un-converge.  With the rule the kernels had before (stop for good at the first convergence) this case fails on the
    discriminating rays: tests/test_sphere_trace_reference.py shows on the CPU that such a march differs from the reference on exactly
    those rays, and one run of the previous library on the device gave 28 / 25 / 25 rays with a different mask for the three fields."""
    from vsrd_amd import rendering, fields, utils
    g = load_golden("g19_sphere_tracing_grazing")
    hard = k == len(g["temperatures"])
    temperature = 1.0 if hard else float(g["temperatures"][k])
    loc, dim, rot = (g[key].to(dev) for key in ("locations", "dimensions", "orientations"))
    members = [rendering.sdfs.translation(rendering.sdfs.rotation(fields.instance_field(rendering.sdfs.box(dim[i]), i, 3), rot[i]), loc[i]) for i in range(3)]
    field = fields.hard_union(members) if hard else utils.compose(fields.soft_union(members, temperature), operator.itemgetter(0))
    directions = g["directions"][k]
    iterations, criteria, radius = int(g["trace"][0]), float(g["trace"][1]), float(g["trace"][2])
    pos, conv = rendering.sphere_tracing(field, torch.zeros(3, device=dev), directions.to(dev), iterations, criteria, bounding_radius=radius, initialization=False)
    assert pos.shape == (1000, 3) and conv.shape == (1000, 1) and conv.dtype == torch.bool
    pos, conv = pos.cpu(), conv.cpu()[:, 0]
    double, single, borderline = oracles(3, torch.zeros(3), directions, iterations, criteria, radius, hard=hard, temperature=temperature)
    _, bound, _ = compare(f"g19-{FIELDS[k]}", pos, conv.to(torch.uint8), double, single, borderline)
    # ... and the reference's own output
    want, keep, flagged = g["convergence_masks"][k], ~borderline, g["discriminating"][k]
    assert torch.equal(conv[keep], want[keep])
    assert int((flagged & keep).sum()) >= 16 and torch.equal(conv[flagged & keep], want[flagged & keep])
    hit = keep & want
    distance = float((pos - g["surface_positions"][k])[hit].norm(dim=-1).max())
    print(f"g19-{FIELDS[k]}: largest distance from the reference's positions over {int(hit.sum())} converged rays = {distance:.3e} m")
    torch.testing.assert_close(pos[hit], g["surface_positions"][k][hit], rtol=1.0e-5, atol=2.0e-3)           # G9's tolerance
    if k == 0:          # T = 0.3 has discriminating rays that converge in the reference: on the box behind, not at the rim
        assert int((hit & flagged).sum()) >= 8 and float((pos - g["surface_positions"][k])[hit & flagged].norm(dim=-1).max()) < 1.0


# ---- options -----------------------------------------------------------------------------------------------------------------------------------
def residual_weights():
    return load_golden("g10_render_residual_n3_s16")["mlp_weights"][:2].float().contiguous()


OPTION_CASES = {
    "soft": dict(N=3),
    "hard": dict(N=3, hard=True),
    "residual": dict(N=2, mlp=True),
    "n64": dict(N=64),
    "no-radius": dict(N=3, radius=None),
    "one-iteration": dict(N=3, iterations=1, least_converged=0),
    "no-iteration": dict(N=3, iterations=0, least_converged=0),
}


@pytest.mark.parametrize("case", list(OPTION_CASES))
def test_options_against_the_float64_oracle(dev, case):
    """257 rays (four full waves and a lane; two workgroups) from a shared origin; also: the shared origin (stride 0) and the expanded [R,3]
    origins give the same bits, and so do two launches."""
    options = dict(OPTION_CASES[case])
    N = options.pop("N")
    least = dict(least_converged=options.pop("least_converged", 32))
    if options.pop("mlp", False):
        options["mlp"] = residual_weights()
    origin, directions = torch.zeros(3), small_rays(N)
    double, single, borderline = oracles(N, origin, directions, **options)
    positions, converged = device_trace(dev, N, origin, directions, **options)
    few = options.get("iterations", TRACE[0]) <= 1          # nothing is in flight yet: every position is compared
    compare(case, positions, converged, double, single, borderline, also=torch.ones(R_SMALL, dtype=torch.bool) if few else None, **least)
    if options.get("iterations", TRACE[0]) == 0:
        assert not converged.any() and same_bits(positions, origin.expand(R_SMALL, 3))
    again = device_trace(dev, N, origin, directions, **options)
    expanded = device_trace(dev, N, origin.expand(R_SMALL, 3).contiguous(), directions, **options)
    for other in (again, expanded):
        assert same_bits(positions, other[0]) and torch.equal(converged, other[1])


def test_initialisation_from_outside_and_inside_the_sphere_with_directions_of_any_length(dev):
    """initialise = 1 with per-ray origins: 150 m behind the camera, outside the sphere (rays through it and rays past it), and the camera
    itself, inside (the entry point then lies BEHIND the origin, as in the reference); direction lengths 0.5, 1 and 2 in turn."""
    R = R_SMALL
    outside, inside = torch.tensor([0.0, 0.0, -150.0]), torch.zeros(3)
    from_outside = torch.arange(R) % 2 == 0
    directions = torch.where(from_outside[:, None], small_rays(3, origin=(0.0, 0.0, -150.0)), small_rays(3))
    past = from_outside & (torch.arange(R) % 8 == 0)                                   # these miss the sphere by a wide margin
    directions = torch.where(past[:, None], torch.nn.functional.normalize(directions + torch.tensor([0.0, 1.5, 0.0]), dim=-1), directions)
    length = (torch.arange(R) // 2) % 3
    directions = directions * torch.tensor([0.5, 1.0, 2.0])[length][:, None]
    origins = torch.where(from_outside[:, None], outside, inside).contiguous()
    entry, hit = otracing.sphere_entry(origins.double(), directions.double(), 100.0)
    assert int((~hit).sum()) >= 16 and int((hit & from_outside).sum()) >= 64 and torch.equal(~hit, past)
    a = (directions.double() ** 2).sum(-1)
    assert float(((directions.double() * origins.double()).sum(-1) ** 2 - a * ((origins.double() ** 2).sum(-1) - 1.0e4)).abs().min()) > 1.0     # no ray near tangency
    options = dict(iterations=200, initialise=True)
    double, single, borderline = oracles(3, origins, directions, **options)
    positions, converged = device_trace(dev, 3, origins, directions, **options)
    compare("initialise", positions, converged, double, single, borderline, also=~hit)
    assert same_bits(positions[~hit], origins[~hit]) and not converged[~hit].any()        # a ray past the sphere keeps its origin
    # a step of twice the distance carries a ray through the box and out of its back, where the distance grows again: none of those converges
    # (in the reference neither); half steps and whole steps do
    assert int((double.converged & (length == 0)).sum()) >= 8 and int((double.converged & (length == 1)).sum()) >= 8
    assert not (double.converged & (length == 2)).any() and int((hit & (length == 2)).sum()) >= 32


def test_explicit_foreground_with_zeros(dev):
    """A zero-foreground ray never moves: it keeps its origin (or, with initialise, its entry point) and its flag is |sdf| < criteria there.
    Ray 5 starts within the criterion of a face (a traced surface point of the float64 oracle, |sdf| < criteria / 2): flag 1."""
    R = R_SMALL
    directions = small_rays(3)
    base = otracing.trace(oracle_field(3, torch.float64), torch.zeros(3, dtype=torch.float64), directions.double(), TRACE[0], TRACE[1],
                          bounding_radius=TRACE[2], initialise=False, early_exit=False)
    sdf = oracle_field(3, torch.float64)(base.positions).abs()
    donor = int(torch.nonzero(base.converged & (sdf < 0.5 * TRACE[1]))[0, 0])
    origins = torch.zeros(R, 3)
    origins[5] = base.positions[donor].float()
    foreground = torch.arange(R) % 4 != 1
    assert not foreground[5]
    for initialise in (False, True):
        options = dict(foreground=foreground, initialise=initialise)
        double, single, borderline = oracles(3, origins, directions, **options)
        positions, converged = device_trace(dev, 3, origins, directions, **options)
        compare(f"foreground-init{int(initialise)}", positions, converged, double, single, borderline, also=~foreground)
        assert not borderline[5] and double.converged[5] == (not initialise)
        if not initialise:
            assert same_bits(positions[~foreground], origins[~foreground]) and converged[5] == 1
            assert int(converged[~foreground].sum()) == 1


def test_non_finite_origins_without_a_foreground_array(dev):
    R = R_SMALL
    directions = small_rays(3)
    origins = torch.zeros(R, 3)
    origins[3, 1] = float("nan")
    origins[64] = float("inf")
    origins[130, 2] = float("-inf")
    origins[256] = float("nan")
    bad = ~torch.isfinite(origins).all(-1)
    for radius in (TRACE[2], None):
        double, single, borderline = oracles(3, origins, directions, radius=radius)
        positions, converged = device_trace(dev, 3, origins, directions, radius=radius)
        compare(f"non-finite-radius{radius}", positions, converged, double, single, borderline)
        assert not converged[bad].any()
        assert torch.equal(torch.isnan(positions[bad]), torch.isnan(origins[bad]))
        torch.testing.assert_close(positions[bad], origins[bad], rtol=0.0, atol=0.0, equal_nan=True)


# ---- independence of the launch ----------------------------------------------------------------------------------------------------------------
def test_a_ray_does_not_depend_on_its_launch(dev):
    """The first R rays of one set, R = 1, 63, 64, 65, 257, for a box-only and a residual field: every ray has the bits it has in the full launch,
    and the sentinel-filled tails of both outputs stay as they are."""
    for N, mlp in ((3, None), (2, residual_weights())):
        directions = small_rays(N)
        full_positions, full_converged = device_trace(dev, N, torch.zeros(3), directions, mlp=mlp)
        assert 32 <= int(full_converged.sum()) <= R_SMALL - 32
        for R in (1, 63, 64, 65, 257):
            positions, converged = device_trace(dev, N, torch.zeros(3), directions[:R], mlp=mlp, tail=7)
            assert same_bits(positions[:R], full_positions[:R]) and torch.equal(converged[:R], full_converged[:R]), (N, R)
            assert (positions[R:].contiguous().view(torch.uint8) == SENTINEL).all() and (converged[R:] == SENTINEL).all(), (N, R)


def test_grid_stride_loop_and_lane_tail_past_the_largest_grid(dev):
    """16384 x 256 + 321 rays -- more than the largest grid holds at once, with a tail of five waves and a lane: a 4096-ray pattern tiled,
    N = 1, 8 iterations, a shared origin.  Every tile has the bits of the 4096-ray launch."""
    from vsrd_amd import _lib, fields
    lib = _lib.load()
    P, R = 4096, 16384 * 256 + 321
    loc, rot, dim = boxes(1)
    instances = fields.pack_instances(loc, rot, dim).to(dev)
    field = _lib.Field(1, T, instances.data_ptr(), None)
    pattern = small_rays(1, R=P).to(dev)
    origin = torch.zeros(3, device=dev)

    def launch(directions):
        count = directions.shape[0]
        positions = torch.full((count + 1, 3), -7.0, device=dev)
        converged = torch.full((count + 1,), SENTINEL, dtype=torch.uint8, device=dev)
        _lib.check(lib.vsrd_sphere_trace(field, pointer(origin), 0, pointer(directions), None, count, 8, TRACE[1], TRACE[2], 0, 0, pointer(positions),
                                         pointer(converged), _lib.stream()))
        torch.cuda.synchronize()
        assert (positions[count] == -7.0).all() and converged[count] == SENTINEL
        return positions[:count], converged[:count]
    want_positions, want_converged = launch(pattern)
    assert 64 <= int(want_converged.sum()) <= P - 64
    tiles = R // P
    directions = torch.cat([pattern.repeat(tiles, 1), pattern[:R - tiles * P]])
    positions, converged = launch(directions)
    assert torch.equal(positions[:tiles * P].view(torch.int32).view(tiles, P, 3), want_positions.view(torch.int32).expand(tiles, P, 3))
    assert torch.equal(converged[:tiles * P].view(tiles, P), want_converged.expand(tiles, P))
    assert torch.equal(positions[tiles * P:].view(torch.int32), want_positions[:R - tiles * P].view(torch.int32))
    assert torch.equal(converged[tiles * P:], want_converged[:R - tiles * P])
