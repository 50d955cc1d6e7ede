"""oracle.tracing against the reference's own sphere_tracing outputs (G9, and G19: rays that graze a rim), on the CPU.

G19 holds, per field (soft union at T = 0.3 and 0.05, hard union), 1000 rays of a 96 x 320 image of three boxes: every ray on which a march
that stops for good at the first convergence differs from the reference, and an even subsample of the rest.  The hard union has such rays
too (25 of them), so the conditions below hold for all three fields."""
import functools

import pytest
import torch

from conftest import load_golden
from oracle import fields as ofields, tracing as otracing

POSITION_TOL = dict(rtol=1.0e-5, atol=2.0e-3)       # G9's, tests/test_hip_render.py
APART = 1.0                                          # metres: two surfaces, not two roundings of one
FIELDS = ("T0.3", "T0.05", "hard")


def grazing_field(g, k, dtype):
    """Field k of G19 -> callable positions [R,3] -> distances [R] in `dtype`."""
    loc, dim, rot = (g[key].to(dtype) for key in ("locations", "dimensions", "orientations"))
    hard = k == len(g["temperatures"])
    union = ofields.InstanceUnion(loc, rot, dim, 1.0 if hard else float(g["temperatures"][k]))
    return functools.partial(union.union_distance, hard=hard)


@functools.lru_cache(maxsize=None)
def grazing_trace(k, dtype, early_exit=False, retired=False):
    g = load_golden("g19_sphere_tracing_grazing")
    iterations, criteria, radius = int(g["trace"][0]), float(g["trace"][1]), float(g["trace"][2])
    out = otracing.trace(grazing_field(g, k, dtype), torch.zeros(3, dtype=dtype), g["directions"][k].to(dtype), iterations, criteria,
                         bounding_radius=radius, initialise=False, early_exit=early_exit, stop_at_first_convergence=retired)
    return out, otracing.borderline(out, criteria, radius)


def test_fixture_is_what_its_generator_promises():
    g = load_golden("g19_sphere_tracing_grazing")
    assert g["directions"].shape == (3, 1000, 3) and g["directions"].dtype == torch.float32
    assert g["surface_positions"].shape == (3, 1000, 3) and g["convergence_masks"].shape == (3, 1000) and g["discriminating"].shape == (3, 1000)
    assert g["directions"].shape[1] % 64 != 0
    torch.testing.assert_close(g["directions"].norm(dim=-1), torch.ones(3, 1000))
    for k in range(3):
        assert 32 <= int(g["convergence_masks"][k].sum()) <= 1000 - 32


@pytest.mark.parametrize("k", range(3), ids=FIELDS)
def test_float32_oracle_reproduces_g19(k):
    g = load_golden("g19_sphere_tracing_grazing")
    for early_exit in (True, False):
        out, borderline = grazing_trace(k, torch.float32, early_exit=early_exit)
        keep = ~borderline
        print(f"{FIELDS[k]} early_exit={early_exit}: {out.iterations} iterations, {out.live_iterations.double().mean():.2f} live per ray, "
              f"{int(borderline.sum())} borderline, {int((out.converged != g['convergence_masks'][k]).sum())} masks differ")
        assert torch.equal(out.converged[keep], g["convergence_masks"][k][keep])
        hit = keep & g["convergence_masks"][k]          # as G9's test: a ray still in flight after the last iteration has no surface position
        torch.testing.assert_close(out.positions[hit], g["surface_positions"][k][hit], **POSITION_TOL)


@pytest.mark.parametrize("k", range(3), ids=FIELDS)
def test_fixture_conditions(k):
    g = load_golden("g19_sphere_tracing_grazing")
    wide, borderline = grazing_trace(k, torch.float32, early_exit=False)
    literal, _ = grazing_trace(k, torch.float32, early_exit=True)
    assert torch.equal(wide.positions, literal.positions) and torch.equal(wide.converged, literal.converged)       # the batch-wide exit changes nothing
    borderline64 = grazing_trace(k, torch.float64)[1]
    either = borderline | borderline64
    assert int(either.sum()) <= 0.01 * len(either)
    discriminating = g["discriminating"][k]
    print(f"{FIELDS[k]}: {int(discriminating.sum())} discriminating, {int((discriminating & ~either).sum())} of them not borderline, {int(either.sum())} borderline")
    assert int((discriminating & ~either).sum()) >= 16
    if k == 0:          # T = 0.3: converged at the rim of the front box under one rule, on the box behind under the other
        retired, _ = grazing_trace(k, torch.float32, retired=True)
        both = discriminating & retired.converged & g["convergence_masks"][k]
        apart = (retired.positions - g["surface_positions"][k]).norm(dim=-1)
        print(f"converged under both rules and apart: {apart[both].tolist()}")
        assert bool((apart[both] > APART).any())


@pytest.mark.parametrize("k", range(3), ids=FIELDS)
def test_the_retired_rule_fails_on_the_discriminating_rays(k):
    g = load_golden("g19_sphere_tracing_grazing")
    retired, _ = grazing_trace(k, torch.float32, retired=True)
    differs = (retired.converged != g["convergence_masks"][k]) | ((retired.positions - g["surface_positions"][k]).norm(dim=-1) > APART)
    assert torch.equal(differs, g["discriminating"][k])
    assert int(differs.sum()) >= 16
    # ... and in float64 as well, off the borderline set: the difference is the rule, not the rounding
    retired64, borderline64 = grazing_trace(k, torch.float64, retired=True)
    differs64 = (retired64.converged != g["convergence_masks"][k]) | ((retired64.positions.float() - g["surface_positions"][k]).norm(dim=-1) > APART)
    keep = ~borderline64 & ~grazing_trace(k, torch.float64)[1]
    assert int((differs64 & g["discriminating"][k] & keep).sum()) >= 16


@pytest.mark.parametrize("k", range(3), ids=FIELDS)
def test_float64_and_float32_oracle_masks_agree_off_the_borderline_set(k):
    single, _ = grazing_trace(k, torch.float32)
    double, borderline = grazing_trace(k, torch.float64)
    keep = ~borderline
    assert torch.equal(single.converged[keep], double.converged[keep])
    both = keep & double.converged
    distance = (single.positions.double() - double.positions)[both].norm(dim=-1).max()
    print(f"{FIELDS[k]}: largest float32-to-float64 distance over {int(both.sum())} converged rays = {float(distance):.3e}")
    assert float(distance) < POSITION_TOL["atol"]


def test_float32_oracle_reproduces_g9():
    """200 iterations with the entry-point initialisation and one origin per ray; the reference's batch-wide exit fires here."""
    g = load_golden("g9_sphere_tracing")
    union = ofields.InstanceUnion(g["locations"], g["orientations"], g["dimensions"], float(g["temperature"]))
    want = g["convergence_masks"][:, 0]
    outs = [otracing.trace(union.distance, g["origins"], g["directions"], 200, 0.01, bounding_radius=100.0, early_exit=e) for e in (True, False)]
    assert outs[0].iterations < 200 and outs[0].iterations <= outs[1].iterations
    assert torch.equal(outs[0].positions, outs[1].positions) and torch.equal(outs[0].converged, outs[1].converged)
    keep = ~otracing.borderline(outs[1], 0.01, 100.0)
    assert int((~keep).sum()) <= 0.01 * len(keep)
    assert torch.equal(outs[1].converged[keep], want[keep])
    torch.testing.assert_close(outs[1].positions[keep & want], g["surface_positions"][keep & want], **POSITION_TOL)
    double = otracing.trace(union_double(g).distance, g["origins"].double(), g["directions"].double(), 200, 0.01, bounding_radius=100.0, early_exit=False)
    keep = ~otracing.borderline(double, 0.01, 100.0)
    assert torch.equal(double.converged[keep], want[keep])


def union_double(g):
    return ofields.InstanceUnion(g["locations"].double(), g["orientations"].double(), g["dimensions"].double(), float(g["temperature"]))


def test_the_stationary_state_is_a_fixed_point():
    """What lets a per-ray march stop early: a ray that did not move and may not move sees the same distance again.  Marching on for more
    iterations changes nothing of a ray that was stationary, and live_iterations counts up to that state."""
    g = load_golden("g19_sphere_tracing_grazing")
    field = grazing_field(g, 0, torch.float32)
    short = otracing.trace(field, torch.zeros(3), g["directions"][0], 64, 0.01, bounding_radius=100.0, initialise=False, early_exit=False)
    longer = otracing.trace(field, torch.zeros(3), g["directions"][0], 80, 0.01, bounding_radius=100.0, initialise=False, early_exit=False)
    settled = short.live_iterations < 64
    assert int(settled.sum()) > 900
    assert torch.equal(short.positions[settled], longer.positions[settled]) and torch.equal(short.converged[settled], longer.converged[settled])
    assert torch.equal(short.live_iterations[settled], longer.live_iterations[settled])


def test_options_of_the_oracle():
    """foreground, initialise, zero iterations: the corners the GPU cases lean on."""
    g = load_golden("g19_sphere_tracing_grazing")
    field = grazing_field(g, 0, torch.float64)
    d = g["directions"][0][:8].double()
    out = otracing.trace(field, torch.zeros(3, dtype=torch.float64), d, 0, 0.01, bounding_radius=100.0)
    assert not out.converged.any() and torch.allclose(out.positions, -100.0 * d)           # an origin inside the sphere: the entry point lies behind it
    origin = torch.tensor([0.0, 0.0, -150.0], dtype=torch.float64)
    out = otracing.trace(field, origin, d, 0, 0.01, bounding_radius=100.0)
    assert torch.allclose(out.positions.norm(dim=-1), torch.full((8,), 100.0, dtype=torch.float64)) and (out.positions[:, 2] < 0).all()
    masked = otracing.trace(field, origin, d, 8, 0.01, foreground=torch.zeros(8, dtype=torch.bool), bounding_radius=100.0, initialise=False)
    assert torch.equal(masked.positions, origin.expand(8, 3)) and not masked.converged.any() and (masked.live_iterations == 1).all()
    nan = otracing.trace(field, torch.full((3,), float("nan"), dtype=torch.float64), d, 8, 0.01, bounding_radius=100.0)
    assert torch.isnan(nan.positions).all() and not nan.converged.any() and not nan.foreground.any()
