"""The yardstick of the patch-correlation tests (tests/patch_correlation_reference.py) pinned by known answers: cases whose result follows
from the definition alone, so that a slip in the restatement cannot hide behind the device tests that are measured against it."""
import math

import pytest
import torch

import patch_correlation_reference as pcr


def _same_camera(scene, V):
    """Every view gets the target's camera: the homography is the identity for any plane."""
    scene["K"] = scene["K"][:1].expand(V, 3, 3).contiguous()
    scene["E"] = torch.eye(4).repeat(V, 1, 1)
    return scene


def _run(scene, patch_size=(11, 11), top_k=4):
    return pcr.reference(scene["images"], scene["K"], scene["E"], scene["pixels"], scene["positions"], scene["normals"], scene["converged"],
                         patch_size, top_k)


def test_equal_patches_have_coefficient_one():
    V, R = 5, 6
    scene = _same_camera(pcr.scene(11, V, R, 48, 96), V)
    scene["images"] = scene["images"][:1].expand(V, 3, 48, 96).contiguous()
    out = _run(scene, (5, 5))
    variance = out["patches"][0].var(dim=-1, unbiased=True)                       # [R]
    expected = variance / torch.sqrt(variance * variance + 1e-12)
    assert torch.allclose(out["coefficients"], expected[:, None, None].expand(R, V, V), rtol=0, atol=1e-12)
    assert 0.0 <= out["loss"].item() < 1e-9                                       # textured: variance ~ 1e-2, 1 - v / sqrt(v^2 + 1e-12) ~ 5e-9


def test_negated_images_cancel():
    V, R = 4, 5
    scene = _same_camera(pcr.scene(12, V, R, 48, 96), V)
    image = scene["images"][0]
    scene["images"] = torch.stack([image, 1.0 - image, image, 1.0 - image])
    out = _run(scene, (5, 5), top_k=4)
    c = out["coefficients"][:, 0, 0]                                              # every row is {c, c, -c, -c}
    signs = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=torch.float64)
    assert torch.allclose(out["coefficients"], c[:, None, None] * signs[:, None] * signs[None, :], rtol=0, atol=1e-9)
    assert abs(out["loss"].item() - 0.5) < 1e-12


def test_constant_view_has_zero_row_and_column():
    V, R = 5, 6
    scene = _same_camera(pcr.scene(13, V, R, 48, 96), V)
    scene["images"][2] = 0.25
    out = _run(scene, (5, 5))
    assert not torch.isnan(out["coefficients"]).any() and not torch.isnan(out["loss"])
    # (the interpolation weights sum to 1 up to rounding: the sampled patch is constant to 1e-16, its coefficients 0 to 1e-12 / sqrt(1e-12))
    assert (out["coefficients"][:, 2, :].abs() < 1e-12).all() and (out["coefficients"][:, :, 2].abs() < 1e-12).all()
    assert (out["coefficients"][:, 0, 0] > 0.999).all()
    scene["images"][2] = 0.0                                                      # ... and exactly 0 for a patch that is constant exactly
    out = _run(scene, (5, 5))
    assert not torch.isnan(out["coefficients"]).any() and not torch.isnan(out["loss"])
    assert (out["coefficients"][:, 2, :] == 0).all() and (out["coefficients"][:, :, 2] == 0).all()
    assert (out["coefficients"][:, 0, 0] > 0.999).all()


def test_nan_pixel_ranks_first_and_is_dropped_by_the_mean():
    V, R, k, bad_view, bad_ray = 6, 4, 4, 3, 1
    scene = _same_camera(pcr.scene(14, V, R, 48, 96), V)
    scene["pixels"] = torch.stack([20 + 10 * torch.arange(R), torch.full((R,), 24)], dim=-1)     # patches of different rays do not overlap
    x, y = scene["pixels"][bad_ray].tolist()
    scene["images"][bad_view, :, y, x] = float("nan")                            # (the centre samples at about (x - 0.2, y + 0.01): a tap on it)
    out = _run(scene, (5, 5), k)
    coefficients = out["coefficients"]
    assert torch.isnan(coefficients[bad_ray, bad_view, :]).all() and torch.isnan(coefficients[bad_ray, :, bad_view]).all()
    others = torch.ones(R, V, V, dtype=torch.bool)
    others[bad_ray, bad_view, :] = False
    others[bad_ray, :, bad_view] = False
    assert not torch.isnan(coefficients[others]).any()
    assert (out["indices"][bad_ray, :, 0] == bad_view).all()                      # NaN is ranked first in every row of the ray
    kept = []                                                                     # by hand: NaNs take their slots, the mean skips them
    for ray in range(R):
        for row in coefficients[ray].tolist():
            numbers = sorted((value for value in row if not math.isnan(value)), reverse=True)
            kept += numbers[:max(k - (len(row) - len(numbers)), 0)]
    expected = (1.0 - sum(kept) / len(kept)) / 2.0
    assert abs(out["loss"].item() - expected) < 1e-12
    assert len(kept) == R * V * k - (k + (V - 1))                                 # the NaN row loses k slots, every other row of the ray one


@pytest.mark.parametrize("patch_size, xs, ys", [
    ((11, 11), list(range(-5, 6)), list(range(-5, 6))),
    ((3, 5), [-1, 0, 1], [-2, -1, 0, 1, 2]),
    ((4, 2), [-2, -1, 0, 1], [-1, 0]),
])
def test_patch_grid(patch_size, xs, ys):
    grid = pcr.patch_grid(patch_size)
    assert grid.shape == (len(ys), len(xs), 2)
    flat = grid.flatten(0, 1).tolist()                                            # x is the fast index
    assert flat == [[float(x), float(y)] for y in ys for x in xs]


def test_identity_homography_still_interpolates():
    V, R, H, W = 2, 5, 48, 96
    scene = _same_camera(pcr.scene(15, V, R, H, W), V)
    out = _run(scene, (3, 3), top_k=2)
    q = scene["pixels"].double()[:, None, :] + pcr.patch_grid((3, 3)).flatten(0, 1)              # [R,P,2]
    size = torch.tensor([W, H], dtype=torch.float64)
    expected = q / (1.0 + 1e-6) * size / (size - 1.0) - 0.5                        # h_z = 1: s = q / (1 + 1e-6), then s W / (W - 1) - 0.5
    assert torch.allclose(out["coordinates"][1], expected, rtol=0, atol=1e-9)
    assert ((expected - expected.round()).abs() > 1e-3).any()                     # not on the pixel centres
    gray = (scene["images"][1].double() * torch.tensor(pcr.GRAY_WEIGHTS, dtype=torch.float64).view(3, 1, 1)).sum(dim=0)
    for ray in range(R):                                                          # the centre pixel's value, by hand
        px, py = expected[ray, 4].tolist()
        x0, y0 = math.floor(px), math.floor(py)
        fx, fy = px - x0, py - y0
        value = ((1 - fy) * ((1 - fx) * gray[y0, x0] + fx * gray[y0, x0 + 1]) + fy * ((1 - fx) * gray[y0 + 1, x0] + fx * gray[y0 + 1, x0 + 1])).item()
        assert abs(out["patches"][1, ray, 4].item() - value) < 1e-12


def test_gray_before_or_after_interpolation_agree():
    """The device op's stated deviation: it samples gray planes where the reference samples colours and turns the samples gray.  Both maps
    are linear, so in float64 the two orders agree to rounding -- zero padding included."""
    V, R, H, W = 5, 12, 48, 96
    scene = pcr.scene(16, V, R, H, W, patch_size=(5, 5))
    scene["E"][4, 0, 3] = 12.0                                                    # a view whose patches straddle the border
    coordinates = pcr.source_coordinates(scene["K"].double(), scene["E"].double(), 0, scene["pixels"], scene["positions"].double(),
                                         scene["normals"].double(), (5, 5))
    after = pcr.sample_patches(scene["images"].double(), coordinates)
    before = pcr.sample_patches(scene["images"].double(), coordinates, gray_first=True)
    assert (after != 0).any() and (after[4] == 0).any()
    assert (after - before).abs().max().item() < 1e-12
