"""Pins the CPU oracle (oracle/) against golden vectors produced by the reference's own
modules (tests/golden/make_golden.py).  CPU only; no HIP involved."""
import numpy as np
import pytest
import torch

from conftest import load_golden, RENDER_CASES, RESIDUAL_CASES
from oracle import fields, rendering, geometry, losses


def union_from(g, dtype=torch.float32, requires_grad=False):
    loc = g["locations"].to(dtype).clone().requires_grad_(requires_grad)
    dim = g["dimensions"].to(dtype).clone().requires_grad_(requires_grad)
    rot = g["orientations"].to(dtype).clone().requires_grad_(requires_grad)
    mlp = None
    if "mlp_weights" in g:
        mlp = g["mlp_weights"].to(dtype).clone().requires_grad_(requires_grad)
    temperature = float(g["temperature"]) if "temperature" in g else 1.0
    return fields.InstanceUnion(loc, rot, dim, temperature, mlp)


def test_g1_ray_casting():
    g = load_golden("g1_ray_casting")
    for tag in ("small", "mid"):
        h, w = (int(v) for v in g[f"{tag}_hw"])
        cam, dirs = geometry.ray_casting((h, w), g[f"{tag}_K"], g[f"{tag}_E"])
        torch.testing.assert_close(cam, g[f"{tag}_camera_positions"], rtol=0, atol=1e-6)
        torch.testing.assert_close(dirs, g[f"{tag}_ray_directions"], rtol=0, atol=1e-6)


def test_g2_box_known_answers():
    g = load_golden("g2_g3_sdf_union")
    d, _ = fields.box_distance_and_gradient(g["known_points"], g["known_dim"])
    torch.testing.assert_close(d, g["known_distances"][:, 0], rtol=0, atol=1e-6)
    # SURVEY.md §4 values
    np.testing.assert_allclose(d.numpy(), [-0.999, -0.499, 1.0, 2.236068, 0.001, 0.500001], atol=2e-6)


def test_g2_instance_distances_and_normals():
    g = load_golden("g2_g3_sdf_union")
    union = union_from(g)
    d, gw = union.instance_terms(g["points"])
    torch.testing.assert_close(d, g["instance_distances"][..., 0], rtol=1e-6, atol=2e-6)
    torch.testing.assert_close(gw, g["instance_gradients"], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("temperature,tag", [(1.0, "T1"), (0.1, "T0p1")])
def test_g3_soft_union(temperature, tag):
    g = load_golden("g2_g3_sdf_union")
    union = union_from(g)
    union.temperature = temperature
    u, w, grad = union.evaluate(g["points"])
    torch.testing.assert_close(u, g[f"union_{tag}_distances"][..., 0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(w, g[f"union_{tag}_labels"], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(grad, g[f"union_{tag}_gradients"], rtol=1e-4, atol=2e-5)


def test_g5_samplers():
    g = load_golden("g5_samplers")
    q = rendering.stratified_distances((0.0, 4.0), 4, torch.full((1, 4), 0.5))
    torch.testing.assert_close(q[0], g["quadrature"], rtol=0, atol=0)
    bins = g["it_bins"][None]
    s = rendering.importance_distances(bins, torch.tensor([[0.0, 1.0, 1.0]]), torch.linspace(0, 1, 5)[None])
    torch.testing.assert_close(s[0], g["it_samples_011"], rtol=0, atol=1e-6)
    s = rendering.importance_distances(bins, torch.zeros(1, 3), torch.linspace(0, 1, 3)[None])
    torch.testing.assert_close(s[0], g["it_samples_000"], rtol=1e-6, atol=0)
    u = torch.sort(g["rand_uniforms"][:, 0], dim=-1).values
    s = rendering.importance_distances(g["rand_bins"][:, 0], g["rand_weights"][:, 0], u)
    torch.testing.assert_close(s, g["rand_samples"][:, 0], rtol=1e-6, atol=1e-5)


def test_g6_encoder_and_mlp():
    g = load_golden("g6_encoder_mlp")
    known = fields.sinusoidal_features(torch.tensor([0.1, 0.2, 0.3]))
    torch.testing.assert_close(known, g["encoder_known"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(known[:6].numpy(), [0.95106, 0.30902, 0.80902, 0.58779, 0.30902, 0.95106], atol=1e-5)
    assert tuple(int(v) for v in g["num_neurons"]) == fields.MLP_SPLITS
    x = g["positions"]
    eye = torch.eye(3).expand(*x.shape[:-1], 3, 3)
    feats, dfeats = fields.sinusoidal_features(x, eye)
    torch.testing.assert_close(feats, g["encoded"], rtol=0, atol=1e-6)
    out, dout = fields.instance_mlp(g["weights"][:, None, :], feats, dfeats)
    torch.testing.assert_close(out, g["outputs"][..., 0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dout, g["input_gradients"], rtol=1e-3, atol=2e-3)
    # the closed-form tangent in float64 against autograd in float64 (derivation check)
    x64 = x.double().requires_grad_(True)
    w64 = g["weights"].double()[:, None, :]
    f64, df64 = fields.sinusoidal_features(x64, torch.eye(3, dtype=torch.float64).expand(*x.shape[:-1], 3, 3))
    o64, do64 = fields.instance_mlp(w64, f64, df64)
    auto, = torch.autograd.grad(o64.sum(), x64)
    torch.testing.assert_close(do64, auto, rtol=1e-9, atol=1e-9)


def test_g7_projection():
    g = load_golden("g7_g8_projection_boxes")
    boxes = g["boxes_3d"].clone().requires_grad_(True)
    out = geometry.project_boxes(boxes, g["K"])
    torch.testing.assert_close(out, g["boxes_2d"], rtol=1e-5, atol=1e-3)
    assert torch.all(out[5] == 0)                      # fully behind the camera
    assert out[4].abs().max() > 1e6                    # straddles z = 0
    grad, = torch.autograd.grad(out[:5].clamp(-1e4, 1e4).sum(), boxes)
    torch.testing.assert_close(grad, g["grad_boxes_3d"], rtol=1e-4, atol=1e-3)
    idx = torch.tensor(geometry.BOX_EDGES)
    clipped, masks = geometry.clip_edges_to_front(g["boxes_3d"][:, idx, :])
    torch.testing.assert_close(clipped, g["clipped_lines"], rtol=1e-6, atol=1e-6)
    assert torch.equal(masks, g["clip_masks"])
    from vsrd_amd import operations                                       # the package's own (host/torch) clip_lines_to_front
    clipped, masks = operations.clip_lines_to_front(g["boxes_3d"][:, idx, :])
    torch.testing.assert_close(clipped, g["clipped_lines"], rtol=1e-6, atol=1e-6)
    assert torch.equal(masks, g["clip_masks"])
    # zero-parameter box projects to these pixels
    loc, dim, rot, corners = geometry.decode_box_parameters(torch.zeros(1, 3), torch.zeros(1, 3), torch.tensor([[1.0, 0.0]]))
    np.testing.assert_allclose(loc.numpy(), [[0.0, 0.675, 50.0]], atol=1e-6)
    np.testing.assert_allclose(dim.numpy(), [[0.875, 0.875, 2.0]], atol=1e-6)
    torch.testing.assert_close(geometry.project_boxes(corners, g["K"])[0], g["zero_box_2d"], rtol=1e-6, atol=1e-4)
    np.testing.assert_allclose(g["zero_box_2d"].numpy(), [[671.9769, 236.4672], [692.1221, 256.6125]], atol=1e-3)


def test_g8_box_parameters():
    g = load_golden("g7_g8_projection_boxes")
    loc, dim, rot, corners = geometry.decode_box_parameters(g["raw_locations"], g["raw_dimensions"], g["raw_orientations"])
    torch.testing.assert_close(loc, g["locations"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dim, g["dimensions"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(rot, g["orientations"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(corners, g["decoded_boxes_3d"], rtol=1e-6, atol=1e-5)
    eloc, edim, erot = geometry.encode_box_corners(g["decoded_boxes_3d"])
    torch.testing.assert_close(eloc, g["encoded_locations"], rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(edim, g["encoded_dimensions"], rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(erot, g["encoded_orientations"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(eloc, loc, rtol=1e-5, atol=1e-4)   # round trip
    torch.testing.assert_close(edim, dim, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(geometry.rotation_matrix_x(torch.tensor([0.0, 0.3, -1.2])), g["rotation_matrix_x"])
    torch.testing.assert_close(geometry.expand_to_4x4(torch.arange(18.0).reshape(2, 3, 3)), g["expand_to_4x4"])


def _check_render_case(name, tol_labels, tol_grad):
    g = load_golden(name)
    S = int(g["num_samples"])
    union = union_from(g, requires_grad=True)
    std, ratio = float(g["sdf_std_deviation"]), float(g["cosine_ratio"])
    coarse, fine = rendering.hierarchical_render(
        union, g["origins"], g["directions"], (0.0, 100.0), S, std, ratio,
        g["u_coarse"], g["u_fine"], return_coarse=True)
    # pass 1
    assert torch.equal(coarse.distances, g["coarse_distances"].t())
    torch.testing.assert_close(coarse.weights, g["coarse_weights"].t(), rtol=1e-4, atol=2e-6)
    torch.testing.assert_close(coarse.labels, g["coarse_labels"], rtol=1e-4, atol=tol_labels)
    # pass 2: sampled distances (importance sampler), then everything downstream
    miss = g["coarse_weights"].sum(0) == 0
    # (the sampler divides by (delta-cdf + 1e-6): fp32 rounding of the coarse weights is amplified
    #  to ~1e-3 of a bin width where delta-cdf is small, hence the looser absolute tolerance)
    torch.testing.assert_close(fine.distances[~miss], g["fine_distances"].t()[~miss], rtol=1e-4, atol=5e-3)
    torch.testing.assert_close(fine.distances[miss], g["fine_distances"].t()[miss], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(fine.labels, g["fine_labels"], rtol=1e-4, atol=tol_labels)
    torch.testing.assert_close(fine.weights, g["fine_weights"].t(), rtol=1e-3, atol=tol_labels)
    # (field gradients at samples the ill-conditioned division above displaced by ~1e-3 m differ visibly where instances overlap:
    #  every gradient at a sample that did NOT move must agree tightly; only the displaced ones -- a few percent of the samples --
    #  get the loose bound, and at most 0.1 % of all entries may need it)
    got_g, want_g = fine.gradients[~miss], g["fine_gradients"].transpose(0, 1)[~miss]
    got_d, want_d = fine.distances[~miss], g["fine_distances"].t()[~miss]
    moved = (got_d - want_d).abs() > 1e-5 + 1e-6 * want_d.abs()                                          # samples the sampler displaced
    moved = (moved[:, :-1] | moved[:, 1:]).unsqueeze(-1).expand_as(got_g)                                # (gradients live at the midpoints)
    error = (got_g - want_g).abs().detach()
    tight = error <= 1e-4 + 1e-3 * want_g.abs()
    # (a sample that stayed may still sit an ulp or two from the golden's -- the sampler's last bit differs between CPUs -- and next to an
    #  edge of a box the field gradient changes that fast: such a sample passes when the field, evaluated at the golden's own positions, is tight)
    nudged = got_d != want_d
    nudged = (nudged[:, :-1] | nudged[:, 1:]).unsqueeze(-1).expand_as(got_g)
    at_golden = rendering.render_given_distances(union, g["origins"], g["directions"], g["fine_distances"].t(), std, ratio).gradients[~miss]
    tight_at_golden = (at_golden - want_g).abs().detach() <= 1e-4 + 1e-3 * want_g.abs()
    stayed_tight = tight | (nudged & tight_at_golden)
    assert bool(stayed_tight[~moved].all()), (int((~stayed_tight & ~moved).sum()), float(error[~moved].max()))   # every sample that stayed: tight
    assert moved.float().mean() <= 5e-2 and (~tight).float().mean() <= 1e-3 and float(error.max()) < 5e-3, \
        (float(moved.float().mean()), int((~tight).sum()), float(error.max()))
    # losses and parameter gradients
    bce = losses.silhouette_loss(fine.labels, g["targets"])
    eik = losses.eikonal_loss(fine.gradients)
    torch.testing.assert_close(bce, g["bce"], rtol=1e-5, atol=1e-6)
    # Rays whose coarse weights are all zero get their fine samples extrapolated to ~1e6 m
    # (SURVEY.md §8a-6); there |x| ~ 1e6 makes (d_i - u)/T pure fp32 rounding noise, so the
    # reference's own gradient norms are not reproducible.  Eikonal parity is asserted on the
    # well-conditioned rays; the full-tensor value only has to agree in magnitude.
    eik_conditioned = losses.eikonal_loss(fine.gradients[~miss])
    torch.testing.assert_close(eik_conditioned, g["eikonal_conditioned"], rtol=1e-3, atol=1e-6)
    assert 0.3 < float(eik) / max(float(g["eikonal"]), 1e-12) < 3.0
    loss = bce + float(g["eikonal_weight"]) * eik_conditioned
    params = [union.locations, union.dimensions, union.orientations]
    names = ["grad_locations", "grad_dimensions", "grad_orientations"]
    if union.mlp_weights is not None:
        params.append(union.mlp_weights)
        names.append("grad_mlp_weights")
    grads = torch.autograd.grad(loss, params)
    for got, key in zip(grads, names):
        scale = float(g[key].abs().max())
        torch.testing.assert_close(got, g[key], rtol=tol_grad, atol=tol_grad * max(scale, 1e-3))
    return fine


@pytest.mark.parametrize("name", RENDER_CASES)
def test_g4_hierarchical_rendering(name):
    _check_render_case(name, tol_labels=2e-5, tol_grad=2e-3)


@pytest.mark.parametrize("name", RESIDUAL_CASES)
def test_g10_residual_rendering(name):
    _check_render_case(name, tol_labels=5e-5, tol_grad=5e-3)


def test_g9_union_at_traced_surface():
    g = load_golden("g9_sphere_tracing")
    union = union_from(g)
    conv = g["convergence_masks"][:, 0]
    u, _, grad = union.evaluate(g["surface_positions"])
    assert torch.all(u[conv].abs() < 0.0101)
    n = torch.nn.functional.normalize(grad, dim=-1)
    torch.testing.assert_close(n[conv], g["surface_normals"][conv], rtol=1e-4, atol=1e-4)


def test_diou_hand_cases():
    """torchvision ops are absent here: hand-computed DIoU cases (PARITY UNPINNED, see oracle/geometry.py)."""
    a = torch.tensor([[0.0, 0.0, 2.0, 2.0]])
    b = torch.tensor([[1.0, 1.0, 3.0, 3.0]])
    # IoU = 1/7, centre distance^2 = 2, enclosing diagonal^2 = 18
    expected = 1.0 / 7.0 - 2.0 / 18.0
    np.testing.assert_allclose(geometry.distance_box_iou(a, b).item(), expected, rtol=1e-6)
    np.testing.assert_allclose(geometry.distance_box_iou_loss(a, b).item(), 1.0 - expected, rtol=1e-6)
    np.testing.assert_allclose(geometry.distance_box_iou(a, a).item(), 1.0, rtol=1e-6)
    c = torch.tensor([[5.0, 0.0, 6.0, 1.0]])   # disjoint: IoU 0, centres (1,1)-(5.5,.5), diag^2 = 36+4
    np.testing.assert_allclose(geometry.distance_box_iou(a, c).item(), -(4.5 ** 2 + 0.5 ** 2) / 40.0, rtol=1e-6)
    clipped = geometry.clip_boxes_to_image(torch.tensor([[[-5.0, 3.0], [2000.0, 500.0]]]), (376, 1408))
    assert clipped.tolist() == [[[0.0, 3.0], [1408.0, 376.0]]]


def test_g11_soft_rasterizer():
    g = load_golden("g11_soft_rasterizer")
    H, W = (int(v) for v in g["hw"])
    for k in range(3):
        d = geometry.polygon_distance_map(g[f"polygon_{k}"], (H, W))
        torch.testing.assert_close(d, g[f"distance_{k}"], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(geometry.soft_mask(d, g[f"inside_{k}"], float(g["temperature"])), g[f"soft_{k}"], rtol=1e-5, atol=1e-5)


def test_g14_box_3d_iou():
    """vsrd.operations.box_3d_iou (evaluation metric, scripts/main.py:888-905): the oracle restatement and the package's host-side
    function against the reference's outputs, quirks included (clockwise footprints, + 0.01 in the clip)."""
    from vsrd_amd import operations
    g = load_golden("g14_box_3d_iou")
    for a, b, want_3d, want_bev in zip(g["corners1"], g["corners2"], g["iou_3d"], g["iou_bev"]):
        for function in (geometry.box_3d_iou, operations.box_3d_iou):
            got_3d, got_bev = function(a, b)
            assert abs(float(got_3d) - float(want_3d)) < 1e-5 and abs(float(got_bev) - float(want_bev)) < 1e-5, function.__module__
    # a pair the reference's corner order does not break: counter-clockwise footprints, plain geometry
    square = torch.tensor([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=torch.float32)[[3, 2, 1, 0]]
    top, bottom = torch.cat([square, torch.ones(4, 1)], 1), torch.cat([square, torch.zeros(4, 1)], 1)
    box = torch.cat([top, bottom])
    shifted = box + torch.tensor([0.5, 0.0, 0.0])
    for function in (geometry.box_3d_iou, operations.box_3d_iou):
        iou_3d, iou_bev = function(box, shifted)
        assert abs(float(iou_bev) - 1.0 / 3.0) < 2e-2 and abs(float(iou_3d) - 1.0 / 3.0) < 2e-2       # the + 0.01 moves the crossings a little


def test_g15_hypernetwork_state_dict_and_forward():
    """a12: the package's HyperDistanceField loads the reference's state dict (same parameter names: weight_g / weight_v of the
    weight-normed linears, LayerNorm affine) and reproduces its per-instance MLP weights and embedding gradients."""
    from vsrd_amd import models
    g = load_golden("g15_hypernetwork")
    state = {k[len("state__"):].replace("__", "."): v for k, v in g.items() if k.startswith("state__")}
    module = models.HyperDistanceField(48, [16, 16, 16, 16], 12, [10, 14])
    assert set(module.state_dict()) == set(state)
    module.load_state_dict(state)
    embeddings = g["embeddings"].clone().requires_grad_(True)
    weights = module(embeddings)
    assert weights.shape == (1, 3, 1617) and module.num_neurons_list == [784, 272, 272, 272, 17]
    torch.testing.assert_close(weights, g["weights"], rtol=1e-5, atol=1e-6)
    grad, = torch.autograd.grad((weights * g["probe"]).sum(), embeddings)
    torch.testing.assert_close(grad, g["grad_embeddings"], rtol=1e-4, atol=1e-6)


def test_g6_package_distance_field_method():
    """a11: HyperDistanceField.distance_field(weights, positions) (hyper_distance_field.py:57-73) -- the method scripts/main.py:541
    binds with functools.partial -- and SinusoidalEncoder, against the reference's outputs and input gradients (G6)."""
    import functools
    from vsrd_amd import models
    g = load_golden("g6_encoder_mlp")
    module = models.HyperDistanceField(48, [16, 16, 16, 16], 256, [256, 256, 256, 256])
    encoder = models.SinusoidalEncoder(8)
    assert module.num_neurons_list == [int(v) for v in g["num_neurons"]]
    x = g["positions"].clone().requires_grad_(True)
    feats = encoder(x)
    torch.testing.assert_close(feats, g["encoded"], rtol=0, atol=1e-6)
    out = module.distance_field(g["weights"][:, None, :], feats)
    assert out.shape == g["outputs"].shape
    torch.testing.assert_close(out, g["outputs"], rtol=1e-4, atol=1e-5)
    grad, = torch.autograd.grad(out, x, torch.ones_like(out))
    torch.testing.assert_close(grad, g["input_gradients"], rtol=1e-3, atol=2e-3)
    bound = functools.partial(module.distance_field, g["weights"][0])          # main.py:541-544
    torch.testing.assert_close(bound(feats[0].detach()), g["outputs"][0], rtol=1e-4, atol=1e-5)


def test_g16_rendering_helpers():
    """sphere_intersection, phong_shading (visualisation helpers of vsrd.rendering) and sdfs.norm against the reference's outputs."""
    from vsrd_amd import rendering
    g = load_golden("g16_rendering_helpers")
    near, far, hit = rendering.sphere_intersection(g["positions"], g["directions"], 4.0)
    assert torch.equal(hit, g["hit"]) and int(hit.sum()) not in (0, hit.numel())
    torch.testing.assert_close(near[hit], g["near"][g["hit"]], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(far[hit], g["far"][g["hit"]], rtol=1e-6, atol=1e-6)
    colors = rendering.phong_shading(**{k[len("phong__"):]: v for k, v in g.items() if k.startswith("phong__")})
    torch.testing.assert_close(colors, g["colors"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(rendering.sdfs.norm(g["vectors"], dim=-1, keepdim=True), g["norms"], rtol=1e-7, atol=0)


def test_diou_terms_against_an_independent_box_iou():
    """torchvision 0.14 (distance_box_iou, distance_box_iou_loss: scripts/main.py:359-362, 375, 393) is not in the image, so the oracle's DIoU has
    no reference output to be pinned by ("DIoU unpinned").  What CAN be cross-checked here: `transformers` ships DETR's
    box_iou / generalized_box_iou, themselves taken from torchvision.ops.boxes -- an independent implementation of two of the three terms.  On
    random boxes (overlapping, disjoint, nested, touching):  oracle DIoU + rho^2 / c^2  ==  transformers' IoU,  and the enclosing box whose
    squared diagonal c^2 the oracle divides by has the area that generalized_box_iou's  IoU - (area_c - union) / area_c  implies.  The centre
    distance rho^2 is the one term left to the hand cases above (test_diou_hand_cases)."""
    import pytest
    loss_module = pytest.importorskip("transformers.loss.loss_for_object_detection")
    from oracle import geometry
    g = torch.Generator().manual_seed(0)
    lo = torch.rand(64, 2, generator=g, dtype=torch.float64) * 100.0
    a = torch.cat([lo, lo + torch.rand(64, 2, generator=g, dtype=torch.float64) * 60.0 + 1.0], -1)
    lo = torch.rand(48, 2, generator=g, dtype=torch.float64) * 100.0
    b = torch.cat([lo, lo + torch.rand(48, 2, generator=g, dtype=torch.float64) * 60.0 + 1.0], -1)
    b[0] = a[0]                                                        # identical
    b[1] = torch.tensor([a[1, 0] + 1.0, a[1, 1] + 1.0, a[1, 2] - 1.0, a[1, 3] - 1.0]) if float((a[1, 2:] - a[1, :2]).min()) > 3 else b[1]     # nested
    b[2] = torch.tensor([a[2, 2], a[2, 1], a[2, 2] + 10.0, a[2, 3]])  # touching along an edge
    b[3] = a[3] + 500.0                                                # far apart
    iou, union = loss_module.box_iou(a, b)
    x1, y1, x2, y2 = (c[:, None] for c in a.unbind(-1))
    x1g, y1g, x2g, y2g = (c[None, :] for c in b.unbind(-1))
    centre = ((x1 + x2) / 2 - (x1g + x2g) / 2) ** 2 + ((y1 + y2) / 2 - (y1g + y2g) / 2) ** 2
    width, height = torch.max(x2, x2g) - torch.min(x1, x1g), torch.max(y2, y2g) - torch.min(y1, y1g)
    diou = geometry.distance_box_iou(a, b)
    torch.testing.assert_close(diou + centre / (width ** 2 + height ** 2 + 1.0e-7), iou, rtol=1e-12, atol=1e-12)
    giou = loss_module.generalized_box_iou(a, b)
    torch.testing.assert_close(iou - (width * height - union) / (width * height), giou, rtol=1e-12, atol=1e-12)       # the same enclosing box
    assert float(diou[0, 0]) == pytest.approx(1.0, abs=1e-9) and float(diou[3, 3]) < -0.5
    # the element-wise loss form on matched pairs: 1 - DIoU of the pair (its IoU carries eps in the denominator: 1e-7 / union)
    pairs = min(a.shape[0], b.shape[0])
    loss = geometry.distance_box_iou_loss(a[:pairs], b[:pairs])
    torch.testing.assert_close(loss, 1.0 - torch.diagonal(diou)[:pairs], rtol=1e-7, atol=1e-7)
