"""The patch-correlation photometric loss on the device (csrc/patch_correlation.h; include/vsrd_hip.h: vsrd_grayscale_images,
vsrd_patch_correlation_forward / _backward; losses.patch_correlation_loss) against tests/patch_correlation_reference.py, the float64
restatement of scripts/main.py:783-851 that tests/test_patch_correlation_reference.py pins by known answers.

Every launch through the C ABI runs on an arena whose buffers are separated by 256-byte guards filled with a sentinel (RowArena); the guards
and the inputs are compared byte for byte after every call.

The bounds.  SENSITIVITY_* is the yardstick's own sensitivity to rounding: its float32 run against its float64 run on the scenes of the
six cases below (computed on the CPU, x86-64, torch 2.x; the worst case and its scene are named beside the constant).  DEVICE_* is the
device's distance from the float64 yardstick on the same scenes, measured on an MI355X (gfx950).  Tests 1, 3 and 4 assert three times the
larger of the two; test 2 -- where only the summation order and float32 storage differ -- ten times the measured maximum.
"""
import numpy as np
import pytest
import torch

import patch_correlation_reference as pcr
from conftest import margin
from frame_rows import RowArena

pytestmark = pytest.mark.gpu

# (V, R, H, W, (pw, ph), k): the smallest shapes at which a distinct piece of the kernel can go wrong
CASES = [
    (4, 1, 24, 40, (3, 3), 4),            # k = V; P < 64; one ray
    (5, 16, 48, 96, (3, 5), 4),           # one coefficient dropped; rectangular patch; waves with no view
    (6, 16, 96, 320, (11, 11), 4),        # P = 121: a lane's second pixel with a tail
    (17, 100, 94, 352, (11, 11), 4),      # the reference's counts at a quarter of its image
    (32, 24, 48, 97, (4, 2), 4),          # the view limit; even sizes; W no multiple of 4
    (32, 3, 48, 96, (16, 16), 32),        # P and k at their limits; LDS at its largest
]
IDS = [f"V{V}-R{R}-{H}x{W}-{p[0]}x{p[1]}-k{k}" for V, R, H, W, p, k in CASES]
SEED_FORWARD, SEED_GRADIENT = 100, 200    # scene seed = base + index of the case

SENSITIVITY_PATCHES = 5.2e-5              # max |float32 - float64| yardstick patches, images in [0,1]: V17-R100-94x352-11x11 (seed 103), CPU
DEVICE_PATCHES = 4.6e-5                   # max |device - float64 yardstick|: V6-R16-96x320-11x11 (seed 102), MI355X
SENSITIVITY_LOSS = 8.4e-8                 # |float32 - float64| yardstick loss: V6-R16-96x320-11x11 (seed 102), CPU
DEVICE_LOSS = 2.9e-7                      # |device - float64 yardstick|: V4-R1-24x40-3x3 (seed 100: one ray, nine pixels), MI355X
SENSITIVITY_GRADIENT = 7.5e-5             # max |float32 - float64| autograd over the largest entry: normals of V32-R3-48x96-16x16 (seed 205), CPU
DEVICE_GRADIENT = 8.5e-5                  # max |device - float64 autograd| over the largest entry: normals of V32-R24-48x97-4x2 (seed 204), MI355X
MEASURED_COEFFICIENTS = 1.9e-7            # test 2, max |coefficient - float64 on the device's patches|: V32-R24-48x97-4x2 (seed 104), MI355X
MEASURED_STATS = 6.8e-8                   # test 2, |sum - float64| / count: the same case, MI355X
MEASURED_LINK_LOSS = 2.9e-8               # test 2, |loss - float64|: the same case, MI355X
BOUND_PATCHES = 3.0 * max(SENSITIVITY_PATCHES, DEVICE_PATCHES)
BOUND_LOSS = 3.0 * max(SENSITIVITY_LOSS, DEVICE_LOSS)
BOUND_GRADIENT = 3.0 * max(SENSITIVITY_GRADIENT, DEVICE_GRADIENT)
BOUND_COEFFICIENTS = 10.0 * MEASURED_COEFFICIENTS
BOUND_STATS = 10.0 * MEASURED_STATS
BOUND_LINK_LOSS = 10.0 * MEASURED_LINK_LOSS
MIN_GAP = 1e-4                            # rows (test 2) and rays (test 4) whose selection is decided by less are left out of the comparison
MAX_SHARE = 0.25                          # ... and may be no more than a quarter

SENTINEL_BITS = int(np.array(-777.0, dtype=np.float32).view(np.int32))
INPUTS = ("gray", "intrinsics", "extrinsics", "pixels", "positions", "normals", "converged", "grad_loss")
OUTPUTS = ("loss", "stats", "patches", "coefficients", "selected", "grad_positions", "grad_normals")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


# ---- the C ABI by hand ----------------------------------------------------------------------------------------------------------------
class Arena(RowArena):
    """One row with every buffer of a forward + backward call, a 256-byte guard in front of each and behind the last."""

    def __init__(self, V, R, H, W, P, workspace_bytes):
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        buffers = [("gray", (V, H, W), f32), ("intrinsics", (V, 3, 3), f32), ("extrinsics", (V, 4, 4), f32), ("pixels", (R, 2), i32),
                   ("positions", (R, 3), f32), ("normals", (R, 3), f32), ("converged", (R,), u8), ("grad_loss", (1,), f32),
                   ("workspace", (workspace_bytes,), u8), ("loss", (1,), f32), ("stats", (2,), f32), ("patches", (V, R, P), f32),
                   ("coefficients", (R, V, V), f32), ("selected", (R, V), i32), ("grad_positions", (R, 3), f32), ("grad_normals", (R, 3), f32)]
        fields = []
        for name, shape, dtype in buffers:
            fields += [("guard_" + name, (64,), i32), (name, shape, dtype)]
        super().__init__(fields, 1, SENTINEL_BITS, 256)
        self.guards = ["guard_" + name for name, _, _ in buffers]


def gray_planes(dev, images):
    from vsrd_amd import losses
    return losses.grayscale_images(images.to(dev)).cpu()


def launch(dev, s, patch_size, top_k, backward=True, upstream=1.0, export=True, gray=None):
    """Forward (and backward) through the C ABI on a guarded arena -> the outputs as host tensors."""
    from vsrd_amd import _lib
    lib = _lib.load()
    V, _, H, W = s["images"].shape
    R, P = s["pixels"].shape[0], patch_size[0] * patch_size[1]
    need = lib.vsrd_patch_correlation_workspace_bytes(V, R, P)
    assert need > 0
    arena = Arena(V, R, H, W, P, need)
    arena.view("gray").copy_(gray_planes(dev, s["images"]) if gray is None else gray)
    arena.view("intrinsics").copy_(s["K"]); arena.view("extrinsics").copy_(s["E"]); arena.view("pixels").copy_(s["pixels"].to(torch.int32))
    arena.view("positions").copy_(s["positions"]); arena.view("normals").copy_(s["normals"]); arena.view("converged").copy_(s["converged"].to(torch.uint8))
    arena.view("grad_loss").fill_(upstream)
    device = arena.host.to(dev)
    p = arena.pointers(device, () if export else ("patches", "coefficients", "selected"))
    config = _lib.PatchCorrelationConfig(V, R, H, W, patch_size[0], patch_size[1], top_k, 0, 1e-6, 1e-12)
    shared = [p(name) for name in ("gray", "intrinsics", "extrinsics", "pixels", "positions", "normals", "converged", "workspace")]
    _lib.check(lib.vsrd_patch_correlation_forward(config, *shared, need, p("loss"), p("stats"), p("patches"), p("coefficients"), p("selected"), _lib.stream()))
    if backward:
        _lib.check(lib.vsrd_patch_correlation_backward(config, *shared, need, p("stats"), p("grad_loss"), p("grad_positions"), p("grad_normals"), _lib.stream()))
    torch.cuda.synchronize()
    after = device.cpu()
    written = set(OUTPUTS) if backward else set(OUTPUTS[:5])
    if not export:
        written -= {"patches", "coefficients", "selected"}
    for name in arena.guards + list(INPUTS) + [name for name in OUTPUTS if name not in written]:
        assert torch.equal(arena.view(name).contiguous().view(torch.uint8), arena.view(name, 0, after).contiguous().view(torch.uint8)), name
    assert torch.equal(after[-256:], arena.host[-256:])
    return {name: arena.view(name, 0, after).clone() for name in written}


def yardstick(s, patch_size, top_k, dtype=torch.float64):
    return pcr.reference(s["images"], s["K"], s["E"], s["pixels"], s["positions"], s["normals"], s["converged"], patch_size, top_k, dtype=dtype)


_FORWARD, _GRADIENT = {}, {}


def forward_case(dev, index):
    """The noise scene of case `index`, its float64 yardstick and the device's forward, computed once and shared by tests 1-3."""
    if index not in _FORWARD:
        V, R, H, W, patch_size, k = CASES[index]
        s = pcr.scene(SEED_FORWARD + index, V, R, H, W, smooth=False, patch_size=patch_size)
        _FORWARD[index] = (s, yardstick(s, patch_size, k), launch(dev, s, patch_size, k, backward=False))
    return _FORWARD[index]


def gradient_case(index):
    """The smooth scene of case `index` with ill-conditioned rays re-drawn and every third ray unconverged, and its float64 gradients."""
    if index not in _GRADIENT:
        V, R, H, W, patch_size, k = CASES[index]
        s = pcr.scene(SEED_GRADIENT + index, V, R, H, W, smooth=True, patch_size=patch_size)
        share = pcr.redraw_rays(s, patch_size, k, MIN_GAP)
        if R >= 3:
            s["converged"] = torch.arange(R) % 3 != 1
        out = yardstick(s, patch_size, k)
        _GRADIENT[index] = (s, share, pcr.border_share(out["coordinates"]),
                            pcr.reference_gradients(s["images"], s["K"], s["E"], s["pixels"], s["positions"], s["normals"], s["converged"], patch_size, k))
    return _GRADIENT[index]


def relative(a, b):
    """max |a - b| over the largest entry of b."""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


# ---- 1-3: forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_patches_link(dev, index):
    s, ref, out = forward_case(dev, index)
    distance = (out["patches"].double() - ref["patches"]).abs().max().item()
    print(f"patches[{IDS[index]}]: device distance {distance:.3e}")
    margin(f"test_patches_link[{IDS[index]}]", "max |patch - float64|", distance, BOUND_PATCHES)
    assert distance <= BOUND_PATCHES


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_correlation_link(dev, index):
    """Steps 5-6 of the yardstick on the kernel's OWN patches against the kernel's coefficients, selection, stats and loss."""
    V, R, H, W, patch_size, k = CASES[index]
    s, _, out = forward_case(dev, index)
    loss, coefficients, indices = pcr.correlate(out["patches"].double(), s["converged"], k)
    error = (out["coefficients"].double() - coefficients).abs().max().item()
    top = torch.gather(coefficients, -1, indices)
    expected_sum, expected_count = torch.nansum(top).item(), (~torch.isnan(top)).sum().item()
    stats_error = abs(out["stats"][0].item() - expected_sum) / max(expected_count, 1)
    loss_error = abs(out["loss"].item() - loss.item())
    print(f"correlation[{IDS[index]}]: coefficients {error:.3e} stats/count {stats_error:.3e} loss {loss_error:.3e}")
    margin(f"test_correlation_link[{IDS[index]}]", "max |coefficient - float64|", error, BOUND_COEFFICIENTS)
    margin(f"test_correlation_link[{IDS[index]}]", "|sum - float64| / count", stats_error, BOUND_STATS)
    margin(f"test_correlation_link[{IDS[index]}]", "|loss - float64|", loss_error, BOUND_LINK_LOSS)
    decided = pcr.row_tie_gaps(coefficients, k) >= MIN_GAP
    skipped = 1.0 - decided.double().mean().item()
    margin(f"test_correlation_link[{IDS[index]}]", "rows skipped (tie gap)", skipped, MAX_SHARE)
    assert skipped <= MAX_SHARE
    assert torch.equal(out["selected"].to(torch.int64)[decided] & 0xffffffff, pcr.selection_mask(indices, V)[decided])
    assert out["stats"][1].item() == expected_count
    assert error <= BOUND_COEFFICIENTS and stats_error <= BOUND_STATS and loss_error <= BOUND_LINK_LOSS


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_end_to_end_loss(dev, index):
    s, ref, out = forward_case(dev, index)
    distance = abs(out["loss"].item() - ref["loss"].item())
    print(f"loss[{IDS[index]}]: device distance {distance:.3e}")
    margin(f"test_end_to_end_loss[{IDS[index]}]", "|loss - float64|", distance, BOUND_LOSS)
    assert distance <= BOUND_LOSS


# ---- 4: gradients -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_gradients(dev, index):
    V, R, H, W, patch_size, k = CASES[index]
    s, share, border, (_, grad_positions, grad_normals) = gradient_case(index)
    margin(f"test_gradients[{IDS[index]}]", "rays re-drawn", share, MAX_SHARE)
    margin(f"test_gradients[{IDS[index]}]", "border share (reported)", border, 1.0)
    assert share <= MAX_SHARE
    out = launch(dev, s, patch_size, k, backward=True, export=False)
    unconverged = ~s["converged"]
    assert (out["grad_positions"][unconverged] == 0).all() and (out["grad_normals"][unconverged] == 0).all()
    dp, dn = relative(out["grad_positions"], grad_positions), relative(out["grad_normals"], grad_normals)
    print(f"gradients[{IDS[index]}]: positions {dp:.3e} normals {dn:.3e} (re-drawn {share:.2f}, border {border:.4f})")
    margin(f"test_gradients[{IDS[index]}]", "grad positions / max", dp, BOUND_GRADIENT)
    margin(f"test_gradients[{IDS[index]}]", "grad normals / max", dn, BOUND_GRADIENT)
    assert dp <= BOUND_GRADIENT and dn <= BOUND_GRADIENT
    # the upstream gradient scales both -- to the precision the gradients are asserted at: it enters every term of sums that cancel
    scaled = launch(dev, s, patch_size, k, backward=True, upstream=-2.5, export=False)
    assert relative(scaled["grad_positions"], -2.5 * out["grad_positions"]) <= BOUND_GRADIENT
    assert relative(scaled["grad_normals"], -2.5 * out["grad_normals"]) <= BOUND_GRADIENT


# ---- 5: hazards ---------------------------------------------------------------------------------------------------------------------------
def hazard_scene():
    """V = 6, 96 x 320, 11 x 11.  Ray 0's plane is fronto-parallel (n = -z) and view 1's camera, unrotated and 100 m to the side, has its
    centre p_z 1e-6 behind that plane (within 1e-3 of it): there h_z = 1 - C_z / p_z = -1e-6 up to float32 rounding, h_z + 1e-6 is ~1e-8
    and the coordinates pass int32.  View 2 stands 1000 m to the side (patches wholly outside); view 3 is shifted by about half an image at the
    mean depth, so that patches straddle the image border (partly outside)."""
    s = pcr.scene(300, 6, 16, 96, 320, smooth=True, patch_size=(11, 11))
    s["normals"][0] = torch.tensor([0.0, 0.0, -1.0])
    p = s["positions"][0]
    s["E"][1] = torch.eye(4)
    s["E"][1, :3, 3] = -torch.tensor([p[0] + 100.0, p[1], p[2] * (1.0 + 1e-6)])    # R = I: the camera centre is -t
    s["E"][2] = torch.eye(4)
    s["E"][2, 0, 3] = 1000.0
    s["E"][3] = torch.eye(4)
    s["E"][3, 0, 3] = s["positions"][:, 2].mean() * 160.0 / s["K"][0, 0, 0]
    return s


def test_hazards(dev):
    patch_size, k = (11, 11), 4
    s = hazard_scene()
    H, W = s["images"].shape[-2:]
    ref = yardstick(s, patch_size, k)
    coordinates = ref["coordinates"]
    assert torch.isfinite(coordinates[1, 0]).all() and coordinates[1, 0].abs().max() > 2.0 ** 31      # finite in the yardstick, beyond int32
    assert (ref["patches"][1, 0] == 0).all()
    assert (ref["patches"][2] == 0).all()                                          # wholly outside
    outside = ((coordinates[3, ..., 0] < 0) | (coordinates[3, ..., 0] > W - 1)).any(dim=-1)
    inside = ((coordinates[3, ..., 0] > 0) & (coordinates[3, ..., 0] < W - 1)).any(dim=-1)
    assert (outside & inside).any()                                                # partly outside
    out = launch(dev, s, patch_size, k, backward=True)
    assert (out["patches"][1, 0] == 0).all() and (out["patches"][2] == 0).all()
    distance = (out["patches"].double() - ref["patches"]).abs().max().item()
    loss_distance = abs(out["loss"].item() - ref["loss"].item())
    margin("test_hazards", "max |patch - float64|", distance, BOUND_PATCHES)
    margin("test_hazards", "|loss - float64|", loss_distance, BOUND_LOSS)
    print(f"hazards: patches {distance:.3e} loss {loss_distance:.3e}")
    assert distance <= BOUND_PATCHES and loss_distance <= BOUND_LOSS
    assert torch.isfinite(out["grad_positions"]).all() and torch.isfinite(out["grad_normals"]).all()
    s["converged"] = torch.zeros_like(s["converged"])                             # the all-unconverged frame: loss 0, zero gradients
    none = launch(dev, s, patch_size, k, backward=True)
    assert none["loss"].item() == 0.0 and (none["stats"] == 0).all()
    assert (none["grad_positions"] == 0).all() and (none["grad_normals"] == 0).all()
    assert (none["coefficients"] == 0).all() and (none["selected"] == 0).all()
    assert torch.equal(none["patches"], out["patches"])                            # exported patches are sampled for every ray


# ---- 6: determinism and capture -------------------------------------------------------------------------------------------------------
def device_inputs(dev, s, gray):
    """What every call shares, on the device once (a capture allows no copy from the host)."""
    W = gray.shape[-1]
    return dict(gray=gray, K=s["K"].to(dev), E=s["E"].to(dev), indices=(s["pixels"][:, 1] * W + s["pixels"][:, 0]).to(dev), converged=s["converged"].to(dev))


def public_loss(d, patch_size, k, positions, normals):
    from vsrd_amd import losses
    return losses.patch_correlation_loss(d["gray"], d["K"], d["E"], d["indices"], positions, normals, d["converged"], patch_size, k)


def test_determinism_and_capture(dev):
    from vsrd_amd import losses
    index = 3
    V, R, H, W, patch_size, k = CASES[index]
    s, *_ = gradient_case(index)
    d = device_inputs(dev, s, losses.grayscale_images(s["images"].to(dev)))
    other = s["positions"] * 1.01

    def eager(values):
        p, n = values.to(dev).requires_grad_(True), s["normals"].to(dev).requires_grad_(True)
        loss = public_loss(d, patch_size, k, p, n)
        gp, gn = torch.autograd.grad(loss, [p, n])
        return loss.detach().clone(), gp.clone(), gn.clone()

    first, second, moved = eager(s["positions"]), eager(s["positions"]), eager(other)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert not torch.equal(first[1], moved[1])
    p, n = s["positions"].to(dev).requires_grad_(True), s["normals"].to(dev).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                  # warm-up: the workspace is allocated outside the capture
        torch.autograd.grad(public_loss(d, patch_size, k, p, n), [p, n])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = public_loss(d, patch_size, k, p, n)
        gp, gn = torch.autograd.grad(loss, [p, n])
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, (loss, gp, gn)):
        assert torch.equal(a, b)
    with torch.no_grad():
        p.copy_(other.to(dev))                                                     # through the captured input buffer
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(moved, (loss, gp, gn)):
        assert torch.equal(a, b)


# ---- 7: grayscale -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V, H, W", [(3, 24, 40), (3, 48, 97)])
def test_grayscale_bit_for_bit(dev, V, H, W):
    """gray = fma(0.114, b, fma(0.587, g, 0.2989 r)) in float32.  NumPy has no fma: a float32 product is exact in float64, the sum is then
    rounded to float64 and to float32 -- the same as one rounding unless the float64 sum falls on a float32 tie, which these seeded images do
    not hit.  H W = 48 x 97 is no multiple of 4: planes that are not 16-byte aligned, the scalar path."""
    images = torch.rand(V, 3, H, W, generator=torch.Generator().manual_seed(7 + W))
    r, g, b = (images[:, c].numpy().astype(np.float64) for c in range(3))
    w = [np.float64(np.float32(x)) for x in pcr.GRAY_WEIGHTS]
    t = (w[0] * r).astype(np.float32)
    t = (w[1] * g + t.astype(np.float64)).astype(np.float32)
    t = (w[2] * b + t.astype(np.float64)).astype(np.float32)
    gray = gray_planes(dev, images)
    assert gray.shape == (V, H, W) and gray.dtype == torch.float32
    assert np.array_equal(gray.numpy().view(np.int32), t.view(np.int32))
    offset = gray_planes(dev, torch.cat([torch.zeros(1), images.flatten()])[1:].view(V, 3, H, W))      # a base address that is not 16-byte aligned
    assert torch.equal(offset, gray)


# ---- 8: the public function ---------------------------------------------------------------------------------------------------------------
def test_public_function_shapes(dev):
    from vsrd_amd import losses
    index = 1
    V, R, H, W, patch_size, k = CASES[index]
    s, ref, out = forward_case(dev, index)
    images, K, E = s["images"].to(dev), s["K"].to(dev), s["E"].to(dev)
    indices = (s["pixels"][:, 1] * W + s["pixels"][:, 0]).to(dev)
    positions, normals, masks = s["positions"].to(dev)[None], s["normals"].to(dev)[None], s["converged"].to(dev)[None, :, None]
    loss, patches = losses.patch_correlation_loss(images, K[None], E[None], indices[None], positions, normals, masks, patch_size, k, return_patches=True)
    assert loss.dim() == 0 and patches.shape == (V, R, patch_size[0] * patch_size[1])
    assert loss.item() == out["loss"].item() and torch.equal(patches.cpu(), out["patches"])
    planes = losses.grayscale_images(images)
    again = losses.patch_correlation_loss(planes, K, E, indices, positions[0], normals[0], masks[0, :, 0], patch_size, k)
    assert again.dim() == 0 and again.item() == loss.item()
    with pytest.raises(ValueError):
        losses.patch_correlation_loss(planes, K[:-1], E, indices, positions, normals, masks, patch_size, k)


def test_public_function_on_sphere_traced_boxes(dev):
    """The main.py:747-851 shape: a hard union of three boxes, differentiable sphere tracing, surface normals, the loss, backward()."""
    from vsrd_amd import fields, losses, rendering
    V, H, W, patch_size, k, N = 6, 96, 320, (11, 11), 4, 3
    generator = torch.Generator().manual_seed(400)
    K, E = pcr.cameras(V, H, W)
    images = pcr.smooth_images(generator, V, H, W)
    locations = torch.tensor([[-2.0, 0.6, 14.0], [0.5, 0.5, 18.0], [2.5, 0.7, 12.0]])
    dimensions = torch.tensor([[0.9, 0.8, 2.0], [0.9, 0.8, 2.0], [0.8, 0.75, 1.8]])
    yaws = torch.tensor([0.3, -0.5, 1.1])
    rotations = torch.stack([torch.stack([torch.cos(yaws), torch.zeros(N), torch.sin(yaws)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                             torch.stack([-torch.sin(yaws), torch.zeros(N), torch.cos(yaws)], -1)], -2)
    aims = locations[torch.arange(48) % N] + torch.randn(48, 3, generator=generator) * torch.tensor([0.5, 0.4, 0.5])
    projected = aims @ K[0].T
    pixels = (projected[:, :2] / projected[:, 2:]).round().long()
    pixels[:, 0].clamp_(12, W - 13); pixels[:, 1].clamp_(12, H - 13)
    indices = (pixels[:, 1] * W + pixels[:, 0]).to(dev)
    directions = torch.nn.functional.normalize((torch.linalg.inv(K[0]) @ torch.nn.functional.pad(pixels.float(), (0, 1), value=1.0).T).T, dim=-1).to(dev)

    def trace(l, d):
        union = fields.hard_union([rendering.sdfs.translation(rendering.sdfs.rotation(fields.instance_field(rendering.sdfs.box(d[i]), i, N), rotations[i].to(dev)), l[i])
                                   for i in range(N)])
        positions, converged = rendering.sphere_tracing(union, torch.zeros(3, device=dev).expand(directions.shape[0], 3), directions, 100, 1e-3,
                                                        bounding_radius=100.0, initialization=False, differentiable=True)
        return union, positions, converged

    l, d = locations.to(dev).requires_grad_(True), dimensions.to(dev).requires_grad_(True)
    union, positions, converged = trace(l, d)
    normals = rendering.surface_normal(union, positions).detach()
    assert 0.25 < converged.float().mean().item()
    loss = losses.patch_correlation_loss(images.to(dev), K.to(dev), E.to(dev), indices, positions, normals, converged, patch_size, k)
    loss.backward()
    flags = converged.reshape(-1).cpu()
    ref_loss, ref_gp, _ = pcr.reference_gradients(images, K, E, pixels, positions.detach().cpu(), normals.cpu(), flags, patch_size, k)
    distance = abs(loss.item() - ref_loss.item())
    margin("test_public_function_on_sphere_traced_boxes", "|loss - float64|", distance, BOUND_LOSS)
    l2, d2 = locations.to(dev).requires_grad_(True), dimensions.to(dev).requires_grad_(True)
    _, positions2, _ = trace(l2, d2)
    assert torch.equal(positions2.detach(), positions.detach())
    positions2.backward(ref_gp.float().to(dev))
    dl, dd = relative(l.grad.cpu(), l2.grad.cpu()), relative(d.grad.cpu(), d2.grad.cpu())
    print(f"traced boxes: loss {distance:.3e} grad locations {dl:.3e} grad dimensions {dd:.3e} converged {flags.float().mean().item():.2f}")
    margin("test_public_function_on_sphere_traced_boxes", "grad locations / max", dl, BOUND_GRADIENT)
    margin("test_public_function_on_sphere_traced_boxes", "grad dimensions / max", dd, BOUND_GRADIENT)
    assert distance <= BOUND_LOSS and dl <= BOUND_GRADIENT and dd <= BOUND_GRADIENT
