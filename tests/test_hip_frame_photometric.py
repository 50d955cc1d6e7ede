"""vsrd_frame_photometric (include/vsrd_hip.h; csrc/frame_photometric.h): one frame's photometric term in ONE call -- gather, trace, Newton
step, normal, patch correlation forward and backward, the two field adjoints, the accumulation into the render step's gradients -- against

  * the device autograd composition rendering.sphere_tracing(differentiable=True) -> rendering.surface_normal ->
    losses.patch_correlation_loss on the same packed instances: p1, converged, n, the loss and (sum, count) BIT FOR BIT;
  * the float64 chain of tests/test_hip_field_normals.py::test_photometric_chain_reaches_the_rotations (pcr.reference_gradients pulled
    back through oracle.fields.InstanceUnion's Newton step and normalised hard-union gradient): the term's own gradients.

The scene is that test's: V = 6, 96 x 320, N = 3, 11 x 11 patches, k = 4, 100 iterations, criterion 1e-3, yaw rotations, smooth images.

The gradient bound.  Distances are max |x - float64| over the largest entry of the float64 tensor.  The float32 run of the same chain on
the CPU is the yardstick's own sensitivity to rounding; the bound of a case is three times the larger of that figure -- computed by the
test from the oracle alone -- and SENSITIVITY_CHAIN, the figure test_hip_field_normals.py records for this scene, and never above the
2e-3 ceiling of this kernel family.  The device's figures are printed and recorded with conftest.margin.
Measured on an MI355X (gfx950), worst tensor of each case, device / float32 chain (bound), and the distance to the device composition's
gradients: box-48 1.6e-5 / 1.3e-4 (4.2e-4), 1.0e-7; residual-48 1.6e-5 / 2.5e-4 (7.5e-4), 1.8e-7; box-100 1.5e-5 / 6.4e-5 (4.2e-4),
1.8e-7; one-box-48 1.8e-5 / 9.7e-5 (4.2e-4), 2.7e-7.  89.6 %, 66.7 %, 92.0 % and 89.6 % of the rays converge.
"""
import functools

import pytest
import torch

import patch_correlation_reference as pcr
from conftest import margin
from oracle import fields as ofields

pytestmark = pytest.mark.gpu

T = 0.4
V, H, W, PATCH, TOP_K = 6, 96, 320, (11, 11), 4
ITERATIONS, CRITERION, RADIUS = 100, 1e-3, 100.0
SCALE = 0.37
SENSITIVITY_CHAIN = 1.4e-4                # test_hip_field_normals.py: the float32 chain of this scene on the CPU
CEILING = 2e-3
CANARY, CANARY_VALUE = 64, 123
CASES = {"box-48": (3, 48, False), "residual-48": (3, 48, True), "box-100": (3, 100, False), "one-box-48": (1, 48, False)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


# ---- the scene --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(case, behind=False):
    """Host tensors of a case: cameras, images, boxes (and centred-to-be MLP weights), the pixel indices of the rays."""
    N, R, residual = CASES[case]
    generator = torch.Generator().manual_seed(400)
    K, E = pcr.cameras(V, H, W)
    images = pcr.smooth_images(generator, V, H, W)
    locations = torch.tensor([[-2.0, 0.6, 14.0], [0.5, 0.5, 18.0], [2.5, 0.7, 12.0]])[:N]
    dimensions = torch.tensor([[0.9, 0.8, 2.0], [0.9, 0.8, 2.0], [0.8, 0.75, 1.8]])[:N]
    yaws = torch.tensor([0.3, -0.5, 1.1])[:N]
    rotations = torch.stack([torch.stack([torch.cos(yaws), torch.zeros(N), torch.sin(yaws)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                             torch.stack([-torch.sin(yaws), torch.zeros(N), torch.cos(yaws)], -1)], -2)
    aims = locations[torch.arange(R) % N] + torch.randn(R, 3, generator=generator) * torch.tensor([0.5, 0.4, 0.5])
    projected = aims @ K[0].T
    pixels = (projected[:, :2] / projected[:, 2:]).round().long()
    pixels[:, 0].clamp_(12, W - 13); pixels[:, 1].clamp_(12, H - 13)
    indices = pixels[:, 1] * W + pixels[:, 0]
    mlp = torch.randn(N, 1617, generator=generator) * 0.05 if residual else None
    if behind:
        locations = locations * torch.tensor([1.0, 1.0, -1.0])
    return dict(K=K, E=E, images=images, locations=locations, dimensions=dimensions, rotations=rotations, pixels=pixels, indices=indices, mlp=mlp)


_device_cache = {}


def on_device(dev, case, behind=False):
    """The case's device tensors, made once: gray planes, camera tables, the ray table of view 0, packed instances, centred MLP weights."""
    key = (case, behind)
    if key not in _device_cache:
        from vsrd_amd import fields, losses, rendering
        from vsrd_amd.rendering import renderers
        s = scene(case, behind)
        K, E = s["K"].to(dev), s["E"].to(dev)
        cam, dirs = rendering.ray_casting((H, W), K, E)
        _device_cache[key] = dict(
            K=K.contiguous(), E=E.contiguous(), gray=losses.grayscale_images(s["images"].to(dev)), camera=cam[0].contiguous(),
            directions=dirs[0].reshape(-1, 3).contiguous(), indices=s["indices"].to(dev),
            instances=fields.pack_instances(s["locations"], s["rotations"], s["dimensions"]).to(dev).contiguous(),
            mlp=None if s["mlp"] is None else renderers._centre_mlp(s["mlp"].to(dev).contiguous()).contiguous())
    return _device_cache[key]


# ---- the call ----------------------------------------------------------------------------------------------------------------------------
def guarded(shape, fill, dev, dtype=torch.float32):
    """(view, whole): a buffer of `shape` with CANARY elements of CANARY_VALUE behind it."""
    count = 1
    for x in shape:
        count *= x
    whole = torch.full((count + CANARY,), CANARY_VALUE, dtype=dtype, device=dev)
    view = whole[:count].view(shape)
    if isinstance(fill, torch.Tensor):
        view.copy_(fill.to(dev))
    else:
        view.fill_(fill)
    return view, whole


def pattern(rows, columns, dev):
    """A known pattern with both zeros' signs in it: k / 7 - 3, every 5th entry +0.0, every 11th -0.0."""
    values = torch.arange(rows * columns, dtype=torch.float32) / 7.0 - 3.0
    values[::5] = 0.0
    values[::11] = -0.0
    return values.view(rows, columns).to(dev)


class Call:
    """The buffers of one vsrd_frame_photometric call (outputs with canaries, grad_instances laid out for two rows more than N) and the call."""

    def __init__(self, dev, d, rays=None, extra_rows=2):
        from vsrd_amd import _lib
        self.lib, self.dev, self.d = _lib.load(), dev, d
        N = d["instances"].shape[0]
        R = int(d["indices"].numel()) if rays is None else rays
        self.N, self.R, self.residual = N, R, d["mlp"] is not None
        nan = float("nan")
        self.buffers, self.wholes = {}, {}
        spec = dict(loss=((1,), nan), stats=((2,), nan), own_instances=((N, 16), nan), own_mlp=((N, 1617), nan), positions=((R, 3), nan),
                    normals=((R, 3), nan), grad_instances=((N + extra_rows, 16), pattern(N + extra_rows, 16, dev)),
                    grad_mlp=((N, 1617), pattern(N, 1617, dev)))
        for name, (shape, fill) in spec.items():
            self.buffers[name], self.wholes[name] = guarded(shape, fill, dev)
        self.buffers["converged"], self.wholes["converged"] = guarded((R,), 77, dev, torch.uint8)
        self.before = {name: whole.clone() for name, whole in self.wholes.items()}
        nbytes = self.lib.vsrd_frame_photometric_workspace_bytes(N, 1 if self.residual else 0, V, R, PATCH[0] * PATCH[1])
        assert nbytes > 0
        self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        self.workspace_bytes = nbytes
        self.patch = _lib.PatchCorrelationConfig(V, R, H, W, PATCH[0], PATCH[1], TOP_K, 0, 1.0e-6, 1.0e-12)
        self.config = _lib.FramePhotometricConfig(ITERATIONS, CRITERION, RADIUS, SCALE, 1, 0)
        self.field = _lib.make_field(d["instances"], T, d["mlp"])

    def refill(self):
        for name, whole in self.wholes.items():
            whole.copy_(self.before[name])

    def __call__(self, **replace):
        from vsrd_amd import _lib
        d, b = self.d, self.buffers
        offset = (-self.workspace.data_ptr()) % 256
        arguments = dict(config=self.config, patch=self.patch, field=self.field, camera=_lib.ptr(d["camera"]), directions=_lib.ptr(d["directions"]),
                         gray=_lib.ptr(d["gray"]), intrinsics=_lib.ptr(d["K"]), extrinsics=_lib.ptr(d["E"]), indices=d["indices"].data_ptr(),
                         workspace=self.workspace.data_ptr() + offset, workspace_bytes=self.workspace_bytes, loss=_lib.ptr(b["loss"]),
                         stats=_lib.ptr(b["stats"]), own_instances=_lib.ptr(b["own_instances"]), own_mlp=_lib.ptr(b["own_mlp"]),
                         grad_instances=_lib.ptr(b["grad_instances"]), grad_mlp=_lib.ptr(b["grad_mlp"]), positions=_lib.ptr(b["positions"]),
                         normals=_lib.ptr(b["normals"]), converged=b["converged"].data_ptr(), stream=_lib.stream())
        arguments.update(replace)
        return self.lib.vsrd_frame_photometric(*arguments.values())

    def canaries_intact(self):
        return all(torch.equal(whole[-CANARY:], self.before[name][-CANARY:]) for name, whole in self.wholes.items())

    def untouched(self):
        return all(torch.equal(whole.view(torch.uint8), self.before[name].view(torch.uint8)) for name, whole in self.wholes.items())

    def snapshot(self):
        return {name: whole.clone() for name, whole in self.wholes.items()}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


# ---- the device autograd composition -----------------------------------------------------------------------------------------------------
def forward_stats(d, out):
    """(sum, count) of the composition's loss -- patch_correlation_loss keeps them to itself: the library's forward on its positions and normals."""
    from vsrd_amd import _lib
    lib, dev = _lib.load(), d["gray"].device
    R = out["positions"].shape[0]
    config = _lib.PatchCorrelationConfig(V, R, H, W, PATCH[0], PATCH[1], TOP_K, 0, 1.0e-6, 1.0e-12)
    pixels = torch.stack([d["indices"] % W, d["indices"] // W], dim=-1).to(torch.int32).contiguous()
    workspace = torch.empty(lib.vsrd_patch_correlation_workspace_bytes(V, R, PATCH[0] * PATCH[1]), dtype=torch.uint8, device=dev)
    loss, stats = torch.empty(1, device=dev), torch.empty(2, device=dev)
    _lib.check(lib.vsrd_patch_correlation_forward(config, _lib.ptr(d["gray"]), _lib.ptr(d["K"]), _lib.ptr(d["E"]), _lib.iptr(pixels),
                                                  _lib.ptr(out["positions"].contiguous()), _lib.ptr(out["normals"].contiguous()),
                                                  out["converged"].to(torch.uint8).contiguous().data_ptr(), workspace.data_ptr(), workspace.numel(),
                                                  _lib.ptr(loss), _lib.ptr(stats), None, None, None, _lib.stream()))
    assert torch.equal(loss, out["loss"])
    return stats


def composition(d):
    """-> dict(positions, normals, converged, loss, grad_instances, grad_mlp) of the autograd composition on the packed instances."""
    from vsrd_amd import fields, losses, rendering
    instances = d["instances"].clone().requires_grad_(True)
    mlp = None if d["mlp"] is None else d["mlp"].clone().requires_grad_(True)
    block = fields.FieldBlock(instances, T, mlp, None, hard=True)
    directions = d["directions"][d["indices"]]
    positions, converged = rendering.sphere_tracing(block, d["camera"], directions, ITERATIONS, CRITERION, bounding_radius=RADIUS, initialization=False,
                                                    differentiable=True)
    normals = rendering.surface_normal(block, positions)
    loss = losses.patch_correlation_loss(d["gray"], d["K"], d["E"], d["indices"], positions, normals, converged, PATCH, TOP_K)
    out = dict(positions=positions.detach(), normals=normals.detach(), converged=converged.reshape(-1), loss=loss.detach().reshape(1))
    out["stats"] = forward_stats(d, out)
    if bool(converged.any()):
        loss.backward()
        out["grad_instances"], out["grad_mlp"] = instances.grad, None if mlp is None else mlp.grad
    with torch.no_grad():
        out["start"] = rendering.sphere_tracing(block, d["camera"], directions, ITERATIONS, CRITERION, bounding_radius=RADIUS, initialization=False)[0]
    return out


# ---- the float64 chain --------------------------------------------------------------------------------------------------------------------
def oracle_chain(case, dtype, positions, normals, flags, start, directions, mlp):
    """d loss / d (locations, dimensions, rotations[, MLP weights]) of the chain in `dtype` on the CPU, at the device's positions and normals."""
    s = scene(case)
    _, gp, gn = pcr.reference_gradients(s["images"], s["K"], s["E"], s["pixels"], positions, normals, flags, PATCH, TOP_K, dtype=dtype)
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in (s["locations"], s["dimensions"], s["rotations"])]
    if mlp is not None:
        leaves.append(mlp.clone().to(dtype).requires_grad_(True))
    field = ofields.InstanceUnion(leaves[0], leaves[2], leaves[1], T, leaves[3] if mlp is not None else None)
    x0, r = start.to(dtype).requires_grad_(True), directions.to(dtype)
    sdf = field.hard_distance(x0)
    constant_normal, = torch.autograd.grad(sdf.sum(), x0, retain_graph=True)
    x1 = torch.where(flags[:, None], x0.detach() + r * (-sdf / (constant_normal * r).sum(-1))[:, None], x0.detach())
    d, g_world = field.instance_terms(x1)
    index = d.argmin(0)
    n1 = torch.nn.functional.normalize(g_world.gather(0, index[None, :, None].expand(1, -1, 3))[0], dim=-1)
    return [t.double() for t in torch.autograd.grad([x1, n1], leaves, [gp.to(dtype), gn.to(dtype)])]


def tensor_distance(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def unpacked(grad_instances):
    """[N,16] -> (locations [N,3], dimensions [N,3], rotations [N,3,3]) in the order of the chain's leaves."""
    g = grad_instances.double().cpu()
    return [g[:, 0:3], g[:, 12:15], g[:, 3:12].reshape(-1, 3, 3)]


# ---- 1: the forward bits, the gradients, the accumulate ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_composition_and_the_float64_chain(dev, case):
    """(the figures of an MI355X: the module's docstring)"""
    from vsrd_amd import _lib
    tag = f"test_against_the_composition_and_the_float64_chain[{case}]"
    d = on_device(dev, case)
    N, R, residual = CASES[case]
    call = Call(dev, d)
    _lib.check(call())
    torch.cuda.synchronize()
    b = call.buffers
    want = composition(d)
    share = float(want["converged"].float().mean())
    print(f"{tag}: {share:.1%} of {R} rays converge; loss {float(b['loss']):.7f}, stats {b['stats'].tolist()}")
    assert share > 0.25
    # the forward: bit for bit
    assert torch.equal(b["converged"], want["converged"].to(torch.uint8))
    assert same_bits(b["positions"], want["positions"]), float((b["positions"] - want["positions"]).abs().max())
    assert same_bits(b["normals"], want["normals"]), float((b["normals"] - want["normals"]).abs().max())
    assert same_bits(b["loss"], want["loss"]), (float(b["loss"]), float(want["loss"]))
    assert float(b["stats"][1]) > 0 and same_bits(b["stats"], want["stats"]), (b["stats"].tolist(), want["stats"].tolist())
    # the term's own gradients: against the float64 chain, beside the float32 chain
    host = [want[k].cpu() for k in ("positions", "normals", "converged", "start")]
    directions = d["directions"][d["indices"]].cpu()
    mlp = None if d["mlp"] is None else d["mlp"].cpu()
    exact = oracle_chain(case, torch.float64, *host, directions, mlp)
    own = oracle_chain(case, torch.float32, *host, directions, mlp)
    got = unpacked(b["own_instances"]) + ([b["own_mlp"].double().cpu()] if residual else [])
    composed = unpacked(want["grad_instances"]) + ([want["grad_mlp"].double().cpu()] if residual else [])
    names = ["locations", "dimensions", "rotations"] + (["mlp_weights"] if residual else [])
    sensitivity = max(tensor_distance(c, e) for c, e in zip(own, exact))
    bound = min(3.0 * max(sensitivity, SENSITIVITY_CHAIN), CEILING)
    figures = []
    for name, g, e, o, c in zip(names, got, exact, own, composed):
        figures.append((name, tensor_distance(g, e), tensor_distance(o, e), tensor_distance(g, c)))
        print(f"{tag}: grad {name:12s} / max  device {figures[-1][1]:.3e}  float32 chain {figures[-1][2]:.3e}  bound {bound:.3e}  "
              f"to the device composition {figures[-1][3]:.3e}")
        margin(tag, "grad / max", figures[-1][1], bound)
        margin(tag, "grad / max to composition", figures[-1][3], bound)
    assert float(exact[2].abs().max()) > 0.0                    # the rotations do get a gradient
    for name, device, _, _ in figures:
        assert device <= bound, (name, device, bound)
    # the accumulate: pattern + scale * own, one rounding (the fused multiply-add), rows beyond N and every canary untouched
    scale = float(torch.tensor(SCALE, dtype=torch.float32))
    before = call.before["grad_instances"][:-CANARY].view(N + 2, 16)
    expected = (before[:N].double() + scale * b["own_instances"].double()).float()
    assert same_bits(b["grad_instances"][:N], expected)
    assert same_bits(b["grad_instances"][N:], before[N:])
    before_mlp = call.before["grad_mlp"][:-CANARY].view(N, 1617)
    if residual:
        assert same_bits(b["grad_mlp"], (before_mlp.double() + scale * b["own_mlp"].double()).float())
    else:
        assert same_bits(b["grad_mlp"], before_mlp) and same_bits(call.wholes["own_mlp"], call.before["own_mlp"])
    assert call.canaries_intact()
    # finish: record[4] += weight * loss, the product rounded and then the sum
    record, whole = guarded((5,), torch.tensor([0.1, 0.2, 0.3, 0.4, 1.7]), dev)
    weight = torch.tensor(0.05, dtype=torch.float32, device=dev)
    expected = record.clone()
    expected[4] = record[4] + weight * b["loss"][0]
    _lib.check(call.lib.vsrd_frame_photometric_finish(_lib.ptr(b["loss"]), _lib.ptr(b["stats"]), float(weight), _lib.ptr(record), _lib.stream()))
    torch.cuda.synchronize()
    assert same_bits(record, expected) and bool((whole[-CANARY:] == CANARY_VALUE).all())


# ---- 2: no converged ray ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["box-48", "residual-48"])
def test_no_ray_converges(dev, case):
    """Boxes behind the camera: loss 0, the term's own gradients zero, grad_instances / grad_mlp and the record with the bits they had."""
    from vsrd_amd import _lib
    d = on_device(dev, case, behind=True)
    call = Call(dev, d)
    _lib.check(call())
    torch.cuda.synchronize()
    b = call.buffers
    assert int(b["converged"].sum()) == 0
    assert same_bits(b["loss"], torch.zeros(1, device=dev)) and same_bits(b["stats"], torch.zeros(2, device=dev))
    assert same_bits(b["own_instances"], torch.zeros_like(b["own_instances"]))
    if CASES[case][2]:
        assert same_bits(b["own_mlp"], torch.zeros_like(b["own_mlp"]))
    for name in ("grad_instances", "grad_mlp"):
        assert same_bits(call.wholes[name], call.before[name]), name
    assert call.canaries_intact()
    record, whole = guarded((5,), torch.tensor([0.1, -0.0, 0.3, 0.4, -0.0]), dev)
    kept = whole.clone()
    _lib.check(call.lib.vsrd_frame_photometric_finish(_lib.ptr(b["loss"]), _lib.ptr(b["stats"]), 0.05, _lib.ptr(record), _lib.stream()))
    torch.cuda.synchronize()
    assert same_bits(whole, kept)


# ---- 3: determinism, capture and replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["box-100", "residual-48"])
def test_two_calls_and_a_replay_give_the_same_bits(dev, case):
    from vsrd_amd import _lib
    d = on_device(dev, case)
    call = Call(dev, d)
    results = []
    for _ in range(2):
        call.refill()
        _lib.check(call())
        torch.cuda.synchronize()
        results.append(call.snapshot())
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.graph(graph, stream=stream):
        call.refill()
        _lib.check(call())
    call.refill()
    for whole in call.wholes.values():
        whole.fill_(3)                                           # (the replay's own refill puts the start values back)
    graph.replay()
    torch.cuda.synchronize()
    results.append(call.snapshot())
    for name in call.wholes:
        assert same_bits(results[0][name], results[1][name]), name
        assert same_bits(results[0][name], results[2][name]), name
    assert not torch.isnan(results[0]["own_instances"][:-CANARY]).any()


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    from vsrd_amd import _lib
    d = on_device(dev, "residual-48")
    call = Call(dev, d)
    lib = call.lib
    two = _lib.FramePhotometricConfig(ITERATIONS, CRITERION, RADIUS, SCALE, 2, 1 << 20)
    assert call(config=two) == _lib.E_UNSUPPORTED
    invalid = []
    for name in ("config", "patch", "field", "camera", "directions", "gray", "intrinsics", "extrinsics", "indices", "loss", "stats", "own_instances",
                 "own_mlp", "grad_instances", "grad_mlp"):
        invalid.append((name, call(**{name: None})))

    def patch(**changes):
        values = dict(num_views=V, num_rays=call.R, height=H, width=W, patch_width=PATCH[0], patch_height=PATCH[1], top_k=TOP_K, target_view=0,
                      sample_epsilon=1.0e-6, correlation_epsilon=1.0e-12)
        values.update(changes)
        return _lib.PatchCorrelationConfig(*values.values())
    invalid.append(("rays beyond the sampler's limit", call(patch=patch(num_rays=2049))))
    invalid.append(("no ray", call(patch=patch(num_rays=0))))
    invalid.append(("top_k beyond the views", call(patch=patch(top_k=V + 1))))
    invalid.append(("too many views", call(patch=patch(num_views=33))))
    invalid.append(("patch too large", call(patch=patch(patch_width=17, patch_height=17))))
    many = _lib.Field(65, T, d["instances"].data_ptr(), d["mlp"].data_ptr())
    invalid.append(("too many instances", call(field=many)))
    negative = _lib.FramePhotometricConfig(-1, CRITERION, RADIUS, SCALE, 1, 0)
    invalid.append(("negative iterations", call(config=negative)))
    for name, code in invalid:
        assert code == _lib.E_INVALID_ARGUMENT, (name, code)
    assert call(workspace=None) == _lib.E_WORKSPACE and call(workspace_bytes=call.workspace_bytes - 1) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert call.untouched()
    assert lib.vsrd_frame_photometric_workspace_bytes(65, 0, V, 48, 121) == 0 and lib.vsrd_frame_photometric_workspace_bytes(3, 0, V, 2049, 121) == 0
    assert lib.vsrd_frame_photometric_workspace_bytes(3, 0, V, 48, 289) == 0 and lib.vsrd_frame_photometric_workspace_bytes(3, 0, 33, 48, 121) == 0
    assert lib.vsrd_frame_photometric_finish(None, _lib.ptr(call.buffers["stats"]), 1.0, _lib.ptr(call.buffers["loss"]), _lib.stream()) == _lib.E_INVALID_ARGUMENT
    # the call still works after all that
    _lib.check(call())
    torch.cuda.synchronize()
    assert not call.untouched() and call.canaries_intact()
