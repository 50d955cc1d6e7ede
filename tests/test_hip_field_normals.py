"""The differentiable field normal on the device (csrc/aux_kernels.h: field_eval_backward_kernel<., true>; include/vsrd_hip.h:
vsrd_field_eval_adjoint; rendering.evaluate_field / surface_normal) against oracle.fields.InstanceUnion in float64 under torch.autograd:
the oracle writes the normal out analytically, so first-order autograd through it is the reference's double backward.

The bounds.  SENSITIVITY_* is the oracle's own sensitivity to rounding: its float32 run against its float64 run on the inputs of the
cases below (CPU, x86-64, torch 2.x).  DEVICE_* is the device's distance from the float64 oracle on the same inputs, measured on an MI355X
(gfx950).  Every comparison asserts three times the larger of the two; the worst case is named beside each constant.
The precedent for this kernel family, 2e-3 of a tensor's largest entry (tests/test_hip_render.py::test_field_evaluation_is_differentiable),
is not used as a bound: the measured ones are far below it.

Kinks.  The second derivative of the field jumps where a local coordinate or a q = |local| - half extent crosses 0, where the interior
arg max of q ties and where the hard arg min ties.  A point the float64 oracle puts within KINK of one of these is left out of the
comparison (its cotangents are zeroed, so shapes stay); at most MAX_SHARE of a case's points may be.
"""
import functools

import pytest
import torch

import patch_correlation_reference as pcr
from conftest import load_golden, margin
from oracle import fields as ofields

pytestmark = pytest.mark.gpu

T = 0.4
POINTS = 300                              # four full waves and a 44-lane tail
KINK = 1e-3
MAX_SHARE = 0.05
NAMES = ("locations", "dimensions", "orientations", "mlp_weights", "positions")

CASES = ["g10-box", "g10-residual", "n16-box", "n1-box"]
# Per case, the worst of soft / hard union, of the two losses and of the tensors (the worst one is named).  n1-box has a point (216) 1.05 mm
# outside a face, just beyond KINK: the box Hessian 1e-6 / (q^2 + 1e-6)^1.5 is 3.3e2 there and changes by 1.5e-3 of itself over the float32
# spacing of the point's position, so the oracle's own float32 run is 2.7e-4 of the largest entry away from its float64 run, a hundred times
# the other cases; the device is closer than that.
# max |x - float64| over the largest entry of the float64 tensor
SENSITIVITY_TENSOR = {"g10-box": 8.3e-7,        # soft, all cotangents, positions;  float32 oracle, CPU
                      "g10-residual": 1.7e-6,   # hard, normal alone, positions
                      "n16-box": 3.6e-6,        # hard, normal alone, positions
                      "n1-box": 2.8e-4}         # all cotangents, positions
DEVICE_TENSOR = {"g10-box": 9.8e-7,             # hard, all cotangents, positions;  MI355X
                 "g10-residual": 2.7e-6,        # hard, all cotangents, positions
                 "n16-box": 3.5e-6,             # hard, normal alone, positions
                 "n1-box": 8.1e-5}              # all cotangents, positions
# positions row by row: the smallest f with |row - float64 row| <= f (|float64 row| + f * the tensor's largest entry) for every row -- each row
# relative to its own norm plus the same fraction of the largest entry, so that one large row does not hide the others
SENSITIVITY_ROW = {"g10-box": 7.8e-5, "g10-residual": 1.6e-5, "n16-box": 6.6e-5, "n1-box": 9.2e-4}        # float32 oracle, CPU
DEVICE_ROW = {"g10-box": 7.1e-5, "g10-residual": 1.8e-5, "n16-box": 1.2e-4, "n1-box": 1.5e-3}             # MI355X
# the photometric chain (test 8): max |x - float64 chain| over the largest entry, the worst of locations / dimensions / rotations
SENSITIVITY_CHAIN = 1.4e-4                # float32 chain, CPU: rotations (locations 1.7e-5, dimensions 1.8e-5)
DEVICE_CHAIN = 1.7e-5                     # MI355X: rotations (locations 9.0e-6, dimensions 1.3e-5)
BOUND_TENSOR = {case: 3.0 * max(SENSITIVITY_TENSOR[case], DEVICE_TENSOR[case]) for case in CASES}
BOUND_ROW = {case: 3.0 * max(SENSITIVITY_ROW[case], DEVICE_ROW[case]) for case in CASES}
BOUND_CHAIN = 3.0 * max(SENSITIVITY_CHAIN, DEVICE_CHAIN)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """The boxes (and MLP weights) of a case, POINTS points around them (generator seed 3, centres + 1.5 randn: for g10 the very points of
    test_field_evaluation_is_differentiable) and random cotangents a [P], b [P,N], c [P,3] for distances, labels and normals."""
    if case.startswith("g10"):
        g = load_golden("g10_render_residual_n3_s16")
    elif case == "n16-box":
        g = load_golden("g4_render_n16_s64_mid")
    else:
        g = {k: v[:1] for k, v in load_golden("g10_render_residual_n3_s16").items() if k in NAMES}
    params = [g[k].float().clone() for k in NAMES[:3]]
    if case.endswith("residual"):
        params.append(g["mlp_weights"].float().clone())
    N = params[0].shape[0]
    gen = torch.Generator().manual_seed(3)
    centres = params[0][torch.randint(0, N, (POINTS,), generator=gen)]
    points = centres + torch.randn(POINTS, 3, generator=gen) * 1.5
    a, b, c = torch.randn(POINTS, generator=gen), torch.randn(POINTS, N, generator=gen), torch.randn(POINTS, 3, generator=gen)
    return params, points, (a, b, c)


def leaves_of(params, points, device, dtype=torch.float32):
    return [p.clone().to(device=device, dtype=dtype).requires_grad_(True) for p in params], points.clone().to(device=device, dtype=dtype).requires_grad_(True)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------------
def oracle_union(leaves):
    return ofields.InstanceUnion(leaves[0], leaves[2], leaves[1], T, leaves[3] if len(leaves) > 3 else None)


def oracle_outputs(union, points, hard):
    """(distances [P], labels [P,N] or None, gradient [P,3]): evaluate() for the soft union, the arg-min member's terms for the hard one."""
    if not hard:
        return union.evaluate(points)
    d, g_world = union.instance_terms(points)
    index = d.argmin(0)
    return d.gather(0, index[None])[0], None, g_world.gather(0, index[None, :, None].expand(1, -1, 3))[0]


def kink_distance(params, points, hard):
    """[P] float64: how far each point is from the nearest place where the second derivative jumps, over all members."""
    loc, dim, rot = (p.double() for p in params[:3])
    local = torch.einsum("npk,nkj->npj", points.double()[None] - loc[:, None], rot)
    q = local.abs() - dim[:, None]
    distance = torch.minimum(local.abs().min(-1).values, q.abs().min(-1).values)
    top = q.topk(2, dim=-1).values
    distance = torch.where(top[..., 0] < 0, torch.minimum(distance, top[..., 0] - top[..., 1]), distance)      # the interior arg max
    distance = distance.min(0).values
    if hard and loc.shape[0] > 1:
        with torch.no_grad():
            d, _ = oracle_union([p.double() for p in params]).instance_terms(points.double())
        low = d.topk(2, dim=0, largest=False).values
        distance = torch.minimum(distance, low[1] - low[0])
    return distance


@functools.lru_cache(maxsize=None)
def kept_points(case, hard):
    params, points, _ = case_inputs(case)
    return kink_distance(params, points, hard) >= KINK


def loss_of(outputs, cotangents, keep, normalise, only_normals):
    u, labels, gradient = outputs
    a, b, c = (w.to(device=u.device, dtype=u.dtype) * keep.to(u.device).reshape(-1, *([1] * (w.dim() - 1))).to(u.dtype) for w in cotangents)
    if normalise:
        gradient = torch.nn.functional.normalize(gradient, dim=-1)
    loss = (gradient * c).sum()
    if not only_normals:
        loss = loss + (u * a).sum() + (0.0 if labels is None else (labels * b).sum())
    return loss


@functools.lru_cache(maxsize=None)
def oracle_gradients(case, hard, normalise, dtype):
    """d loss / d (locations, dimensions, orientations, [mlp weights], positions) of the oracle in `dtype`, on the CPU."""
    params, points, cotangents = case_inputs(case)
    leaves, pts = leaves_of(params, points, torch.device("cpu"), dtype)
    loss = loss_of(oracle_outputs(oracle_union(leaves), pts, hard), cotangents, kept_points(case, hard), normalise, only_normals=normalise)
    return [t.double() for t in torch.autograd.grad(loss, leaves + [pts])]


# ---- the device ----------------------------------------------------------------------------------------------------------------------------------
def hip_field(leaves, hard):
    from vsrd_amd import fields, rendering
    loc, dim, rot = leaves[:3]
    N = loc.shape[0]

    def member(i):
        box = rendering.sdfs.box(dim[i])
        if len(leaves) > 3:
            box = fields.residual_composition(box, fields.ResidualField(leaves[3][i]))
        return rendering.sdfs.translation(rendering.sdfs.rotation(fields.instance_field(box, i, N), rot[i]), loc[i])
    members = [member(i) for i in range(N)]
    return fields.hard_union(members) if hard else fields.soft_union(members, T)


def device_gradients(dev, case, hard, normalise):
    from vsrd_amd import rendering
    params, points, cotangents = case_inputs(case)
    leaves, pts = leaves_of(params, points, dev)
    field = hip_field(leaves, hard)
    if normalise:
        outputs = (pts.new_zeros(POINTS), None, rendering.surface_normal(field, pts))
        loss = (outputs[2] * (cotangents[2] * kept_points(case, hard)[:, None]).to(dev)).sum()
    else:
        out = rendering.evaluate_field(field, pts, with_gradients=True, with_labels=not hard)
        outputs = (out[0][..., 0], None if hard else out[1], out[-1])
        loss = loss_of(outputs, cotangents, kept_points(case, hard), False, False)
    return [t.double().cpu() for t in torch.autograd.grad(loss, leaves + [pts])]


def tensor_distance(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def row_distance(got, want):
    """The smallest f with |got row - want row| <= f (|want row| + f max|want|) for every row: the positive root of a quadratic per row."""
    error, norm, largest = (got - want).norm(dim=-1), want.norm(dim=-1), want.abs().max().clamp_min(1e-30)
    return float(((torch.sqrt(norm * norm + 4.0 * largest * error) - norm) / (2.0 * largest)).max())


def packed(instances_like, dev):
    from vsrd_amd import fields
    loc, dim, rot = instances_like
    return fields.pack_instances(loc, rot, dim).to(dev)


def call(dev, instances, mlp, points, grad_distances, grad_labels, grad_gradients, hard, entry="adjoint"):
    """One call of vsrd_field_eval_adjoint / vsrd_field_eval_backward through the C ABI -> (grad_positions, grad_instances, grad_mlp)."""
    from vsrd_amd import _lib
    lib = _lib.load()
    P, N = points.shape[0], instances.shape[0]
    bytes_needed = lib.vsrd_workspace_bytes(N, 0 if mlp is None else 1)
    workspace = torch.empty(bytes_needed, dtype=torch.uint8, device=dev)
    gp = torch.full((P, 3), float("nan"), device=dev)
    gi = torch.full((N, 16), float("nan"), device=dev)
    gm = None if mlp is None else torch.full_like(mlp, float("nan"))
    field = _lib.make_field(instances, T, mlp)
    head = (field, _lib.ptr(points), P, _lib.ptr(grad_distances), _lib.ptr(grad_labels))
    tail = (1 if hard else 0, workspace.data_ptr(), bytes_needed, _lib.ptr(gp), _lib.ptr(gi), _lib.ptr(gm), _lib.stream())
    if entry == "adjoint":
        _lib.check(lib.vsrd_field_eval_adjoint(*head, _lib.ptr(grad_gradients), *tail))
    else:
        assert grad_gradients is None
        _lib.check(lib.vsrd_field_eval_backward(*head, *tail))
    torch.cuda.synchronize()
    return gp, gi, gm


def abi_inputs(dev, case, hard):
    params, points, (a, b, c) = case_inputs(case)
    instances = packed(params[:3], dev).contiguous()
    mlp = params[3].to(dev).contiguous() if len(params) > 3 else None
    return instances, mlp, points.to(dev).contiguous(), a.to(dev), (None if hard else b.to(dev).contiguous()), c.to(dev).contiguous()


# ---- 1-3: parity with the float64 oracle, kinks left out, measured bounds ---------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("case", CASES)
def test_parity_with_the_float64_oracle(dev, case, hard):
    """All three cotangents live at once through evaluate_field, then the normalised normal alone through surface_normal: gradients w.r.t.
    locations, dimensions, orientations, MLP weights and positions.  (device figures of an MI355X, worst over the cases: see DEVICE_*)"""
    tag = f"test_parity_with_the_float64_oracle[{case}-{'hard' if hard else 'soft'}]"
    share = 1.0 - float(kept_points(case, hard).float().mean())
    print(f"{tag}: {share:.3%} of the points within {KINK} of a kink are left out")
    assert share <= MAX_SHARE
    figures = []
    for normalise in (False, True):
        got = device_gradients(dev, case, hard, normalise)
        want = oracle_gradients(case, hard, normalise, torch.float64)
        own = oracle_gradients(case, hard, normalise, torch.float32)
        assert len(got) == len(want)
        names = [n for n in NAMES if n != "mlp_weights" or len(want) == 5]
        for name, a, b, c in zip(names, got, want, own):
            figures.append((f"{'normal' if normalise else 'all'} {name} / max", tensor_distance(a, b), tensor_distance(c, b), BOUND_TENSOR[case]))
        figures.append((f"{'normal' if normalise else 'all'} positions by row", row_distance(got[-1], want[-1]), row_distance(own[-1], want[-1]), BOUND_ROW[case]))
        assert float(want[2].abs().max()) > 0.0                # the rotations do get a gradient
    for what, device, sensitivity, bound in figures:
        print(f"{tag}: {what:32s} device {device:.3e} float32 oracle {sensitivity:.3e} bound {bound:.3e}")
        margin(tag, what.split(" ", 1)[1] if "row" in what else "tensor / max", device, bound)
    for what, device, sensitivity, bound in figures:
        assert device <= bound, (what, device, bound)


# ---- 4: known answers ----------------------------------------------------------------------------------------------------------------------
def one_box(dev, point, gamma, hard):
    instances = packed((torch.zeros(1, 3), torch.tensor([[1.0, 1.0, 2.0]]), torch.eye(3)[None]), dev)
    gp, gi, _ = call(dev, instances, None, torch.tensor([point], device=dev), None, None, torch.tensor([gamma], device=dev), hard)
    return gp[0].cpu(), gi[0].cpu()


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_known_answers(dev, hard):
    from vsrd_amd import _lib
    # q = (1, 2, -2): the corner region of two faces, r = sqrt(5 + 1e-6)
    gp, gi = one_box(dev, [2.0, 3.0, 0.0], [1.0, 0.0, 0.0], hard)
    r = (5.0 + 1e-6) ** 0.5
    x_bar = torch.tensor([0.8 / r, -0.4 / r, 0.0])
    torch.testing.assert_close(x_bar, torch.tensor([0.357771, -0.178885, 0.0]), rtol=0, atol=1e-6)
    torch.testing.assert_close(gp, x_bar, rtol=0, atol=1e-5)
    torch.testing.assert_close(gi[0:3], -x_bar, rtol=0, atol=1e-5)
    torch.testing.assert_close(gi[12:15], -x_bar, rtol=0, atol=1e-5)
    assert gi[15] == 0.0
    # inside the box, and in the face region of +x at q_x = 5: the gradient is (locally) a constant vector in the box frame, so only
    # the rotation gets anything, R_bar = gamma (x) gl.  Inside that is exact.  In the face region gl_x = 5 / sqrt(25 + 1e-6) = 1 - 2e-8 is
    # not quite constant: q_bar_x = gamma_x (1 - gl_x^2) / sqrt(25 + 1e-6) = 8e-9 gamma_x, which R_bar sees as rel (x) p_bar <= 6 * 8e-9 * 0.7
    # = 3.4e-8, beside a float32 gl_x that may be one spacing (6e-8) below 1: exact for a gamma in the face's plane (p_bar is exactly 0
    # then), within 2e-7 for a general one.
    for point, gamma, exact in (([0.2, 0.3, -0.4], [0.3, -0.5, 0.7], True), ([6.0, 0.3, -0.4], [0.0, -0.5, 0.7], True),
                                ([6.0, 0.3, -0.4], [0.3, -0.5, 0.7], False)):
        instances = packed((torch.zeros(1, 3), torch.tensor([[1.0, 1.0, 2.0]]), torch.eye(3)[None]), dev)
        lib = _lib.load()
        gl = torch.empty(1, 3, device=dev)
        _lib.check(lib.vsrd_field_eval(_lib.make_field(instances, T, None), _lib.ptr(torch.tensor([point], device=dev)), 1, None, _lib.ptr(gl), None,
                                       1 if hard else 0, _lib.stream()))
        gl = gl[0].cpu()
        assert gl.abs().max() > 0.99
        gp, gi = one_box(dev, point, gamma, hard)
        zero = torch.zeros(3)
        torch.testing.assert_close(gp, zero, rtol=0, atol=1e-6)
        torch.testing.assert_close(gi[0:3], zero, rtol=0, atol=1e-6)
        torch.testing.assert_close(gi[12:15], zero, rtol=0, atol=1e-6)
        expected = torch.tensor(gamma)[:, None] * gl[None, :]
        if exact:
            assert torch.equal(gi[3:12].reshape(3, 3), expected), (point, gamma, gi[3:12])
        else:
            torch.testing.assert_close(gi[3:12].reshape(3, 3), expected, rtol=0, atol=2e-7)
        assert gi[15] == 0.0


# ---- 5: the old entry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("case", ["g10-box", "g10-residual"])
def test_old_entry_is_the_new_one_without_a_normal_cotangent(dev, case, hard):
    instances, mlp, points, a, b, _ = abi_inputs(dev, case, hard)
    old = call(dev, instances, mlp, points, a, b, None, hard, entry="backward")
    new = call(dev, instances, mlp, points, a, b, None, hard, entry="adjoint")
    for x, y in zip(old, new):
        assert (x is None and y is None) or torch.equal(x, y)
    assert not torch.isnan(old[0]).any() and not torch.isnan(old[1]).any()


# ---- 6: determinism and tails ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("case", ["g10-box", "g10-residual"])
def test_determinism_and_tails(dev, case, hard):
    instances, mlp, points, a, b, c = abi_inputs(dev, case, hard)
    first = call(dev, instances, mlp, points, a, b, c, hard)
    again = call(dev, instances, mlp, points, a, b, c, hard)
    for x, y in zip(first, again):
        assert (x is None and y is None) or (torch.equal(x, y) and not torch.isnan(x).any())
    for P in (1, 63, 64, 65):                                  # a point's row does not depend on how many points the call has
        part = call(dev, instances, mlp, points[:P].contiguous(), a[:P].contiguous(), None if hard else b[:P].contiguous(), c[:P].contiguous(), hard)
        assert torch.equal(part[0], first[0][:P]), P
    # gamma = 0 is gamma = NULL.  Box-only fields: every output, bit for bit (what gamma adds is exactly zero).  Residual fields: the
    # parameter gradients bit for bit; the position gradient comes out of the MLP adjoint as R p_bar where the kernel without gamma
    # takes d_bar R gl from the forward jet -- two float32 evaluations of one number, so they agree to the measured bound of the rows
    # (each is within BOUND_ROW of the float64 value: twice that).
    null = call(dev, instances, mlp, points, a, b, None, hard)
    zero = call(dev, instances, mlp, points, a, b, torch.zeros_like(c), hard)
    assert torch.equal(null[1], zero[1])
    if mlp is None:
        assert torch.equal(null[0], zero[0])
    else:
        assert torch.equal(null[2], zero[2])
        distance = row_distance(zero[0].double().cpu(), null[0].double().cpu())
        print(f"test_determinism_and_tails[{case}]: gamma = 0 against NULL, positions by row {distance:.3e} (bound {2.0 * BOUND_ROW[case]:.3e})")
        assert distance <= 2.0 * BOUND_ROW[case]


# ---- 7: the autograd surface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True], ids=["box", "residual"])
def test_autograd_surface(dev, residual):
    """What requires grad and what does not; the finite-difference branch; sphere_tracing(differentiable=True) as before."""
    from vsrd_amd import rendering
    params, points, _ = case_inputs("g10-residual" if residual else "g10-box")
    leaves, pts = leaves_of(params, points, dev)
    field = hip_field(leaves, True)
    assert rendering.surface_normal(field, pts.detach()).requires_grad                       # a leaf of the field does
    detached = hip_field([p.detach() for p in leaves], True)
    assert rendering.surface_normal(detached, pts).requires_grad                             # the positions do
    assert not rendering.surface_normal(detached, pts.detach()).requires_grad                # nothing does
    with torch.no_grad():
        quiet = rendering.surface_normal(field, pts)
    assert not quiet.requires_grad and quiet.grad_fn is None
    assert torch.equal(quiet, rendering.surface_normal(field, pts).detach())
    out = rendering.evaluate_field(field, pts, with_gradients=True, with_labels=False)
    assert out[0].requires_grad and out[-1].requires_grad
    # the finite-difference branch: six distance evaluations, differentiable through the distances as before
    fd = rendering.surface_normal(field, pts, finite_difference_epsilon=1e-3)
    probes = torch.stack([pts + o for o in torch.eye(3, device=dev) * 1e-3] + [pts - o for o in torch.eye(3, device=dev) * 1e-3])
    d = rendering.evaluate_field(field, probes, with_labels=False)
    assert torch.equal(fd, torch.nn.functional.normalize(torch.cat([d[k] - d[k + 3] for k in range(3)], dim=-1), dim=-1)) and fd.requires_grad
    # sphere_tracing(differentiable=True) takes the normal as a constant (the reference's autograd.grad without create_graph): its
    # gradients are those of its own formula on a detached normal, bit for bit
    gen = torch.Generator().manual_seed(5)
    directions = torch.nn.functional.normalize(params[0][torch.arange(64) % 3] + torch.randn(64, 3, generator=gen) * 0.3, dim=-1).to(dev)
    origins, probe = torch.zeros(64, 3, device=dev), torch.randn(64, 3, generator=gen).to(dev)
    leaves, _ = leaves_of(params, torch.zeros(1, 3), dev)
    traced, converged = rendering.sphere_tracing(hip_field(leaves, True), origins, directions, 64, 1e-3, differentiable=True)
    assert int(converged.sum()) > 16 and traced.requires_grad
    got = torch.autograd.grad((traced * probe).sum(), leaves)
    again, _ = leaves_of(params, torch.zeros(1, 3), dev)
    field = hip_field(again, True)
    plain, flags = rendering.sphere_tracing(field, origins, directions, 64, 1e-3)
    assert torch.equal(flags, converged) and not plain.requires_grad
    out = rendering.evaluate_field(field, plain, with_gradients=True, with_labels=False)
    sdf, normals = out[0], out[-1].detach()
    step = -sdf / (normals * directions).sum(dim=-1, keepdim=True)
    expected = torch.where(flags, plain + directions * step, plain)
    assert torch.equal(expected.detach(), traced.detach())
    for a, b in zip(got, torch.autograd.grad((expected * probe).sum(), again)):
        assert torch.equal(a, b)


# ---- 8: the photometric chain ---------------------------------------------------------------------------------------------------------------
def test_photometric_chain_reaches_the_rotations(dev):
    """main.py:747-851 on the scene of test_public_function_on_sphere_traced_boxes with the rotations as leaves: traced positions
    (differentiable), attached normals, the patch-correlation loss, backward() -- against the float64 gradients of the loss w.r.t.
    positions and normals (at the device's positions and normals) pulled back through the float64 oracle's Newton step and normalised
    hard-union gradient.  (device figures of an MI355X: see DEVICE_CHAIN)"""
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
    directions = torch.nn.functional.normalize((torch.linalg.inv(K[0]) @ torch.nn.functional.pad(pixels.float(), (0, 1), value=1.0).T).T, dim=-1)
    origins = torch.zeros(48, 3, device=dev)

    def union_of(l, d, r):
        return fields.hard_union([rendering.sdfs.translation(rendering.sdfs.rotation(fields.instance_field(rendering.sdfs.box(d[i]), i, N), r[i]), l[i])
                                  for i in range(N)])

    def device_chain(detach_normals):
        leaves = [t.clone().to(dev).requires_grad_(True) for t in (locations, dimensions, rotations)]
        union = union_of(*leaves)
        positions, converged = rendering.sphere_tracing(union, origins, directions.to(dev), 100, 1e-3, bounding_radius=100.0, initialization=False,
                                                        differentiable=True)
        normals = rendering.surface_normal(union, positions)
        used = normals.detach() if detach_normals else normals
        loss = losses.patch_correlation_loss(images.to(dev), K.to(dev), E.to(dev), indices, positions, used, converged, patch_size, k)
        loss.backward()
        return [t.grad.double().cpu() for t in leaves], positions.detach().cpu(), normals.detach().cpu(), converged.reshape(-1).cpu(), union

    got, positions, normals, flags, union = device_chain(False)
    constant, positions2, _, _, _ = device_chain(True)
    assert torch.equal(positions, positions2) and 0.25 < flags.float().mean().item()
    with torch.no_grad():
        start, flags0 = rendering.sphere_tracing(union, origins, directions.to(dev), 100, 1e-3, bounding_radius=100.0, initialization=False)
    assert torch.equal(flags0.reshape(-1).cpu(), flags)
    start = start.cpu()

    def oracle_chain(dtype):
        _, gp, gn = pcr.reference_gradients(images, K, E, pixels, positions, normals, flags, patch_size, k, dtype=dtype)
        leaves = [t.clone().to(dtype).requires_grad_(True) for t in (locations, dimensions, rotations)]
        field = ofields.InstanceUnion(leaves[0], leaves[2], leaves[1], T)
        x0, r = start.to(dtype).requires_grad_(True), directions.to(dtype)
        sdf = field.hard_distance(x0)
        constant_normal, = torch.autograd.grad(sdf.sum(), x0, retain_graph=True)
        x1 = torch.where(flags[:, None], x0.detach() + r * (-sdf / (constant_normal * r).sum(-1))[:, None], x0.detach())
        n1 = torch.nn.functional.normalize(oracle_outputs(field, x1, True)[2], dim=-1)
        return [t.double() for t in torch.autograd.grad([x1, n1], leaves, [gp.to(dtype), gn.to(dtype)])]

    want, own = oracle_chain(torch.float64), oracle_chain(torch.float32)
    tag = "test_photometric_chain_reaches_the_rotations"
    figures = [(name, tensor_distance(a, b), tensor_distance(c, b)) for name, a, b, c in zip(NAMES, got, want, own)]
    for name, device, sensitivity in figures:
        print(f"{tag}: grad {name:12s} / max  device {device:.3e} float32 chain {sensitivity:.3e} bound {BOUND_CHAIN:.3e}")
        margin(tag, "grad / max", device, BOUND_CHAIN)
    # the rotations get a gradient, and it is not the one of constant normals (what the code before this gave: positions only)
    assert float(got[2].abs().max()) > 0.0
    apart = tensor_distance(constant[2], want[2])
    print(f"{tag}: rotation gradient with detached normals is {apart:.3e} of the largest entry away from the float64 chain")
    assert apart > 10.0 * BOUND_CHAIN and not torch.equal(constant[2], got[2])
    for name, device, sensitivity in figures:
        assert device <= BOUND_CHAIN, (name, device, BOUND_CHAIN)
