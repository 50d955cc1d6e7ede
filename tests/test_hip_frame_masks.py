"""vsrd_frame_masks (csrc/frame_masks.h) on the GPU: the bit layout over widths, the existing entry points and the float64 oracle as
references, counts, batches with headers, the Philox path, empty views, argument validation, and FrameOptimizer / FrameBatch.masks()."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import fields as ofields, rendering as orendering, tracing as otracing

pytestmark = pytest.mark.gpu

LABEL_TOL = 1.0e-4        # the project's north-star bound (tests/test_hip_render.py:12)
H, S = 6, 16
TRACE = (64, 0.01, 100.0)                 # iterations, convergence criterion, bounding radius
T, STD, RATIO = 0.3, 0.3, 0.5
RANGE = (0.0, 100.0)
THRESHOLD = 0.5
FOCAL = 60.0
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def scene(N):
    """2-3 boxes 9-16 m in front of the camera: box 1 stands behind box 0 and overlaps it on screen, box 2 stands apart; rays between and
    beside them miss."""
    loc = torch.tensor([[-2.0, 0.3, 10.0], [-1.0, 0.1, 16.0], [3.0, 0.2, 9.0]])[:N]
    dim = torch.tensor([[0.9, 0.45, 1.8], [1.0, 0.6, 2.0], [0.8, 0.5, 1.6]])[:N]
    yaw = torch.tensor([0.3, -0.4, 1.1])[:N]
    rot = torch.stack([torch.stack([torch.cos(yaw), torch.zeros(N), torch.sin(yaw)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                       torch.stack([-torch.sin(yaw), torch.zeros(N), torch.cos(yaw)], -1)], -2)
    return loc, dim, rot


def rays(W, cameras=((0.0, 0.0, 0.0),), away=False):
    """Pinhole cameras without rotation: positions [V,3], directions [V*H*W,3] (row-major pixels, integer centres)."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.stack([(x - (W - 1) / 2) / FOCAL, (y - (H - 1) / 2) / FOCAL, torch.full_like(x, -1.0 if away else 1.0)], -1)
    d = torch.nn.functional.normalize(d, dim=-1).reshape(-1, 3)
    return torch.tensor(cameras, dtype=torch.float32), d.repeat(len(cameras), 1).contiguous()


def uniforms(W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(H * W, S, generator=g), torch.rand(H * W, S, generator=g)


def pointer(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_masks(dev, instances, W, cam, dirs, mlp=None, u=None, targets=None, columns=None, view=0, soft=True, header=None, frames=None, out=None,
              flags=0, stream_offset=0, seed=0, stride=None, trace=TRACE, num_samples=S, capacity=None, height=None):
    """One vsrd_frame_masks call -> (code, dict of outputs).  `out`: pre-made output tensors (batches); else sentinel-filled ones."""
    rows = H if height is None else height
    from vsrd_amd import _lib
    lib = _lib.load()
    N = int(instances.shape[0]) if capacity is None else capacity
    V = int(cam.shape[0])
    field = _lib.Field(N, T, instances.data_ptr(), None if mlp is None else mlp.data_ptr())
    config = _lib.make_config(0, num_samples, RANGE, STD, RATIO, 1.0e-6, 3, seed=seed, stream_offset=stream_offset, flags=flags, frames=frames)
    masks = _lib.FrameMasksConfig(view, V, rows, W, trace[0], trace[1], trace[2], THRESHOLD, N if stride is None else stride)
    if out is None:
        out = dict(inside=torch.full((N, rows, (W + 7) // 8 + 3), SENTINEL, dtype=torch.uint8, device=dev)[:, :, :(W + 7) // 8].contiguous(),
                   soft=torch.full((rows * W, N), float("nan"), device=dev) if soft else None,
                   counts=torch.full((N, 3), -7, dtype=torch.int32, device=dev) if targets is not None else None)
    code = lib.vsrd_frame_masks(field, config, masks, pointer(cam), pointer(dirs), pointer(None if u is None else u[0]), pointer(None if u is None else u[1]),
                                pointer(targets), pointer(columns), pointer(out["inside"]), pointer(out["soft"]), pointer(out["counts"]),
                                pointer(header), _lib.stream())
    return code, out


def packed(soft, N, W):
    """numpy.packbits of (soft > threshold) as [N,H,ceil(W/8)]."""
    bits = (soft.reshape(H, W, N).permute(2, 0, 1) > THRESHOLD).cpu().numpy()
    return np.packbits(bits, axis=-1)


def instances_of(dev, N):
    from vsrd_amd import fields
    loc, dim, rot = scene(N)
    return fields.pack_instances(loc, rot, dim).to(dev)


@pytest.mark.parametrize("W", [64, 70, 72, 136])
def test_bits_are_packbits_of_soft_over_widths(dev, W):
    """One full run; a tail with a partial byte; a tail of one whole byte; two runs and a tail with a row stride that is no multiple of 8."""
    N = 3
    cam, dirs = (t.to(dev) for t in rays(W))
    u = [t.to(dev) for t in uniforms(W)]
    row_bytes = (W + 7) // 8
    big = torch.full((N + 1, H, row_bytes), SENTINEL, dtype=torch.uint8, device=dev)          # one plane more than the call may write
    out = dict(inside=big, soft=torch.full((H * W + 5, N), float("nan"), device=dev), counts=None)
    code, out = run_masks(dev, instances_of(dev, N), W, cam, dirs, u=u, out=out)
    assert code == 0
    torch.cuda.synchronize()
    soft = out["soft"][:H * W]
    assert torch.isfinite(soft).all() and torch.isnan(out["soft"][H * W:]).all()
    inside = big[:N].cpu().numpy()
    assert np.array_equal(inside, packed(soft, N, W))
    assert (big[N] == SENTINEL).all()
    if W % 8:
        assert not (inside[:, :, -1] & ((1 << (8 - W % 8)) - 1)).any()                        # pad bits
    hit = (soft > THRESHOLD).any(-1)
    assert 0 < int(hit.sum()) < H * W                                                         # some pixels hit, some miss
    assert int(((soft[:, 0] > THRESHOLD) | (soft[:, 1] > THRESHOLD)).sum()) > 0
    assert (soft[~(soft != 0).any(-1)] == 0).all()


def reference_entry_points(dev, instances, mlp, cam, dirs, view, W, u, flags=0, stream_offset=0, seed=0, weights=False):
    """converged, |sdf| at the traced position and labels of the view's rays from vsrd_sphere_trace, vsrd_field_eval and vsrd_render_hierarchical_forward."""
    from vsrd_amd import _lib
    lib = _lib.load()
    N, R = int(instances.shape[0]), H * W
    field = _lib.Field(N, T, instances.data_ptr(), None if mlp is None else mlp.data_ptr())
    origin = cam[view].contiguous()
    d = dirs[view * R:(view + 1) * R].contiguous()
    positions, converged = torch.empty(R, 3, device=dev), torch.empty(R, dtype=torch.uint8, device=dev)
    _lib.check(lib.vsrd_sphere_trace(field, pointer(origin), 0, pointer(d), None, R, TRACE[0], TRACE[1], TRACE[2], 0, 0, pointer(positions),
                                     pointer(converged), _lib.stream()))
    sdf = torch.empty(R, device=dev)
    _lib.check(lib.vsrd_field_eval(field, pointer(positions), R, pointer(sdf), None, None, 0, _lib.stream()))
    config = _lib.make_config(R, S, RANGE, STD, RATIO, 1.0e-6, 0, seed=seed, stream_offset=stream_offset, flags=flags)
    labels = torch.empty(R, N, device=dev)
    w = torch.empty(R, 2 * S - 1, device=dev) if weights else None
    _lib.check(lib.vsrd_render_hierarchical_forward(field, config, pointer(origin), pointer(d), pointer(None if u is None else u[0]),
                                                    pointer(None if u is None else u[1]), pointer(labels), None, None, pointer(w), None, None, None, _lib.stream()))
    torch.cuda.synchronize()
    return converged.bool(), sdf.abs(), labels


@pytest.mark.parametrize("residual", [False, True])
def test_against_the_existing_entry_points(dev, residual, golden):
    W = 70
    N = 2 if residual else 3
    instances = instances_of(dev, N)
    mlp = golden("g10_render_residual_n3_s16")["mlp_weights"][:N].contiguous().to(dev) if residual else None
    cam, dirs = (t.to(dev) for t in rays(W))
    u = [t.to(dev) for t in uniforms(W)]
    code, out = run_masks(dev, instances, W, cam, dirs, mlp=mlp, u=u)
    assert code == 0
    converged, sdf, labels = reference_entry_points(dev, instances, mlp, cam, dirs, 0, W, u)
    soft = out["soft"]
    mine = (soft != 0).any(-1) | converged & (labels == 0).all(-1)            # (a converged pixel whose labels are all exactly 0 shows no trace in soft)
    borderline = (sdf - TRACE[1]).abs() <= 1.0e-4 * TRACE[1]
    disagree = mine != converged
    print(f"converged {int(converged.sum())} of {H * W}, disagreeing {int(disagree.sum())}, borderline {int(borderline.sum())}")
    assert not (disagree & ~borderline).any()
    assert int(borderline.sum()) <= 0.01 * H * W
    keep = ~borderline
    want = labels * converged[:, None]
    error = (soft - want).abs()[keep].max()
    print(f"max |soft - labels x converged| = {float(error):.3e}")
    assert error < LABEL_TOL
    assert 0 < int(converged.sum()) < H * W


def oracle_trace(union, origin, directions):
    """sphere_tracing(initialization=False, differentiable=False) in float64 (renderers.py:21-59) without its batch-wide exit (oracle.tracing)
    -> converged, borderline: a decision anywhere along the ray's path within 1e-4 relative of its threshold."""
    out = otracing.trace(union.distance, origin, directions, TRACE[0], TRACE[1], bounding_radius=TRACE[2], initialise=False, early_exit=False)
    return out.converged, otracing.borderline(out, TRACE[1], TRACE[2])


def test_against_the_float64_oracle(dev):
    W, N = 70, 3
    loc, dim, rot = (t.double() for t in scene(N))
    union = ofields.InstanceUnion(loc, rot, dim, T)
    cam, dirs = rays(W)
    u = uniforms(W)
    origin = cam[0].double()
    with torch.no_grad():
        converged, borderline = oracle_trace(union, origin, dirs.double())
        labels = orendering.hierarchical_render(union, origin.expand(H * W, 3), dirs.double(), RANGE, S, STD, RATIO, u[0].double(), u[1].double()).labels
    want = labels * converged[:, None]
    code, out = run_masks(dev, instances_of(dev, N), W, cam.to(dev), dirs.to(dev), u=[t.to(dev) for t in u])
    assert code == 0
    torch.cuda.synchronize()
    soft = out["soft"].cpu().double()
    mine = (soft != 0).any(-1) | converged & (want == 0).all(-1)
    assert not ((mine != converged) & ~borderline).any()
    assert int(borderline.sum()) <= 0.01 * H * W
    agreed = mine == converged
    error = (soft - want).abs()[agreed].max()
    print(f"max |soft - oracle| = {float(error):.3e} over {int(agreed.sum())} pixels, {int(converged.sum())} converged")
    assert error < LABEL_TOL
    decided = ((want - THRESHOLD).abs() > LABEL_TOL) & agreed[:, None]
    bits = torch.from_numpy(np.unpackbits(out["inside"].cpu().numpy(), axis=-1)[:, :, :W]).bool().permute(1, 2, 0).reshape(H * W, N)
    assert torch.equal(bits[decided], (want > THRESHOLD)[decided])


def test_grazing_rays_against_the_reference(dev):
    """G19's T = 0.3 rays (tests/golden/make_golden.py: rays that converge at a rim, step past it and un-converge) as an 8 x 125 image:
    where the trace phase converged -- soft's zero pattern, and no bit outside it -- against the reference's own convergence masks, and the
    labels against the float64 oracle, off the borderline set.  A trace that stops at the first convergence fails here on the
    discriminating rays."""
    g = load_golden("g19_sphere_tracing_grazing")
    height, W, N = 8, 125, 3
    dirs, want_converged, flagged = g["directions"][0], g["convergence_masks"][0], g["discriminating"][0]
    loc, dim, rot = g["locations"], g["dimensions"], g["orientations"]
    union = ofields.InstanceUnion(loc.double(), rot.double(), dim.double(), T)
    origin = torch.zeros(3, dtype=torch.float64)
    gen = torch.Generator().manual_seed(19)
    u = torch.rand(height * W, S, generator=gen), torch.rand(height * W, S, generator=gen)
    with torch.no_grad():
        converged, borderline = oracle_trace(union, origin, dirs.double())
        labels = orendering.hierarchical_render(union, origin.expand(height * W, 3), dirs.double(), RANGE, S, STD, RATIO, u[0].double(), u[1].double()).labels
    keep = ~borderline
    assert int(borderline.sum()) <= 0.01 * height * W
    assert torch.equal(converged[keep], want_converged[keep])                      # the oracle is the reference here
    from vsrd_amd import fields
    instances = fields.pack_instances(loc, rot, dim).to(dev)
    code, out = run_masks(dev, instances, W, torch.zeros(1, 3, device=dev), dirs.to(dev).contiguous(), u=[t.to(dev) for t in u], height=height)
    assert code == 0
    torch.cuda.synchronize()
    soft = out["soft"].cpu().double()
    want = labels * want_converged[:, None]
    mine = (soft != 0).any(-1) | want_converged & (want == 0).all(-1)
    wrong = (mine != want_converged) & keep
    print(f"converged {int(want_converged.sum())} of {height * W}, discriminating {int(flagged.sum())}, borderline {int(borderline.sum())}, wrong {int(wrong.sum())}")
    assert not wrong.any(), torch.nonzero(wrong)[:, 0].tolist()
    assert int((flagged & keep).sum()) >= 16
    bits = torch.from_numpy(np.unpackbits(out["inside"].cpu().numpy(), axis=-1)[:, :, :W]).bool().permute(1, 2, 0).reshape(height * W, N)
    assert not (bits.any(-1) & ~want_converged & keep).any()                       # no bit where the reference did not converge
    agreed = mine == want_converged
    error = (soft - want).abs()[agreed].max()
    print(f"max |soft - oracle| = {float(error):.3e} over {int(agreed.sum())} pixels")
    assert error < LABEL_TOL
    decided = ((want - THRESHOLD).abs() > LABEL_TOL) & agreed[:, None]
    assert torch.equal(bits[decided], (want > THRESHOLD)[decided])


def test_counts_and_mask_iou(dev):
    from vsrd_amd import optimization
    W, N, stride = 136, 3, 5
    cam, dirs = (t.to(dev) for t in rays(W))
    u = [t.to(dev) for t in uniforms(W)]
    g = torch.Generator().manual_seed(3)
    targets = torch.rand(H * W, stride, generator=g).to(dev)
    columns = torch.tensor([4, 0, 2], dtype=torch.int32, device=dev)
    code, out = run_masks(dev, instances_of(dev, N), W, cam, dirs, u=u, targets=targets, columns=columns, stride=stride)
    assert code == 0
    torch.cuda.synchronize()
    pred = torch.from_numpy(np.unpackbits(out["inside"].cpu().numpy(), axis=-1)[:, :, :W]).bool().reshape(N, H * W).to(dev)
    target = (targets[:, columns.long()] > THRESHOLD).t()
    want = torch.stack([pred.sum(-1), target.sum(-1), (pred & target).sum(-1)], -1).to(torch.int32)
    assert torch.equal(out["counts"], want)
    assert int(want[:, 2].sum()) > 0
    iou = optimization.mask_iou(out["counts"])
    assert torch.allclose(iou, want[:, 2].float() / (want[:, 0] + want[:, 1] - want[:, 2]).float())


def test_batch_with_headers_equals_each_frame_alone(dev):
    """B = 2 rows of capacity 4 with n_f = (3, 2), view 1 of V_cap = 2: every output of frame f is bit-identical to the call on frame f alone
    with N = n_f, and nothing of instances n_f .. 3 is touched."""
    from vsrd_amd import _lib
    W, cap, B, counts_f = 70, 4, 2, (3, 2)
    cam, dirs = rays(W, cameras=((0.0, 0.0, 0.0), (0.5, 0.0, -1.0)))
    R, row_bytes = H * W, (W + 7) // 8
    g = torch.Generator().manual_seed(5)
    layout, at = {}, 0
    for name, nbytes in (("instances", cap * 64), ("cam", 24), ("dirs", 2 * R * 12), ("uc", R * S * 4), ("uf", R * S * 4), ("targets", 2 * R * cap * 4),
                         ("columns", cap * 4), ("inside", cap * H * row_bytes), ("soft", R * cap * 4), ("counts", cap * 12), ("header", 24)):
        layout[name] = (at, nbytes)
        at = (at + nbytes + 255) // 256 * 256
    arena = torch.full((B, at), SENTINEL, dtype=torch.uint8, device=dev)

    def view(f, name, dtype, shape):
        offset, nbytes = layout[name]
        return arena[f, offset:offset + nbytes].view(dtype).view(shape)
    frames = []
    for f, n in enumerate(counts_f):
        instances = instances_of(dev, n)
        if f == 1:
            instances[:, 0] += 0.7
        uc, uf = (t.to(dev) for t in uniforms(W, seed=10 + f))
        targets = torch.rand(2 * R, cap, generator=g).to(dev)
        columns = torch.randperm(n, generator=g).to(torch.int32).to(dev)
        view(f, "instances", torch.float32, (cap, 16))[:n] = instances
        view(f, "cam", torch.float32, (2, 3)).copy_(cam)
        view(f, "dirs", torch.float32, (2 * R, 3)).copy_(dirs)
        view(f, "uc", torch.float32, (R, S)).copy_(uc)
        view(f, "uf", torch.float32, (R, S)).copy_(uf)
        view(f, "targets", torch.float32, (2 * R, cap)).copy_(targets)
        view(f, "columns", torch.int32, (cap,))[:n] = columns
        header = _lib.FrameHeader(n | _lib.FRAME_HEADER_HAS_VIEWS, 0.0, 2, 0, 2 * R)
        view(f, "header", torch.uint8, (24,)).copy_(torch.frombuffer(bytearray(bytes(header)), dtype=torch.uint8))
        # the frame alone, N = n_f: its own dense tensors
        code, alone = run_masks(dev, instances, W, cam.to(dev), dirs.to(dev), u=[uc, uf], targets=targets, columns=columns, view=1, stride=cap)
        assert code == 0
        frames.append(alone)
    out = dict(inside=view(0, "inside", torch.uint8, (cap, H, row_bytes)), soft=view(0, "soft", torch.float32, (R, cap)), counts=view(0, "counts", torch.int32, (cap, 3)))
    code, _ = run_masks(dev, view(0, "instances", torch.float32, (cap, 16)), W, view(0, "cam", torch.float32, (2, 3)), view(0, "dirs", torch.float32, (2 * R, 3)),
                        u=[view(0, "uc", torch.float32, (R, S)), view(0, "uf", torch.float32, (R, S))], targets=view(0, "targets", torch.float32, (2 * R, cap)),
                        columns=view(0, "columns", torch.int32, (cap,)), view=1, header=view(0, "header", torch.uint8, (24,)), frames=(B, at), out=out, stride=cap)
    assert code == 0
    torch.cuda.synchronize()
    for f, n in enumerate(counts_f):
        inside, soft, counts = view(f, "inside", torch.uint8, (cap, H, row_bytes)), view(f, "soft", torch.float32, (R, cap)), view(f, "counts", torch.int32, (cap, 3))
        assert torch.equal(inside[:n], frames[f]["inside"])
        assert torch.equal(soft[:, :n], frames[f]["soft"])
        assert torch.equal(counts[:n], frames[f]["counts"])
        assert (inside[n:] == SENTINEL).all() and (counts[n:].view(torch.uint8) == SENTINEL).all()
        assert (soft[:, n:].contiguous().view(torch.uint8) == SENTINEL).all()
        assert int(counts[:n, 0].sum()) > 0


def test_philox_uniforms(dev):
    from vsrd_amd import _lib
    W, N = 70, 3
    instances = instances_of(dev, N)
    cam, dirs = (t.to(dev) for t in rays(W))
    offset = torch.tensor([41], dtype=torch.int64, device=dev)
    runs = [run_masks(dev, instances, W, cam, dirs, seed=9, stream_offset=offset) for _ in range(2)]
    other = run_masks(dev, instances, W, cam, dirs, seed=9, stream_offset=torch.tensor([42], dtype=torch.int64, device=dev))
    assert all(code == 0 for code, _ in (*runs, other))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][1]["inside"], runs[1][1]["inside"]) and torch.equal(runs[0][1]["soft"], runs[1][1]["soft"])
    assert not torch.equal(runs[0][1]["soft"], other[1]["soft"])
    converged, _, labels = reference_entry_points(dev, instances, None, cam, dirs, 0, W, None, seed=9, stream_offset=41, weights=True)
    soft = runs[0][1]["soft"]
    same = ((soft != 0).any(-1) | (labels == 0).all(-1)) == converged
    assert int((~same).sum()) <= 0.01 * H * W
    error = (soft - labels * converged[:, None]).abs()[same].max()
    print(f"max |soft - labels| with Philox uniforms = {float(error):.3e}")
    assert error < LABEL_TOL


def test_a_view_that_sees_no_box_renders_nothing(dev):
    W, N = 136, 3
    cam, dirs = (t.to(dev) for t in rays(W, away=True))
    targets = torch.rand(H * W, N, device=dev)
    code, out = run_masks(dev, instances_of(dev, N), W, cam, dirs, u=[t.to(dev) for t in uniforms(W)], targets=targets)
    assert code == 0
    torch.cuda.synchronize()
    assert not out["inside"].any() and not out["soft"].any() and not out["counts"][:, 0].any() and not out["counts"][:, 2].any()
    assert torch.equal(out["counts"][:, 1].long(), (targets > THRESHOLD).sum(0))


def test_argument_validation(dev):
    """Every VSRD_E_INVALID_ARGUMENT case of the header; none launches anything: the sentinel-filled outputs stay as they are."""
    from vsrd_amd import _lib
    lib = _lib.load()
    W, N = 64, 3
    instances = instances_of(dev, N)
    mlp = torch.zeros(N, _lib.MLP_WEIGHTS, device=dev)
    cam, dirs = (t.to(dev) for t in rays(W))
    targets = torch.rand(H * W, N, device=dev)
    columns = torch.arange(N, dtype=torch.int32, device=dev)
    bad = []
    bad.append(run_masks(dev, instances, W, cam, dirs, view=1))                                  # view >= V
    bad.append(run_masks(dev, instances, W, cam, dirs, view=-1))
    bad.append(run_masks(dev, instances, W, cam, dirs, capacity=0))                              # N outside 1..64
    bad.append(run_masks(dev, instances, W, cam, dirs, capacity=_lib.MAX_INSTANCES + 1))
    bad.append(run_masks(dev, instances, W, cam, dirs, num_samples=1))                           # S outside what the one-ray kernel serves
    bad.append(run_masks(dev, instances, W, cam, dirs, num_samples=257))
    bad.append(run_masks(dev, instances, W, cam, dirs, mlp=mlp, num_samples=129))
    out = dict(inside=torch.full((N, H, 8), SENTINEL, dtype=torch.uint8, device=dev), soft=None, counts=None)
    bad.append(run_masks(dev, instances, W, cam, dirs, targets=targets, out=out))                # targets without counts
    out = dict(inside=torch.full((N, H, 8), SENTINEL, dtype=torch.uint8, device=dev), soft=None, counts=torch.full((N, 3), -7, dtype=torch.int32, device=dev))
    bad.append(run_masks(dev, instances, W, cam, dirs, out=out))                                 # counts without targets
    torch.cuda.synchronize()
    for code, out in bad:
        assert code == _lib.E_INVALID_ARGUMENT
        assert (out["inside"] == SENTINEL).all()
        assert out["counts"] is None or (out["counts"] == -7).all()
    # members of the render config that belong to the step entry points
    field = _lib.Field(N, T, instances.data_ptr(), None)
    masks = _lib.FrameMasksConfig(0, 1, H, W, *TRACE, THRESHOLD, N)
    inside = torch.full((N, H, 8), SENTINEL, dtype=torch.uint8, device=dev)
    indices = torch.zeros(H * W, dtype=torch.int64, device=dev)
    scratch = torch.zeros(H * W, 2 * S, device=dev)
    for change in (dict(gather=(indices, H * W, None, 0)), dict(gather=(None, 0, columns, N)), dict(samples=(scratch, None, None, None)),
                   dict(samples=(None, None, scratch, None))):
        config = _lib.make_config(H * W, S, RANGE, STD, RATIO, 1.0e-6, 3, **change)
        code = lib.vsrd_frame_masks(field, config, masks, pointer(cam), pointer(dirs), None, None, None, None, pointer(inside), None, None, None, _lib.stream())
        assert code == _lib.E_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (inside == SENTINEL).all()
    # ... and num_rays is ignored
    config = _lib.make_config(-5, S, RANGE, STD, RATIO, 1.0e-6, 3)
    assert lib.vsrd_frame_masks(field, config, masks, pointer(cam), pointer(dirs), None, None, None, None, pointer(inside), None, None, None, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert not (inside == SENTINEL).all()


def test_frame_batch_masks_equal_each_frame_alone_and_leave_the_trajectory(dev):
    from vsrd_amd import launcher, optimization
    size = (47, 176)
    inputs = [launcher.synthetic_frame_inputs(dev, 3, 2, 3, *size), launcher.synthetic_frame_inputs(dev, 4, 2, 2, *size)]
    config = optimization.OptimizationConfig(num_samples=40, num_rays=64, warmup_steps=2, num_steps=12, seed=3, mlp_adjoint_item_slots=8,
                                             surface_num_iterations=64)

    def parameters(loop):
        return [t.detach().clone() for t in (loop.detector.locations, loop.detector.dimensions, loop.detector.orientations, loop.detector.embeddings)]
    alone, untouched = [], []
    for k, frame in enumerate(inputs):
        for with_masks in (True, False):
            loop = optimization.FrameOptimizer(frame, dataclasses.replace(config, init_seed=70 + k), dev, graph=True, persistent=True)
            if with_masks:
                with pytest.raises(RuntimeError, match="no step has run"):
                    loop.masks()
            loop.run(3, steps_per_graph=1)
            if with_masks:
                alone.append({key: value.clone() if isinstance(value, torch.Tensor) else value for key, value in loop.masks(soft=True).items()})
            loop.run(1, steps_per_graph=1)
            torch.cuda.synchronize()
            if with_masks:
                alone[-1]["after"] = parameters(loop)
            else:
                untouched.append(parameters(loop))
            if with_masks:
                assert loop.reset(frame, init_seed=70 + k)
                with pytest.raises(RuntimeError, match="no step has run"):
                    loop.masks()
            loop.close()
    for with_masks, without in zip(alone, untouched):                 # masks() leaves the trajectory bit-identical
        assert all(torch.equal(a, b) for a, b in zip(with_masks["after"], without))
    batch = optimization.FrameBatch(inputs, config, dev, init_seeds=[70, 71], max_instances=3)
    with pytest.raises(RuntimeError, match="no step has run"):
        batch.masks()
    batch.run(3, steps_per_graph=1)
    got = batch.masks(soft=True)
    torch.cuda.synchronize()
    for k, (mine, want) in enumerate(zip(got, alone)):
        n = inputs[k].soft_masks.shape[-1]
        assert mine["inside"].shape == (n, size[0], (size[1] + 7) // 8) and mine["counts"].shape == (n, 3) and mine["soft"].shape == (*size, n)
        for key in ("inside", "counts", "mask_iou", "soft"):
            assert torch.equal(mine[key], want[key]), (k, key)
        assert int(mine["counts"][:, 1].sum()) > 0
    batch.run(1, steps_per_graph=1)
    torch.cuda.synchronize()
    for k, member in enumerate(batch.frames):
        assert all(torch.equal(a, b) for a, b in zip(parameters(member), untouched[k]))
    assert batch.reset(0, inputs[0], init_seed=70)
    with pytest.raises(RuntimeError, match="no step has run"):
        batch.masks()
    batch.close()
