"""The photometric term in the frame loop (vsrd_amd/optimization.py; scripts/main.py:689-853): the eager loop's autograd composition against
the captured fused-glue loop's vsrd_frame_photometric, the weight-0 trajectory, the in-graph draw, reset() of a persistent slot.

The scene is that of tests/test_hip_step.py::test_graph_mode_replays_the_same_steps -- V = 3, 128 x 128, N = 4, S = 32, R = 256 -- with
smooth images, warmup_steps = 2 and 48 photometric rays (k = 3: the term needs top_k <= V).  The parity runs supply the term's rays: the 48
pixels of the target view whose rays end farthest from every place where the hard union's normal jumps, judged on the CPU with the float64
oracle at the start parameters -- the edges of the hit box (the gap between its two largest q = |local| - half extent, on the surface and
0.3 m behind it, where the residual phase's surface lies), the fold plane local x = 0 of the residual MLP and the hard arg-min switch.  No
supplied ray may end within KINK of one; none is excluded afterwards.
"""
import dataclasses
import functools
import math

import pytest
import torch

import patch_correlation_reference as pcr
from conftest import margin
from oracle import fields as ofields, geometry as ogeometry

pytestmark = pytest.mark.gpu

V, H, W, N, S, R = 3, 128, 128, 4, 32, 256
RAYS, TOP_K, PATCH = 48, 3, (11, 11)
WARMUP = 2
KINK = 1e-3
WEIGHT = 0.05
# tests/test_hip_frame_photometric.py: three times the float32 chain's own distance from the float64 chain (test_hip_field_normals.py: 1.4e-4)
GRADIENT_BOUND = 3.0 * 1.4e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def c1_frame():
    """The cameras, ground-truth boxes, their 2-D boxes and visibility of tests/test_hip_step.py's frame (seed 0)."""
    g = torch.Generator().manual_seed(0)
    sx, sy = W / 1408.0, H / 376.0
    K = torch.tensor([[552.554261 * sx, 0.0, 682.049453 * sx], [0.0, 552.554261 * sy, 238.769549 * sy], [0.0, 0.0, 1.0]]).expand(V, 3, 3).contiguous()
    E = torch.eye(4).repeat(V, 1, 1)
    for v, k in enumerate([0, 1, -1][:V]):
        yaw = math.radians(0.5 * k)
        E[v, :3, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
        E[v, 2, 3] = 1.0 * k
    raw_loc = torch.randn(N, 3, generator=g) * 0.3
    raw_loc[:, 2] = torch.empty(N).uniform_(-2.2, -1.2, generator=g)
    raw_dim = torch.randn(N, 3, generator=g) * 0.5
    raw_ori = torch.nn.functional.normalize(torch.randn(N, 2, generator=g), dim=-1)
    loc, dim, rot, corners = ogeometry.decode_box_parameters(raw_loc, raw_dim, raw_ori)
    gt_boxes, _ = ogeometry.project_boxes_multi_view(corners, E, K, (H, W))
    visible = torch.ones(V, N, dtype=torch.bool)
    visible[2, 3] = False
    return K, E, (loc, dim, rot), gt_boxes * visible[..., None, None], visible


def start_parameters():
    g = torch.Generator().manual_seed(4)
    start = [torch.randn(N, 3, generator=g) * 0.2, torch.randn(N, 3, generator=g) * 0.2,
             torch.nn.functional.normalize(torch.tensor([1.0, 0.0]) + torch.randn(N, 2, generator=g) * 0.2, dim=-1)]
    start[0][:, 2] -= 1.5
    return start


def kink_distance(union, points):
    """[P] float64: the distance of each point from the nearest jump of the hard union's normal (see the module's docstring)."""
    local = torch.einsum("npk,nkj->npj", points[None] - union.locations[:, None], union.orientations)
    q = local.abs() - union.dimensions[:, None]
    d, _ = union.instance_terms(points)
    member = d.argmin(0)
    top = q.topk(2, dim=-1).values
    edge = (top[..., 0] - top[..., 1]).gather(0, member[None])[0]
    fold = local[..., 0].abs().gather(0, member[None])[0]
    low = d.topk(2, dim=0, largest=False).values
    return torch.minimum(torch.minimum(edge, fold), low[1] - low[0])


@functools.lru_cache(maxsize=None)
def surface_rays():
    """(indices [RAYS] int64, their smallest kink distance): the rays of the target view that hit the START boxes farthest from a kink."""
    K = c1_frame()[0][0].double()
    loc, dim, rot, _ = ogeometry.decode_box_parameters(*[s.double() for s in start_parameters()])
    union = ofields.InstanceUnion(loc, rot, dim, 0.4)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pixels = torch.stack([x.reshape(-1), y.reshape(-1)], -1)
    r = torch.nn.functional.normalize((torch.linalg.inv(K) @ torch.nn.functional.pad(pixels.double(), (0, 1), value=1.0).T).T, dim=-1)
    p = torch.zeros_like(r)
    for _ in range(100):
        p = p + r * union.union_distance(p, hard=True)[:, None]
    usable = union.union_distance(p, hard=True).abs() < 1e-3
    usable &= (pixels[:, 0] >= 12) & (pixels[:, 0] <= W - 13) & (pixels[:, 1] >= 12) & (pixels[:, 1] <= H - 13)
    score = torch.minimum(kink_distance(union, p), kink_distance(union, p + 0.3 * r))
    best = torch.where(usable, score, torch.full_like(score, -1.0)).topk(RAYS)
    return best.indices.sort().values, float(best.values.min())


_frames = {}


def frame(dev, seed=400):
    """The FrameInputs of the scene (made once per image seed): soft masks rendered from the ground-truth boxes, smooth images."""
    if seed not in _frames:
        from vsrd_amd import optimization, rendering, fields
        K, E, (loc, dim, rot), gt_boxes, visible = c1_frame()
        cam, dirs = rendering.ray_casting((H, W), K.to(dev), E.to(dev))
        block = fields.FieldBlock(fields.pack_instances(loc.to(dev), rot.to(dev), dim.to(dev)), 0.1, None, None)
        origins = cam[:, None, None, :].expand(V, H, W, 3).reshape(-1, 3).contiguous()
        soft = rendering.render_hierarchical(block, origins, dirs.reshape(-1, 3), (0.0, 100.0), S, 0.1, 1.0, seed=5)["labels"].clamp(0, 1)
        soft = (soft.reshape(V, H, W, N) * visible.to(dev)[:, None, None, :]).contiguous()
        images = pcr.smooth_images(torch.Generator().manual_seed(seed), V, H, W).to(dev)
        _frames[seed] = optimization.FrameInputs((H, W), K.to(dev), E.to(dev), soft, gt_boxes.to(dev), visible.to(dev), images=images)
    return _frames[seed]


def config(weight=WEIGHT, warmup=WARMUP, **changes):
    from vsrd_amd import losses, optimization
    return optimization.OptimizationConfig(num_samples=S, num_rays=R, warmup_steps=warmup, num_steps=3000, surface_num_rays=RAYS, surface_top_k=TOP_K,
                                           surface_patch_size=PATCH, surface_num_iterations=100, surface_convergence_criteria=1e-3,
                                           loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": weight}, **changes)


def new_loop(dev, inputs, cfg, **how):
    from vsrd_amd import optimization
    torch.manual_seed(0)
    loop = optimization.FrameOptimizer(inputs, cfg, dev, **how)
    with torch.no_grad():
        for p, v in zip((loop.detector.locations, loop.detector.dimensions, loop.detector.orientations), start_parameters()):
            p.copy_(v[None].to(dev))
    return loop


def tensors(loop):
    params = list(loop.detector.parameters()) + list(loop.hyper_distance_field.parameters())
    moments = [[loop.optimizer.state[p][k] for k in ("exp_avg", "exp_avg_sq", "step")] if loop.optimizer.state.get(p) else None for p in params]
    return params, moments


def synchronise(source, target):
    with torch.no_grad():
        (pe, me), (pg, mg) = tensors(source), tensors(target)
        for a, b in zip(pe, pg):
            b.copy_(a)
        for a, b in zip(me, mg):
            if a is not None and b is not None:
                b[0].copy_(a[0]), b[1].copy_(a[1])


def state_bits(loop):
    params, moments = tensors(loop)
    out = [p.detach().clone() for p in params]
    for m in moments:
        out += [] if m is None else [t.detach().clone() for t in m]
    out.append(loop._glue["record"].clone())
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def step_rays(dev, inputs):
    weights = inputs.soft_masks.reshape(-1, N).max(-1).values
    return torch.multinomial((weights > 0.5).float(), R, replacement=False)


# ---- 1: the supplied rays -----------------------------------------------------------------------------------------------------------------
def test_supplied_rays_stay_away_from_every_kink():
    indices, closest = surface_rays()
    print(f"test_supplied_rays_stay_away_from_every_kink: the closest of {RAYS} rays ends {closest:.4f} m from a kink")
    assert indices.numel() == RAYS and indices.unique().numel() == RAYS
    assert closest >= KINK


# ---- 2: eager against the captured fused loop ----------------------------------------------------------------------------------------------
def test_graph_loop_walks_the_eager_loops_steps(dev):
    """Two box-only and four residual steps, parameters and moments synchronised before every step, the step's and the term's rays given."""
    inputs, cfg = frame(dev), config()
    surface = surface_rays()[0].to(dev)
    eager_loop, graph_loop = new_loop(dev, inputs, cfg), new_loop(dev, inputs, cfg, graph=True)
    graph_loop.hyper_distance_field.load_state_dict(eager_loop.hyper_distance_field.state_dict())
    with torch.no_grad():
        graph_loop.detector.embeddings.copy_(eager_loop.detector.embeddings)
    errors = []
    for step in range(WARMUP + 4):
        rays = step_rays(dev, inputs)
        synchronise(eager_loop, graph_loop)
        eager, replayed = eager_loop.step(rays, surface_ray_indices=surface), graph_loop.step(rays, surface_ray_indices=surface)
        residual = step >= WARMUP
        assert ("photometric_loss" in eager) == residual and ("photometric_loss" in replayed) == residual, step
        for key in ("silhouette_loss", "iou_projection_loss", "l1_projection_loss", "loss") + (("photometric_loss",) if residual else ()):
            print(f"test_graph_loop_walks_the_eager_loops_steps: step {step} {key:20s} eager {float(eager[key]):.7f} graph {float(replayed[key]):.7f}")
            torch.testing.assert_close(replayed[key], eager[key], rtol=1e-4, atol=1e-6, msg=lambda m: f"step {step} {key}: {m}")
        if residual:
            assert 0.0 < float(replayed["photometric_loss"]) < 1.0
        worst = max(float((a - b).abs().max()) / max(float(a.abs().max()), 1e-6) for a, b in zip(eager["raw_gradients"], replayed["raw_gradients"]))
        margin("test_graph_loop_walks_the_eager_loops_steps", "raw gradients, " + ("residual step (informative)" if residual else "box-only step"), worst,
               1.0 if residual else 1e-3)
        print(f"test_graph_loop_walks_the_eager_loops_steps: step {step} raw gradients {worst:.3e}")
        assert worst <= (0.5 if residual else 1e-3), step        # (held as test_graph_mode_replays_the_same_steps holds its residual steps)
        if residual:
            errors.append(worst)
    margin("test_graph_loop_walks_the_eager_loops_steps", "raw gradients, median residual step", sorted(errors)[len(errors) // 2], 1e-4)
    assert sorted(errors)[len(errors) // 2] <= 1e-4 and sum(e > 1e-3 for e in errors) <= 2, errors
    assert graph_loop.step_index == WARMUP + 4 and int(graph_loop.step_tensor) == WARMUP + 4
    eager_loop.close(), graph_loop.close()


# ---- 3: the row after a step is enough to recompute the term ----------------------------------------------------------------------------------
def test_the_rows_buffers_reproduce_the_term(dev):
    from vsrd_amd import fields, losses, rendering
    inputs, cfg = frame(dev), config()
    surface = surface_rays()[0].to(dev)
    loop = new_loop(dev, inputs, cfg, graph=True)
    for _ in range(WARMUP + 1):
        out = loop.step(surface_ray_indices=surface)
    torch.cuda.synchronize()
    b, p = loop._glue, loop._photometric
    instances = b["instances"][:N].clone().requires_grad_(True)
    block = fields.FieldBlock(instances, 1.0, b["mlp_centred"][:N].clone(), None, hard=True)
    positions, converged = rendering.sphere_tracing(block, loop.camera_positions[0], loop.ray_directions[surface], 100, 1e-3, bounding_radius=100.0,
                                                    initialization=False, differentiable=True)
    normals = rendering.surface_normal(block, positions)
    loss = losses.patch_correlation_loss(p["gray"][:V], inputs.intrinsic_matrices, inputs.extrinsic_matrices, surface, positions, normals, converged, PATCH, TOP_K)
    loss.backward()
    # (the freshly drawn hypernetwork's residual, sigmoid(MLP - 1), pulls the surface deep into the boxes: only the rays through their middles converge)
    print(f"test_the_rows_buffers_reproduce_the_term: {int(converged.sum())} of {RAYS} rays converge, loss {float(loss.detach()):.7f}")
    assert int(converged.sum()) >= 1
    assert same_bits(out["photometric_loss"].reshape(1), loss.detach().reshape(1)), (float(out["photometric_loss"]), float(loss))
    distance = float((p["grad_instances"][:N] - instances.grad).abs().max() / instances.grad.abs().max())
    margin("test_the_rows_buffers_reproduce_the_term", "grad instances / max", distance, GRADIENT_BOUND)
    print(f"test_the_rows_buffers_reproduce_the_term: grad instances / max {distance:.3e} (bound {GRADIENT_BOUND:.3e})")
    assert distance <= GRADIENT_BOUND
    loop.close()


# ---- 4: weight 0 is today's trajectory, bit for bit ---------------------------------------------------------------------------------------------
def test_weight_zero_walks_the_trajectory_without_images(dev):
    with_images = frame(dev)
    without = dataclasses.replace(with_images, images=None)
    assert without.images is None and with_images.images is not None
    loops = [new_loop(dev, inputs, config(weight=0.0), graph=True) for inputs in (with_images, without)]
    assert all(loop._photometric is None for loop in loops)
    for step in range(WARMUP + 4):
        results = [loop.step() for loop in loops]
        torch.cuda.synchronize()
        assert "photometric_loss" not in results[0]
        for a, b in zip(state_bits(loops[0]), state_bits(loops[1])):
            assert same_bits(a, b), step
    for loop in loops:
        loop.close()


# ---- 5: the in-graph draw; the term moves the boxes ------------------------------------------------------------------------------------------
def test_in_graph_draw_and_the_terms_pull(dev):
    inputs = frame(dev)
    hard = (inputs.soft_masks[0].amax(-1) > 0.5).reshape(-1)
    # two loops that draw the term's rays in the graph; for the pull, one with the term at the silhouette's weight on the supplied rays (which
    # hit the start boxes) and one without the term -- the four start alike and draw the step's own rays from the same stream
    loops = [new_loop(dev, inputs, config(), graph=True) for _ in range(2)]
    loops += [new_loop(dev, inputs, config(weight=1.0), graph=True), new_loop(dev, inputs, config(weight=0.0), graph=True)]
    surface = surface_rays()[0].to(dev)
    for loop in loops[1:]:
        loop.hyper_distance_field.load_state_dict(loops[0].hyper_distance_field.state_dict())
    with torch.no_grad():
        for loop in loops[1:]:
            loop.detector.embeddings.copy_(loops[0].detector.embeddings)
    drawn = []
    for step in range(WARMUP + 4):
        results = [loop.step(surface_ray_indices=surface) if loop is loops[2] and step >= WARMUP else loop.step() for loop in loops]
        torch.cuda.synchronize()
        if step >= WARMUP:
            picks = [loop._photometric["ray_indices"].clone() for loop in loops[:2]]
            assert torch.equal(picks[0], picks[1]), step                                   # the same seed draws the same rays
            assert picks[0].unique().numel() == RAYS and bool(hard[picks[0]].all()), step   # distinct, inside the hard-mask union
            drawn.append(picks[0])
            for a, b in zip(state_bits(loops[0]), state_bits(loops[1])):
                assert same_bits(a, b), step
        if step == WARMUP:          # the first residual step: the same start, with and without the term
            with_term, without = results[2]["raw_gradients"][2], results[3]["raw_gradients"][2]
            apart = float((with_term - without).abs().max() / without.abs().max())
            print(f"test_in_graph_draw_and_the_terms_pull: the orientations' gradient moves by {apart:.3e} of its largest entry with the term")
            assert apart > 10.0 * GRADIENT_BOUND
            assert float(results[2]["loss"]) != float(results[3]["loss"])
    assert all(not torch.equal(drawn[0], other) for other in drawn[1:])                     # they change from step to step
    for loop in loops:
        loop.close()


# ---- 6: a persistent slot takes another frame's images without a capture -----------------------------------------------------------------------
def test_reset_to_a_frame_with_other_images(dev):
    first, second = frame(dev, 400), frame(dev, 401)
    assert not torch.equal(first.images, second.images)
    warmup = 4                      # (capture_all captures a phase's one-step graph behind three eager steps: both phases need four steps)
    cfg = config(warmup=warmup, init_seed=7)
    slot = new_loop(dev, first, cfg, graph=True, persistent=True)
    assert slot.capture_all(steps_per_graph=1) == 2
    graphs = {key: entry[0] for key, entry in slot._graphs.items()}
    slot.run(warmup + 2, steps_per_graph=1)
    assert slot.reset(second, init_seed=7) is True
    fresh = new_loop(dev, second, cfg, graph=True, persistent=True)
    with torch.no_grad():
        for p, v in zip((slot.detector.locations, slot.detector.dimensions, slot.detector.orientations), start_parameters()):
            p.copy_(v[None].to(dev))
        for a, b in zip(tensors(fresh)[0], tensors(slot)[0]):            # the two draws of the initial parameters agree (init_seed)
            assert same_bits(a.detach(), b.detach())
    assert same_bits(slot._photometric["gray"], fresh._photometric["gray"])
    for step in range(warmup + 4):
        a, b = slot.step(), fresh.step()
        torch.cuda.synchronize()
        for x, y in zip(state_bits(slot), state_bits(fresh)):
            assert same_bits(x, y), step
        if step >= warmup:
            assert same_bits(a["photometric_loss"].reshape(1), b["photometric_loss"].reshape(1))
            assert torch.equal(slot._photometric["ray_indices"], fresh._photometric["ray_indices"])
    assert {key: entry[0] for key, entry in slot._graphs.items()} == graphs                 # no new capture
    slot.close(), fresh.close()
