"""csrc/frame_step.h -- the two single-workgroup kernels around every render launch of the native loop -- up to the ABI's 32 views x 64
boxes, through the C ABI with buffers of the test's own, against the float64 reference of oracle/frame_glue.py evaluated AT the choices
the device made (its assignment, and above 256 (view, box) pairs its selection, read back from the scratch).  Below that size the
prologue hands its phases' results on through LDS, above it through the caller's scratch in loops of more than one trip.

Where the bounds come from.  For every quantity the float32 oracle (the same reference in float32 at the same choices) is evaluated too
and its distance from the float64 reference is the floor; the device may be at max(project bound, 2 x floor).  Project bounds are those of
test_hip_step.py::test_frame_prologue_matches_the_torch_path: instances 1e-6 (relative to 1 + |x|), losses rtol 1e-5 / atol 1e-6, grad_raw
2e-4 of its largest entry.  2-D boxes and the intermediate gradients have no project bound: 2 x floor + the float32 spacing of the
quantity's largest magnitude (frame_glue_scenes.box_tolerance for the boxes).  The epilogue's update is compared with Adam's formula on
the kernel's own moments at 1e-3 lr + 1e-7 max|p| (test_hypernetwork_kernels_match_torch, for the reason given there)."""
import ctypes

import pytest
import torch

import frame_glue_scenes as scenes
from conftest import margin
from oracle import frame_glue as ref, losses as olosses

pytestmark = pytest.mark.gpu

NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()
GUARD = 4096                               # floats behind the scratch that must keep the fill pattern
NUM_STEPS, W_SIL, BETAS, ADAM_EPS, GAMMA = 3000, 1.0, (0.9, 0.999), 1.0e-8, 0.999
SPACING = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _frame_config(V, N):
    from oracle import geometry
    from vsrd_amd import _lib
    return _lib.make_frame_config(N, V, scenes.IMAGE_SIZE, 1.0e-6, geometry.LOCATION_RANGE, geometry.DIMENSION_RANGE, num_steps=NUM_STEPS,
                                  temperatures=(1.0, 0.1), std_deviations=(1.0, 0.1), loss_weights=(scenes.WEIGHTS[0], scenes.WEIGHTS[1], W_SIL),
                                  betas=BETAS, adam_epsilon=ADAM_EPS, lr_gamma=GAMMA)


def _is_fill(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _prologue(dev, scene, step, sample=False, capacity=None):
    """One launch on buffers of the test's own, everything the kernel writes pre-filled with NaN bits (integers with -7).  `capacity`:
    the rows are laid out for that many boxes and the frame's own count travels in a header (the _with_header twins)."""
    from vsrd_amd import _lib, rendering
    lib = _lib.load()
    V, n = scene["visible"].shape
    NS = n if capacity is None else capacity
    nan = float("nan")
    raw = torch.full((NS, 8), nan)
    raw[:n] = scene["raw"].float()
    gt = torch.full((V, NS, 4), nan)
    gt[:, :n] = scene["gt_boxes"].float()
    visible = torch.ones(V, NS, dtype=torch.uint8)
    visible[:, :n] = scene["visible"].to(torch.uint8)
    t = dict(loc=raw[:, 0:3].contiguous().to(dev), dim=raw[:, 3:6].contiguous().to(dev), ori=raw[:, 6:8].contiguous().to(dev),
             E=scene["E"].float().reshape(V, 16).contiguous().to(dev), K=scene["K"].float().reshape(V, 9).contiguous().to(dev),
             gt=gt.to(dev), visible=visible.to(dev), step=torch.tensor([step], dtype=torch.int64, device=dev))
    scratch_bytes = lib.vsrd_frame_scratch_bytes(V, NS)
    assert scratch_bytes == V * NS * 36 * 4
    out = dict(scratch=torch.full((scratch_bytes // 4 + GUARD,), nan, device=dev), instances=torch.full((NS, 16), nan, device=dev),
               pd_indices=torch.full((NS,), -7, dtype=torch.int64, device=dev), gt_indices=torch.full((NS,), -7, dtype=torch.int64, device=dev),
               target_columns=torch.full((NS,), -7, dtype=torch.int32, device=dev), instance_weights=torch.full((NS,), nan, device=dev),
               schedule=torch.full((3,), nan, device=dev), losses=torch.full((2,), nan, device=dev), grad_raw=torch.full((NS, 8), nan, device=dev))
    frame = _frame_config(V, NS)
    args = [frame, _lib.ptr(t["loc"]), _lib.ptr(t["dim"]), _lib.ptr(t["ori"]), _lib.ptr(t["E"]), _lib.ptr(t["K"]), _lib.ptr(t["gt"]),
            t["visible"].data_ptr(), t["step"].data_ptr(), out["scratch"].data_ptr(), scratch_bytes, _lib.ptr(out["instances"]),
            out["pd_indices"].data_ptr(), out["gt_indices"].data_ptr(), out["target_columns"].data_ptr(), _lib.ptr(out["instance_weights"]),
            _lib.ptr(out["schedule"]), _lib.ptr(out["losses"]), _lib.ptr(out["grad_raw"])]
    name = "vsrd_frame_prologue"
    if sample:
        table = rendering.RayTable((torch.rand(4096, generator=torch.Generator().manual_seed(1)) + 0.1).to(dev))
        rays = torch.full((64,), -7, dtype=torch.int64, device=dev)
        args += [table.table.data_ptr(), table.count, 64, 5, None, rays.data_ptr()]
        name += "_sample"
    if capacity is not None:
        header = torch.zeros(2, dtype=torch.int32, device=dev)
        header[0] = n
        header.view(torch.float32)[1] = 1.0
        args.append(header.data_ptr())
        name += "_with_header"
    _lib.check(getattr(lib, name)(*args, _lib.stream()))
    torch.cuda.synchronize()
    if sample:
        assert bool(((rays >= 0) & (rays < 4096)).all())
    out = {key: value.cpu() for key, value in out.items()}
    out["scratch_floats"] = scratch_bytes // 4
    return out


def _float32(scene):
    return {key: value.float() if value.dtype == torch.float64 else value for key, value in scene.items()}


def _reference_at(scene, selection, assignment, extremes):
    """The float64 reference and the float32 oracle at the same choices."""
    both = []
    for s, e in ((scene, extremes), (_float32(scene), extremes.float())):
        both.append(ref.gradients_at(s["raw"], s["E"], s["K"], scenes.IMAGE_SIZE, s["gt_boxes"], s["visible"], scenes.WEIGHTS, selection, assignment, e))
    return both


def _bound(project, floor, label, what, observed):
    tolerance = max(project, 2.0 * floor)
    margin(label, what, observed, tolerance)
    assert observed <= tolerance, (label, what, observed, tolerance, floor)


def _check_assignment(label, out, n, cost, cost32, unmatched=None):
    """A permutation whose float64 cost is the float64 optimum within the float32 rounding of the costs; the optimum's own indices where it
    is unique by more than that (every row in turn is forbidden its column and the problem solved again: the smallest loss is the gap)."""
    assignment = out["gt_indices"][:n]
    assert sorted(assignment.tolist()) == list(range(n)) and out["pd_indices"][:n].tolist() == list(range(n))
    assert torch.equal(out["target_columns"][:n].long(), assignment) and bool((out["instance_weights"][:n] == 1.0).all())
    rows = torch.arange(n)
    if unmatched is not None:                                              # rows / columns with a NaN cost: nothing asserted about them
        good_rows, good_cols = unmatched
        inside = good_rows & good_cols[assignment]
        # the device's pairs that stay inside the finite block must be an optimal matching of the rows and columns they use
        r, c = rows[inside], assignment[inside]
        sub = cost[r][:, c]
        best = float(sub[torch.arange(len(r)), ref.assign(sub)].sum())
        rounding = 2.0 * len(r) * max(float((cost32.double() - cost)[r][:, c].abs().max()), SPACING) + len(r) * SPACING
        excess = float(sub.diagonal().sum()) - best
        margin(label, "matching cost - optimum", excess, rounding)
        assert excess <= rounding
        return assignment
    optimum = ref.assign(cost)
    best = float(cost[rows, optimum].sum())
    rounding = 2.0 * n * max(float((cost32.double() - cost).abs().max()), SPACING) + n * SPACING
    excess = float(cost[rows, assignment].sum()) - best
    margin(label, "matching cost - optimum", excess, rounding)
    assert -1e-12 <= excess <= rounding
    gap = float("inf")
    for i in range(n if n > 1 else 0):
        forbidden = cost.clone()
        forbidden[i, optimum[i]] = 1.0e6
        gap = min(gap, float(forbidden[rows, ref.assign(forbidden)].sum()) - best)
    if gap > rounding:
        assert torch.equal(assignment, optimum)
    return assignment


def _check_prologue(label, scene, out, step, unmatchable=False):
    """-> the float64 reference at the device's choices (None for the scene the reference cannot match on)."""
    V, n = scene["visible"].shape
    pairs = V * n
    large = pairs > 256
    size = scenes.IMAGE_SIZE
    forward = ref.forward(scene["raw"], scene["E"], scene["K"], size)
    s32 = _float32(scene)
    forward32 = ref.forward(s32["raw"], s32["E"], s32["K"], size)
    # ---- instances, schedule -------------------------------------------------------------------------------------------------
    relative = lambda a, b: float(((a.double() - b) / (1.0 + b.abs())).abs().max())
    _bound(1e-6, relative(forward32["instances"], forward["instances"]), label, "instances", relative(out["instances"][:n], forward["instances"]))
    ratio, temperature, std = olosses.schedules(step, NUM_STEPS)
    torch.testing.assert_close(out["schedule"].double(), torch.tensor([temperature, std, ratio], dtype=torch.float64), rtol=1e-5, atol=1e-6)
    # ---- matching ------------------------------------------------------------------------------------------------------------
    cost = ref.cost_matrix(forward["boxes"][0], scene["gt_boxes"][0])
    cost32 = ref.cost_matrix(forward32["boxes"][0], s32["gt_boxes"][0])
    unmatched = None
    if unmatchable:
        bad = ~torch.isfinite(cost)
        assert bool(bad.any())
        unmatched = (~bad.any(1), ~bad.any(0))
    assignment = _check_assignment(label, out, n, cost, cost32, unmatched)
    assert bool(torch.isfinite(out["losses"]).all()) and bool(torch.isfinite(out["grad_raw"][:n]).all())
    # ---- the scratch: untouched on the LDS path and behind its end ------------------------------------------------------------
    scratch = out["scratch"]
    assert _is_fill(scratch[pairs * 36 if large else 0:])                    # (a header twin: nothing behind the frame's own pairs either)
    box_tolerance = scenes.box_tolerance(float((forward32["boxes"].double() - forward["boxes"]).abs().max()))
    if not large:
        # the selection stayed in LDS: the near-tied alternatives of the reference's own are tried, box by box
        selections = ref.selection_rounds(forward["selection"], ref.alternatives(forward["cand"], forward["front"], forward["selection"],
                                                                                  forward["extremes"], box_tolerance))
    else:
        boxes = scratch[:pairs * 4].reshape(V, n, 4).double()
        selection = scratch[pairs * 4:pairs * 8].view(torch.int32).reshape(V, n, 4).long()
        observed = float((boxes - forward["boxes"]).abs().max())
        margin(label, "2-D boxes [px]", observed, box_tolerance)
        assert observed <= box_tolerance
        # every selection names an end point of an edge in front whose float64 value is the float64 extreme; -1 exactly where the reference
        # clamps or the box is behind (the scenes keep every extreme 1e-2 px away from the border it could be clamped at)
        assert torch.equal(selection < 0, forward["selection"] < 0) and int(selection.max()) < 24
        named = selection >= 0
        edge = selection.clamp_min(0) >> 1
        values = forward["cand"][..., torch.tensor([0, 1, 0, 1])].transpose(-1, -2)                  # [V,n,4,24]
        ends = torch.stack([values.gather(-1, (2 * edge)[..., None]).squeeze(-1), values.gather(-1, (2 * edge + 1)[..., None]).squeeze(-1)], -1)
        off = (ends - forward["extremes"][..., None]).abs()
        assert bool(forward["front"].gather(-1, edge)[named].all())
        worst = float(off.min(-1).values[named].max())
        margin(label, "selected end - extreme [px]", worst, box_tolerance)
        assert worst <= box_tolerance
        # far end or near end by VALUE (an edge parallel to the image plane may order its ends differently in float32); where both ends
        # are the extreme, both are tried, pair by pair
        resolved = torch.where(named, 2 * edge + off.argmin(-1), selection)
        both = named & (off.max(-1).values <= box_tolerance)
        selections = [resolved]
        if bool(both.any()):
            selections = [torch.where(both, 2 * edge + ((torch.tensor(r) >> torch.arange(4)) & 1), resolved) for r in range(16)]
    if unmatchable:
        return None
    # ---- losses and gradients at the device's choices ---------------------------------------------------------------------------
    if large:
        # Link by link: every link against the reference fed with what the device fed it.  The corner gradients are the projection's adjoint
        # applied to the box gradients, so the reference applies it to the DEVICE's box gradients: compared with the reference's own, this
        # link would be charged the rounding of the 2-D boxes again (smooth-L1's quadratic branch hands a box error of 3e-4 px on as it is).
        count = max(int(scene["visible"][:, assignment].sum()), 1)
        gb = scratch[pairs * 8:pairs * 12].reshape(V, n, 4).double() / count              # (the kernel divides by the count where it reads them)
        gw = scratch[pairs * 12:pairs * 36].reshape(V, n, 8, 3).double()
        errors = []
        for sel in selections:                                                # per (view, box): the combination of tied ends that fits
            r64 = ref.gradients_at(scene["raw"], scene["E"], scene["K"], size, scene["gt_boxes"], scene["visible"], scenes.WEIGHTS, sel, assignment,
                                   forward["extremes"], box_cotangent=gb)
            errors.append((gw - r64["grad_corners"]).abs().amax((-1, -2)))
        best = torch.stack(errors).argmin(0)                                  # [V,n]
        selections = [torch.stack(selections).gather(0, best[None, ..., None].expand(1, V, n, 4))[0]]
        link64 = ref.gradients_at(scene["raw"], scene["E"], scene["K"], size, scene["gt_boxes"], scene["visible"], scenes.WEIGHTS, selections[0],
                                  assignment, forward["extremes"], box_cotangent=gb)["grad_corners"]
        link32 = ref.gradients_at(s32["raw"], s32["E"], s32["K"], size, s32["gt_boxes"], s32["visible"], scenes.WEIGHTS, selections[0],
                                  assignment, forward["extremes"].float(), box_cotangent=gb.float())["grad_corners"].double()
    error = floor = None
    for sel in selections:
        r64, r32 = _reference_at(scene, sel, assignment, forward["extremes"])
        scale = float(r64["grad_raw"].abs().max())
        assert scale > 0
        e = (out["grad_raw"][:n].double() - r64["grad_raw"]).abs().amax(-1) / scale                          # per box
        f = float((r32["grad_raw"].double() - r64["grad_raw"]).abs().max()) / scale
        error, floor = (e, f) if error is None else (torch.minimum(error, e), max(floor, f))
    _bound(2e-4, floor, label, "grad_raw / max", float(error.max()))
    for k, name in enumerate(("iou", "l1")):
        value = float(r64[name])
        _bound(1e-5 * abs(value) + 1e-6, abs(float(r32[name]) - value), label, name + " loss", abs(float(out["losses"][k]) - value))
    if large:
        assert count == max(r64["count"], 1)
        for name, got, want, want32 in (("box gradients / max", gb, r64["grad_boxes"], r32["grad_boxes"].double()), ("corner gradients / max", gw, link64, link32)):
            scale = float(want.abs().max())
            floor = float((want32 - want).abs().max()) / scale
            _bound(SPACING, floor + SPACING / 2, label, name, float((got - want).abs().max()) / scale)      # 2 x floor + spacing
    return r64


@pytest.mark.parametrize("V,N", list(scenes.SHAPES), ids=[f"{v}x{n}" for v, n in scenes.SHAPES])
def test_prologue_matches_float64_reference(dev, V, N):
    """3a: every shape, both entry points (256 and 1024 threads), several steps of the schedule."""
    scene = scenes.build(V, N, scenes.SHAPES[(V, N)])
    label = f"test_prologue_matches_float64_reference[{V}x{N}]"
    for step in (0, 1, NUM_STEPS):
        out = _prologue(dev, scene, step)
        ratio, temperature, std = olosses.schedules(step, NUM_STEPS)
        torch.testing.assert_close(out["schedule"].double(), torch.tensor([temperature, std, ratio], dtype=torch.float64), rtol=1e-5, atol=1e-6)
    plain = _prologue(dev, scene, 700)
    sampled = _prologue(dev, scene, 700, sample=True)
    r64 = _check_prologue(label, scene, plain, 700)
    _check_prologue(label + "[sample]", scene, sampled, 700)
    for name in ("instances", "pd_indices", "gt_indices", "target_columns", "instance_weights", "schedule"):
        assert torch.equal(plain[name], sampled[name]), name
    # the two workgroup sizes sum in different orders above 256 pairs: each within its bound of the reference, so within twice of each other
    scale = float(r64["grad_raw"].abs().max())
    assert float((plain["grad_raw"] - sampled["grad_raw"]).abs().max()) <= 4e-4 * scale
    torch.testing.assert_close(plain["losses"], sampled["losses"], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("V,capacity,n", [(17, 20, 9), (17, 20, 16), (17, 64, 16), (17, 64, 15), (4, 64, 40)])
@pytest.mark.parametrize("sample", [False, True], ids=["prologue", "prologue_sample"])
def test_prologue_header_twins_on_either_side_of_256_pairs(dev, V, capacity, n, sample):
    """3b: a row laid out for `capacity` boxes whose header says n gives the bits of a launch with by-value N = n, whichever of the two
    data paths V n takes, and leaves the pad rows of every output alone."""
    scene = scenes.build(V, n, 1)
    alone = _prologue(dev, scene, 700, sample=sample)
    twin = _prologue(dev, scene, 700, sample=sample, capacity=capacity)
    for name in ("instances", "pd_indices", "gt_indices", "target_columns", "instance_weights", "grad_raw"):
        assert torch.equal(twin[name][:n], alone[name]), name
        pad = twin[name][n:]
        assert _is_fill(pad) if pad.dtype == torch.float32 else bool((pad == -7).all()), name
    assert not _is_fill(alone["grad_raw"]) and bool(torch.isfinite(alone["grad_raw"]).all())
    assert torch.equal(twin["schedule"], alone["schedule"]) and torch.equal(twin["losses"], alone["losses"])
    pairs = V * n
    if pairs > 256:                                     # the frame's own pairs at the front of the capacity's scratch, nothing behind them
        assert torch.equal(twin["scratch"][:pairs * 36].view(torch.int32), alone["scratch"][:pairs * 36].view(torch.int32))
        assert _is_fill(twin["scratch"][pairs * 36:])
    else:
        assert _is_fill(twin["scratch"]) and _is_fill(alone["scratch"])


def test_prologue_on_costs_the_reference_cannot_match(dev):
    """3e: a prediction and a ground-truth box of the target view that are both clamped to zero area have DIoU 0 / 0; scipy raises in the
    reference, the kernel maps such costs to 3e38 (matching.h).  It must return a permutation, finite losses and gradients, and on the
    rows and columns whose costs are finite an optimal matching; nothing is asserted about how the NaN pairs are paired."""
    V, N, seed = scenes.UNMATCHABLE
    scene = scenes.build(V, N, seed, matchable=False)
    for sample in (False, True):
        _check_prologue("test_prologue_on_costs_the_reference_cannot_match", scene, _prologue(dev, scene, 700, sample=sample), 700, unmatchable=True)


@pytest.mark.parametrize("N", [1, 9, 40, 64])
def test_epilogue_matches_float64_reference(dev, N):
    """3c: decode adjoint + Adam + rate decay + record at up to 64 boxes, three consecutive calls from moments, step counters and rates that
    are not the initial ones; the render adjoint is random, the projection gradient and losses are a prologue's."""
    from vsrd_amd import _lib
    lib = _lib.load()
    label = f"test_epilogue_matches_float64_reference[{N}]"
    scene = scenes.build(4, N, 3)
    produced = _prologue(dev, scene, 700)
    g = torch.Generator().manual_seed(40 + N)
    raw = scene["raw"].float()
    slices = (slice(0, 3), slice(3, 6), slice(6, 8))
    params = [raw[:, s].contiguous().to(dev) for s in slices]
    exp_avg = [(0.01 * torch.randn(N, s.stop - s.start, generator=g)).to(dev) for s in slices]
    exp_avg_sq = [(1e-4 * torch.rand(N, s.stop - s.start, generator=g) + 1e-8).to(dev) for s in slices]
    steps = [torch.tensor(float(v), device=dev) for v in (5, 6, 7)]
    rates = [torch.tensor(v, device=dev) for v in (1e-2, 3e-3, 2e-3)]
    others = [torch.tensor(v, device=dev) for v in (1e-3, 1e-4)]
    counter = torch.tensor([11], dtype=torch.int64, device=dev)
    grad_raw, projection_losses = produced["grad_raw"].to(dev), produced["losses"].to(dev)
    assert bool(torch.isfinite(grad_raw).all()) and float(grad_raw.abs().max()) > 0
    render_losses = torch.tensor([0.37, 1.9], device=dev)
    record, raw_gradients = torch.full((5,), float("nan"), device=dev), torch.full((N, 8), float("nan"), device=dev)
    adam = [_lib.AdamTensors(p.data_ptr(), m.data_ptr(), v.data_ptr(), s.data_ptr(), lr.data_ptr()) for p, m, v, s, lr in zip(params, exp_avg, exp_avg_sq, steps, rates)]
    frame = _frame_config(4, N)
    eikonal_ratio = 0.3
    for call in range(3):
        grad_instances = torch.randn(N, 16, generator=g).to(dev)
        old = dict(p=torch.cat(params, -1).cpu(), m=torch.cat(exp_avg, -1).cpu().double(), v=torch.cat(exp_avg_sq, -1).cpu().double(),
                   steps=[float(s) for s in steps], rates=[float(r) for r in rates], others=[float(r) for r in others])
        _lib.check(lib.vsrd_frame_epilogue(frame, _lib.ptr(grad_instances), _lib.ptr(grad_raw), _lib.ptr(projection_losses), _lib.ptr(render_losses),
                                           eikonal_ratio, ctypes.byref(adam[0]), ctypes.byref(adam[1]), ctypes.byref(adam[2]), _lib.ptr(others[0]),
                                           _lib.ptr(others[1]), counter.data_ptr(), _lib.ptr(record), _lib.ptr(raw_gradients), _lib.stream()))
        torch.cuda.synchronize()
        # raw gradients: the chain through sigmoid / lerp / normalize by autograd, float64, and the float32 oracle for the floor
        want = ref.epilogue_raw_gradients(old["p"].double(), grad_instances.cpu().double(), grad_raw.cpu().double(), W_SIL)
        want32 = ref.epilogue_raw_gradients(old["p"], grad_instances.cpu(), grad_raw.cpu(), W_SIL)
        scale = float(want.abs().max())
        _bound(2e-4, float((want32.double() - want).abs().max()) / scale, label, "raw_gradients / max", float((raw_gradients.cpu().double() - want).abs().max()) / scale)
        m = old["m"] + (want - old["m"]) * (1.0 - BETAS[0])
        v = old["v"] * BETAS[1] + (1.0 - BETAS[1]) * want * want
        got_m, got_v, got_p = torch.cat(exp_avg, -1).cpu().double(), torch.cat(exp_avg_sq, -1).cpu().double(), torch.cat(params, -1).cpu().double()
        for name, got, wanted in (("exp_avg / max", got_m, m), ("exp_avg_sq / max", got_v, v)):       # (the bound of test_hypernetwork_kernels_match_torch)
            observed = float((got - wanted).abs().max()) / float(wanted.abs().max())
            margin(label, name, observed, 2e-4)
            assert observed <= 2e-4
        for k, s in enumerate(slices):
            assert float(steps[k]) == old["steps"][k] + 1
            assert abs(float(rates[k]) - old["rates"][k] * GAMMA) <= 1e-6 * old["rates"][k]
            bc1, bc2 = 1.0 - BETAS[0] ** (old["steps"][k] + 1), 1.0 - BETAS[1] ** (old["steps"][k] + 1)
            expected = old["p"][:, s].double() - (old["rates"][k] / bc1) * got_m[:, s] / (got_v[:, s].sqrt() / bc2 ** 0.5 + ADAM_EPS)
            tolerance = 1e-3 * old["rates"][k] + 1e-7 * float(old["p"][:, s].abs().max())
            observed = float((expected - got_p[:, s]).abs().max())
            margin(label, f"update of group {k}", observed, tolerance)
            assert observed <= tolerance
        for k in range(2):
            assert abs(float(others[k]) - old["others"][k] * GAMMA) <= 1e-6 * old["others"][k]
        assert int(counter) == 12 + call
        iou, l1, sil, eik = float(projection_losses[0]), float(projection_losses[1]), float(render_losses[0]), float(render_losses[1])
        assert record[:4].tolist() == [iou, l1, sil, eik]
        total = scenes.WEIGHTS[0] * iou + scenes.WEIGHTS[1] * l1 + W_SIL * (sil + eikonal_ratio * eik)
        assert abs(float(record[4]) - total) <= 1e-6 * abs(total)


def _loop_config():
    from vsrd_amd import optimization
    return optimization.OptimizationConfig(num_samples=40, num_rays=128, warmup_steps=4, num_steps=40, seed=3, mlp_adjoint_item_slots=8)


def test_loops_on_the_large_path_walk_the_same_trajectory_alone_and_in_a_batch(dev):
    """3d: 17 views x 16 boxes (272 pairs) through FrameOptimizer(graph=True) and FrameBatch, box-only and residual steps: a frame of a
    batch -- its scratch is its own row's -- walks, bit for bit, the trajectory it walks alone; in a mixed batch of capacity 20 one launch
    takes the scratch path for the row of 16 and the LDS path for the row of 9, and the pad instances stay untouched."""
    from test_frame_batch_mixed import _fill_pads, _pads_untouched, _state
    from vsrd_amd import launcher, optimization
    config, steps = _loop_config(), 7
    frames, alone = [], []
    frame_number = 200
    for k, n in enumerate((16, 16, 9)):
        while True:
            inputs = launcher.synthetic_frame_inputs(dev, frame_number, 17, n, height=128, width=128)
            frame_number += 1
            try:
                slot = optimization.FrameOptimizer(inputs, config, dev, graph=True, persistent=True)
            except optimization.UnsuitableFrameError:
                continue
            break
        assert slot.fused_glue
        slot.capture_all()
        assert slot.reset(inputs, init_seed=80 + k)
        slot.run(steps)
        torch.cuda.synchronize()
        assert slot.step_index == steps
        frames.append(inputs)
        alone.append(_state(slot))
        slot.close()
    for members, capacity in (((0, 1), None), ((0, 2), 20)):
        batch = optimization.FrameBatch([frames[k] for k in members], config, dev, init_seeds=[80 + k for k in members], max_instances=capacity)
        batch.capture_all(actives=[2])
        for row, k in enumerate(members):
            assert batch.reset(row, frames[k], init_seed=80 + k)
            if capacity is not None:
                _fill_pads(batch.frames[row])
        batch.run(steps, active=2)
        torch.cuda.synchronize()
        for row, k in enumerate(members):
            member = batch.frames[row]
            assert member.step_index == steps
            for index, (a, b) in enumerate(zip(_state(member), alone[k])):
                assert a.shape == b.shape and torch.equal(a, b), (capacity, k, index)
            if capacity is not None:
                _pads_untouched(member)
        batch.close()
