"""oracle/frame_glue.py -- the float64 reference of the frame prologue with its discrete choices as arguments -- pinned on the host: with
its own arg-min / arg-max selection and its own assignment it is torch.autograd through oracle.geometry.project_boxes_multi_view +
oracle.losses.projection_losses, on every scene tests/test_hip_frame_glue.py runs on the GPU.  The conditions those scenes are there for
(boxes behind a camera, across z = 0, outside the image, invisible; both smooth-L1 branches; a finite cost matrix) are asserted here, on
the reference alone, so that they are checked without a GPU."""
import pytest
import torch

import frame_glue_scenes as scenes
from oracle import frame_glue as ref


def _reference(scene):
    forward = ref.forward(scene["raw"], scene["E"], scene["K"], scenes.IMAGE_SIZE)
    cost = ref.cost_matrix(forward["boxes"][0], scene["gt_boxes"][0])
    return forward, cost


@pytest.mark.parametrize("V,N", list(scenes.SHAPES), ids=[f"{v}x{n}" for v, n in scenes.SHAPES])
def test_reference_reproduces_autograd_and_scene_conditions(V, N):
    scene = scenes.build(V, N, scenes.SHAPES[(V, N)])
    forward, cost = _reference(scene)
    assert bool(torch.isfinite(cost).all())                                   # the reference's matcher runs
    assignment = ref.assign(cost)
    args = (scene["raw"], scene["E"], scene["K"], scenes.IMAGE_SIZE, scene["gt_boxes"], scene["visible"], scenes.WEIGHTS)
    own = ref.gradients_at(*args, forward["selection"], assignment, forward["extremes"])
    boxes, matched, iou, l1, grad_raw = ref.autograd_reference(*args, assignment=assignment)
    # match_instances' own optimum may differ where two ground-truth columns are the same zeros (invisible in the target view): same cost
    rows = torch.arange(N)
    assert abs(float(cost[rows, matched].sum() - cost[rows, assignment].sum())) <= 1e-12 * N
    scale = float(grad_raw.abs().max())
    assert scale > 0
    assert float((forward["boxes"] - boxes).abs().max()) <= 1e-10 * 1408
    assert float((own["boxes"] - boxes).abs().max()) <= 1e-10 * 1408
    assert abs(float(own["iou"] - iou)) <= 1e-10 * float(iou) and abs(float(own["l1"] - l1)) <= 1e-10 * float(l1)
    assert float((own["grad_raw"] - grad_raw).abs().max()) <= 1e-10 * scale
    # the links: the per-view corner gradients sum to the gradient of the corners, the box gradients vanish on pairs that are not kept
    kept = scene["visible"][:, assignment]
    assert own["count"] == int(kept.sum()) and bool((own["grad_boxes"][~kept] == 0).all())
    raw = scene["raw"].clone().requires_grad_(True)
    _, corners = ref.decode(raw)
    chained, = torch.autograd.grad(corners, raw, own["grad_corners"].sum(0))
    assert float((chained - grad_raw).abs().max()) <= 1e-10 * scale
    # the instance rows are the decode's
    instances, _ = ref.decode(scene["raw"])
    assert instances.shape == (N, 16) and bool((instances[:, 15] == 0).all())
    # ---- what the scene is there for ------------------------------------------------------------------------------------------
    held = scenes.conditions(scene, forward, assignment)
    assert held["quadratic"] > 0 and held["linear"] > 0 and held["invisible"] > 0, held
    assert held["near_ties"] == 0, held                                       # (no DIoU gradient jump within float32's reach)
    if V >= 17:
        assert held["behind"] > 0 and held["straddling"] > 0 and held["outside"] > 0, held
    assert (V * N <= 256) == ((V, N) in ((8, 32), (4, 64), (1, 64)))
    # no extreme within 1e-2 px of the image border it is clamped at: float32 and float64 clamp the same coordinates
    limit = torch.tensor([1408.0, 376.0, 1408.0, 376.0], dtype=torch.float64)
    extremes = forward["extremes"][~forward["behind"]]
    assert not bool(((extremes.abs() < 1e-2) | ((extremes - limit).abs() < 1e-2)).any())
    if V * N <= 256:
        # the kernel keeps its selection in LDS there: the GPU test tries the near-tied alternatives box by box, which must stay few
        floor = float((ref.forward(scene["raw"].float(), scene["E"].float(), scene["K"].float(), scenes.IMAGE_SIZE)["boxes"].double() - forward["boxes"]).abs().max())
        choices = ref.alternatives(forward["cand"], forward["front"], forward["selection"], forward["extremes"], scenes.box_tolerance(floor))
        assert len(ref.selection_rounds(forward["selection"], choices)) <= 64


def test_unmatchable_scene_holds_a_nan_cost():
    """The dedicated scene of the GPU test: a prediction and a ground-truth box of the target view without area -- DIoU 0 / 0, on which the
    reference's matcher raises -- next to rows and columns whose costs are all finite."""
    V, N, seed = scenes.UNMATCHABLE
    scene = scenes.build(V, N, seed, matchable=False)
    _, cost = _reference(scene)
    bad = ~torch.isfinite(cost)
    assert bool(bad.any())
    with pytest.raises(ValueError):
        ref.assign(cost)
    rows, cols = ~bad.any(1), ~bad.any(0)
    assert int(rows.sum()) >= N // 2 and int(cols.sum()) >= N // 2


def test_selection_rounds_cover_every_combination():
    selection = torch.zeros(2, 3, 4, dtype=torch.int64)
    choices = {(0, 1, 0): [4, 5], (1, 1, 2): [6, 7, 8], (0, 2, 3): [9, 10]}
    rounds = ref.selection_rounds(selection, choices)
    assert len(rounds) == 6
    assert {(int(s[0, 1, 0]), int(s[1, 1, 2])) for s in rounds} == {(a, b) for a in (4, 5) for b in (6, 7, 8)}
    assert {int(s[0, 2, 3]) for s in rounds} == {9, 10} and all(int(s[1, 0, 0]) == 0 for s in rounds)
