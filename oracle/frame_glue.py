"""Oracle: the frame prologue / epilogue (csrc/frame_step.h) with its discrete choices made explicit (TEST INFRASTRUCTURE).

The prologue makes three kinds of discrete choice: which edge end point gives each extreme of a projected box (the *selection*), which
ground-truth box every prediction is matched with (the *assignment*), and which branch every clamp takes.  float32 and float64 break a
near-tie differently, and the gradient is discontinuous across such a flip, so a reference that makes its own choices can only be compared
where no tie is near.  Here the choices are arguments: `gradients_at` evaluates losses and gradients AT a given selection and assignment,
every extreme's gradient flowing through the end point the selection names.  With its own choices (`own_selection`, `assign`) it is
`torch.autograd` through `geometry.project_boxes_multi_view` + `losses.projection_losses` (tests/test_frame_glue_reference.py).

Everything is plain torch in the dtype of the raw parameters (float64 for the reference, float32 for the rounding floor), the gradients are
autograd's through `gather` -- nothing of the kernel's hand-derived adjoint is restated.

Index convention of the 24 candidates of a box: 2 e + end, edge e of `geometry.BOX_EDGES`, end 0 = the deeper ("far") corner, end 1 = the
other one pulled to z = 0 where the edge straddles it (`geometry.clip_edges_to_front`).  2-D boxes are (x1, y1, x2, y2).
"""
import itertools

import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

from . import geometry, losses

EPSILON = 1.0e-6


def decode(raw):
    """raw [N,8] (location 3 | dimension 3 | orientation 2) -> (instances [N,16], corners [N,8,3]): the renderer's instance rows
    (location 3 | R_y 9 | half extents 3 | 0) and the world corners."""
    loc, dim, rot, corners = geometry.decode_box_parameters(raw[:, 0:3], raw[:, 3:6], raw[:, 6:8])
    return torch.cat([loc, rot.flatten(-2, -1), dim, torch.zeros_like(loc[:, :1])], dim=-1), corners


def candidates(view_corners, extrinsics, intrinsics):
    """view_corners [V,N,8,3] (the world corners, one copy per view, so that a per-view gradient can be asked for) ->
    (candidate pixel coordinates [V,N,24,2], edge-in-front mask [V,N,12], camera-frame corners [V,N,8,3])."""
    homog = F.pad(view_corners, (0, 1), value=1.0)
    cam = torch.einsum("vmn,vikn->vikm", extrinsics, homog)
    cam = cam[..., :3] / cam[..., 3:]
    idx = torch.tensor(geometry.BOX_EDGES)
    edges, front = geometry.clip_edges_to_front(cam[..., idx, :], EPSILON)                  # [V,N,12,2,3], [V,N,12]
    pix = edges @ intrinsics[:, None, None].transpose(-1, -2)
    pix = pix[..., :2] / pix[..., 2:].clamp_min(EPSILON)
    return pix.flatten(-3, -2), front, cam


def own_selection(cand, front, image_size):
    """The reference's own arg-min / arg-max: (selection [V,N,4] int64, -1 where the coordinate is clamped to the image or the box is
    behind the camera; unclamped extremes [V,N,4]; box-behind mask [V,N])."""
    height, width = image_size
    keep = front.repeat_interleave(2, dim=-1)[..., None]
    inf = torch.full_like(cand, float("inf"))
    lo = torch.where(keep, cand, inf).min(dim=-2)
    hi = torch.where(keep, cand, -inf).max(dim=-2)
    behind = ~front.any(-1)
    extremes = torch.cat([lo.values, hi.values], dim=-1)
    extremes = torch.where(behind[..., None], torch.zeros_like(extremes), extremes)
    selection = torch.cat([lo.indices, hi.indices], dim=-1)
    limit = torch.tensor([width, height, width, height]).to(cand)
    clamped = (extremes < 0) | (extremes > limit)
    selection = torch.where(clamped | behind[..., None], torch.full_like(selection, -1), selection)
    return selection, extremes.detach(), behind


def boxes_at(cand, selection, extremes, image_size):
    """Clipped 2-D boxes [V,N,4] whose coordinate k is candidate `selection[..., k]` (u for k = 0, 2; v for k = 1, 3); where the selection
    is -1 the constant `extremes` (no gradient)."""
    height, width = image_size
    uv = torch.tensor([0, 1, 0, 1])
    picked = cand[..., uv].gather(-2, selection.clamp_min(0)[..., None, :]).squeeze(-2)      # cand[v, n, sel[k], uv[k]]
    coords = torch.where(selection >= 0, picked, extremes.to(cand))
    limit = torch.tensor([width, height, width, height]).to(cand)
    return torch.minimum(torch.maximum(coords, torch.zeros_like(coords)), limit)


def cost_matrix(boxes_target, gt_target):
    """main.py:374-386: negative DIoU of the target view, [N,4] x [N,4] -> [N,N] (NaN where both boxes have no area)."""
    return -geometry.distance_box_iou(boxes_target, gt_target)


def assign(cost):
    """Ground-truth column of every prediction (scipy's Hungarian; raises on a cost that is not finite, as the reference does)."""
    rows, cols = linear_sum_assignment(cost.detach().cpu().numpy())
    assert list(rows) == list(range(cost.shape[0]))
    return torch.as_tensor(cols, dtype=torch.int64)


def forward(raw, extrinsics, intrinsics, image_size):
    """The forward half with the reference's own choices: a dict of instances, corners, cand, front, selection, extremes, behind, boxes."""
    instances, corners = decode(raw)
    view_corners = corners[None].expand(extrinsics.shape[0], *corners.shape)
    cand, front, cam = candidates(view_corners, extrinsics, intrinsics)
    selection, extremes, behind = own_selection(cand, front, image_size)
    boxes = boxes_at(cand, selection, extremes, image_size)
    return dict(instances=instances, corners=corners, cand=cand, front=front, cam=cam, selection=selection, extremes=extremes, behind=behind,
                boxes=boxes)


def gradients_at(raw, extrinsics, intrinsics, image_size, gt_boxes, visible, weights, selection, assignment, extremes, box_cotangent=None):
    """Losses and gradients at the given choices.  gt_boxes [V,N,4], visible [V,N] (bool, by ground-truth instance), weights
    (w_iou, w_l1), selection [V,N,4] (candidate index or -1), assignment [N] (ground-truth column of prediction n), extremes [V,N,4]
    (the value of a coordinate whose selection is -1).  Returns a dict: boxes [V,N,4], iou, l1, count (kept pairs),
    grad_boxes [V,N,4] = d (w_iou iou + w_l1 l1) / d boxes, grad_corners [V,N,8,3] (world frame, per view), grad_raw [N,8].
    `box_cotangent` [V,N,4]: grad_corners is the adjoint of the projection applied to THESE box gradients instead of the reference's own
    -- the link from box gradients to corner gradients alone, without the rounding of the links before it."""
    raw = raw.detach().clone().requires_grad_(True)
    _, corners = decode(raw)
    view_corners = corners[None].expand(extrinsics.shape[0], *corners.shape).clone()
    cand, _, _ = candidates(view_corners, extrinsics, intrinsics)
    boxes = boxes_at(cand, selection, extremes, image_size)
    pd_idx = torch.arange(raw.shape[0])
    shape = (*boxes.shape[:2], 2, 2)
    iou, l1 = losses.projection_losses(boxes.reshape(shape), gt_boxes.reshape(shape), visible, pd_idx, assignment)
    total = weights[0] * iou + weights[1] * l1
    grad_boxes, grad_corners, grad_raw = torch.autograd.grad(total, [boxes, view_corners, raw], allow_unused=True, retain_graph=box_cotangent is not None)
    if box_cotangent is not None:
        grad_corners, = torch.autograd.grad(boxes, view_corners, grad_outputs=box_cotangent.to(boxes), allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    return dict(boxes=boxes.detach(), iou=iou.detach(), l1=l1.detach(), count=int(visible[:, assignment].sum()),
                grad_boxes=zero(grad_boxes, boxes), grad_corners=zero(grad_corners, view_corners), grad_raw=zero(grad_raw, raw))


def autograd_reference(raw, extrinsics, intrinsics, image_size, gt_boxes, visible, weights, assignment=None):
    """The same quantities by autograd straight through geometry.project_boxes_multi_view + losses.match_instances /
    projection_losses (what `gradients_at` with the reference's own choices must reproduce): (boxes [V,N,4], assignment, iou, l1, grad_raw).
    `assignment`: evaluate at this one instead of match_instances' own (two invisible ground-truth boxes of the target view are the same
    column of zeros: the optimum is then not unique)."""
    raw = raw.detach().clone().requires_grad_(True)
    _, corners = decode(raw)
    boxes, _ = geometry.project_boxes_multi_view(corners, extrinsics, intrinsics, image_size)
    shape = boxes.shape
    gt = gt_boxes.reshape(shape)
    pd_idx, gt_idx = losses.match_instances(boxes[0], gt[0])
    assert torch.equal(pd_idx, torch.arange(raw.shape[0]))
    if assignment is not None:
        gt_idx = assignment
    iou, l1 = losses.projection_losses(boxes, gt, visible, pd_idx, gt_idx)
    grad_raw, = torch.autograd.grad(weights[0] * iou + weights[1] * l1, raw)
    return boxes.detach().flatten(-2, -1), gt_idx, iou.detach(), l1.detach(), grad_raw


def admissible(cand, front, extremes, tolerance):
    """[V,N,4,24] bool: candidates of an edge in front whose value is within `tolerance` of the coordinate's extreme."""
    uv = torch.tensor([0, 1, 0, 1])
    values = cand[..., uv].transpose(-1, -2)                                               # [V,N,4,24]
    keep = front.repeat_interleave(2, dim=-1)[..., None, :]
    return keep & ((values - extremes[..., None]).abs() <= tolerance)


def alternatives(cand, front, selection, extremes, tolerance, merge=1.0e-9):
    """The selections float32 may legitimately make instead of the reference's own: for every coordinate with a selection, the admissible
    candidates with distinct values (candidates within `merge` of each other are one corner reached over several edges: one gradient).
    Returns {(v, n, k): [candidate indices]} for the coordinates that have more than one."""
    ok = admissible(cand, front, extremes, tolerance) & (selection >= 0)[..., None]
    uv = (0, 1, 0, 1)
    out = {}
    for v, n, k in (ok.sum(-1) > 1).nonzero().tolist():
        picks = []
        for index in ok[v, n, k].nonzero().flatten().tolist():
            if all(abs(float(cand[v, n, index, uv[k]] - cand[v, n, other, uv[k]])) > merge for other in picks):
                picks.append(index)
        if len(picks) > 1:
            out[(v, n, k)] = picks
    return out


def selection_rounds(selection, choices, limit=256):
    """Selections that between them try every combination of `choices` ({(v, n, k): [indices]}) box by box: the gradient of box n depends
    on the selections of box n alone, so round r holds the r-th combination of every box at once."""
    per_box = {}
    for (v, n, k), picks in choices.items():
        per_box.setdefault(n, []).append(((v, k), picks))
    combos = {n: list(itertools.product(*[picks for _, picks in entries])) for n, entries in per_box.items()}
    rounds = max([len(c) for c in combos.values()], default=1)
    assert rounds <= limit, f"{rounds} combinations of near-tied selections for one box"
    out = []
    for r in range(rounds):
        sel = selection.clone()
        for n, entries in per_box.items():
            combo = combos[n][r % len(combos[n])]
            for ((v, k), _), index in zip(entries, combo):
                sel[v, n, k] = index
        out.append(sel)
    return out


def epilogue_raw_gradients(raw, grad_instances, grad_raw_projection, weight_silhouette):
    """raw_gradients [N,8] of the epilogue: the instance-row adjoint [N,16] chained through the decode (autograd through
    geometry.decode_box_parameters), weighted, plus the projection gradient."""
    raw = raw.detach().clone().requires_grad_(True)
    instances, _ = decode(raw)
    chained, = torch.autograd.grad((instances * grad_instances).sum(), raw)
    return weight_silhouette * chained + grad_raw_projection
