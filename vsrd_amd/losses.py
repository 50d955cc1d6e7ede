"""The losses scripts/main.py assembles inline on the hot path, as device-side functions (torch element-wise ops on
small tensors; the heavy lifting -- rendering -- is in the HIP library).

  matching + projection losses    scripts/main.py:374-415   (torchvision.ops.distance_box_iou / _loss restated: the
                                                              reference pins torchvision==0.14.0, environment.yaml:368)
  schedules                       scripts/main.py:420-431
  silhouette / eikonal            scripts/main.py:653-687
  weights                         configs/.../config.json:120-127
  photometric (patch correlation) scripts/main.py:783-851   (HIP: csrc/patch_correlation.h; FrameOptimizer applies it when its weight is non-zero)
"""
import math

import torch
import torch.nn.functional as F

LOSS_WEIGHTS = dict(silhouette_loss=1.0, l1_projection_loss=1.0, iou_projection_loss=0.1, eikonal_loss=0.01, photometric_loss=0.0)


def cosine_annealing(x, start, end):
    return (math.cos(math.pi * x) + 1.0) / 2.0 * (start - end) + end


def schedules(step, num_steps, max_temperature=1.0, min_temperature=0.1, max_std=1.0, min_std=0.1):
    """-> (cosine_ratio, sdf_union_temperature, sdf_std_deviation), main.py:420-431."""
    x = step / num_steps
    return x, cosine_annealing(x, max_temperature, min_temperature), cosine_annealing(x, max_std, min_std)


def _split(boxes):
    boxes = boxes.flatten(-2, -1) if boxes.shape[-1] == 2 else boxes
    return boxes.unbind(-1)


def distance_box_iou(boxes1, boxes2, eps=1e-7):
    """Pairwise DIoU [N,*] x [M,*] -> [N,M] (boxes as [.,4] or [.,2,2])."""
    x1, y1, x2, y2 = (c[:, None] for c in _split(boxes1))
    x1g, y1g, x2g, y2g = (c[None, :] for c in _split(boxes2))
    inter = (torch.min(x2, x2g) - torch.max(x1, x1g)).clamp_min(0) * (torch.min(y2, y2g) - torch.max(y1, y1g)).clamp_min(0)
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    diagonal = (torch.max(x2, x2g) - torch.min(x1, x1g)).clamp_min(0) ** 2 + (torch.max(y2, y2g) - torch.min(y1, y1g)).clamp_min(0) ** 2 + eps
    centres = ((x1 + x2) - (x1g + x2g)) ** 2 / 4 + ((y1 + y2) - (y1g + y2g)) ** 2 / 4
    return inter / union - centres / diagonal


def distance_box_iou_loss(boxes1, boxes2, eps=1e-7):
    """Element-wise DIoU loss (reduction='none') on matched boxes [...,4] / [...,2,2]."""
    x1, y1, x2, y2 = _split(boxes1)
    x1g, y1g, x2g, y2g = _split(boxes2)
    ix1, iy1, ix2, iy2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
    inter = torch.where((iy2 > iy1) & (ix2 > ix1), (ix2 - ix1) * (iy2 - iy1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    diagonal = (torch.max(x2, x2g) - torch.min(x1, x1g)) ** 2 + (torch.max(y2, y2g) - torch.min(y1, y1g)) ** 2 + eps
    centres = ((x1 + x2) / 2 - (x1g + x2g) / 2) ** 2 + ((y1 + y2) / 2 - (y1g + y2g) / 2) ** 2
    return 1 - inter / (union + eps) + centres / diagonal


def linear_sum_assignment(cost):
    """scipy.optimize.linear_sum_assignment(cost) for a device matrix [P,G] (P, G <= 64) without leaving the device
    (vsrd_linear_sum_assignment: the same shortest-augmenting-path algorithm and tie rule, float64 duals)."""
    from . import _lib
    lib = _lib.load()
    cost = cost.detach().to(torch.float32).contiguous()
    P, G = cost.shape
    rows = torch.empty(min(P, G), dtype=torch.int64, device=cost.device)
    cols = torch.empty_like(rows)
    _lib.check(lib.vsrd_linear_sum_assignment(_lib.ptr(cost), P, G, rows.data_ptr(), cols.data_ptr(), _lib.stream()))
    return rows, cols


def match_instances(pd_boxes_2d, gt_boxes_2d):
    """main.py:374-386: Hungarian assignment on -DIoU of the target view.  The reference copies the cost matrix to the host for
    scipy (one synchronisation per step); here both the cost and the assignment stay on the device (vsrd_match_boxes), so the
    optimisation step has no host round trip and can be captured in a hipGraph."""
    from . import _lib
    lib = _lib.load()
    pd = pd_boxes_2d.detach().reshape(-1, 4).to(torch.float32).contiguous()
    gt = gt_boxes_2d.detach().reshape(-1, 4).to(torch.float32).contiguous()
    P, G = pd.shape[0], gt.shape[0]
    pd_idx = torch.empty(min(P, G), dtype=torch.int64, device=pd.device)
    gt_idx = torch.empty_like(pd_idx)
    _lib.check(lib.vsrd_match_boxes(_lib.ptr(pd), _lib.ptr(gt), P, G, pd_idx.data_ptr(), gt_idx.data_ptr(), _lib.stream()))
    return pd_idx, gt_idx


def projection_losses(pd_boxes_2d, gt_boxes_2d, visible_masks, pd_idx, gt_idx):
    """main.py:391-415 for all views at once: pd/gt [V,N,2,2], visible_masks [V,N] (by gt instance) -> (iou_loss, l1_loss).

    The reference concatenates the kept rows of every view and takes the mean; a masked mean over [V,M] is the same number.
    """
    pd = pd_boxes_2d[:, pd_idx].flatten(-2, -1)                      # [V,M,4]
    gt = gt_boxes_2d[:, gt_idx].flatten(-2, -1)
    keep = visible_masks[:, gt_idx].to(pd.dtype)                     # [V,M]
    count = keep.sum().clamp_min(1.0)
    iou = (distance_box_iou_loss(pd, gt) * keep).sum() / count
    l1 = (F.smooth_l1_loss(pd, gt, reduction="none") * keep.unsqueeze(-1)).sum() / (count * 4.0)
    return iou, l1


def silhouette_loss(labels, targets, pd_idx=None, gt_idx=None):
    """main.py:653-671."""
    if pd_idx is not None:
        labels, targets = labels[..., pd_idx], targets[..., gt_idx]
    return F.binary_cross_entropy(labels.clamp(1.0e-6, 1.0 - 1.0e-6), targets, reduction="none").mean()


def eikonal_loss(gradients):
    """main.py:679-687."""
    return ((gradients.norm(dim=-1) - 1.0) ** 2).mean()


# ---- photometric loss: the homography / patch-correlation part (main.py:783-851) ---------------------------------------------------
def grayscale_images(images):
    """images [V,3,H,W] in [0,1] -> the gray planes [V,H,W] float32 (vsrd_grayscale_images: torchvision's rgb_to_grayscale weights).
    Once per frame: `patch_correlation_loss` takes the planes in place of the images and skips the conversion on every call."""
    from . import _lib
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images must be [V,3,H,W], got {tuple(images.shape)}")
    images = images.detach().to(torch.float32).contiguous()
    V, _, H, W = images.shape
    gray = torch.empty(V, H, W, dtype=torch.float32, device=images.device)
    _lib.check(_lib.load().vsrd_grayscale_images(_lib.ptr(images), V, H, W, _lib.ptr(gray), _lib.stream()))
    return gray


class _PatchCorrelation(torch.autograd.Function):
    """vsrd_patch_correlation_forward / _backward: the loss as a [1] tensor (and the exported patches), gradients to positions and normals."""

    @staticmethod
    def forward(ctx, positions, normals, gray, intrinsics, extrinsics, pixels, converged, meta, want_patches):
        from . import _lib
        from .rendering.renderers import current_workspace
        lib = _lib.load()
        V, H, W = gray.shape
        R = positions.shape[0]
        pw, ph, top_k, target = meta
        config = _lib.PatchCorrelationConfig(V, R, H, W, pw, ph, top_k, target, 1.0e-6, 1.0e-12)
        positions, normals = positions.detach().contiguous(), normals.detach().contiguous()
        workspace = current_workspace().patch_correlation(gray.device, V, R, pw * ph)
        loss = torch.empty(1, dtype=torch.float32, device=gray.device)
        stats = torch.empty(2, dtype=torch.float32, device=gray.device)
        patches = torch.empty(V, R, pw * ph, dtype=torch.float32, device=gray.device) if want_patches else None
        _lib.check(lib.vsrd_patch_correlation_forward(config, _lib.ptr(gray), _lib.ptr(intrinsics), _lib.ptr(extrinsics), _lib.iptr(pixels),
                                                      _lib.ptr(positions), _lib.ptr(normals), converged.data_ptr(), workspace.data_ptr(),
                                                      workspace.numel(), _lib.ptr(loss), _lib.ptr(stats), _lib.ptr(patches), None, None, _lib.stream()))
        ctx.save_for_backward(positions, normals, gray, intrinsics, extrinsics, pixels, converged, stats)
        ctx.config, ctx.workspace = config, workspace
        if want_patches:
            ctx.mark_non_differentiable(patches)
        return loss, patches

    @staticmethod
    def backward(ctx, grad_loss, _grad_patches):
        from . import _lib
        positions, normals, gray, intrinsics, extrinsics, pixels, converged, stats = ctx.saved_tensors
        grad_loss = grad_loss.detach().to(torch.float32).contiguous()
        grad_positions, grad_normals = torch.empty_like(positions), torch.empty_like(normals)
        workspace = ctx.workspace
        _lib.check(_lib.load().vsrd_patch_correlation_backward(
            ctx.config, _lib.ptr(gray), _lib.ptr(intrinsics), _lib.ptr(extrinsics), _lib.iptr(pixels), _lib.ptr(positions), _lib.ptr(normals),
            converged.data_ptr(), workspace.data_ptr(), workspace.numel(), _lib.ptr(stats), _lib.ptr(grad_loss), _lib.ptr(grad_positions),
            _lib.ptr(grad_normals), _lib.stream()))
        return grad_positions, grad_normals, None, None, None, None, None, None, None


def patch_correlation_loss(images, intrinsic_matrices, extrinsic_matrices, pixel_indices, positions, normals, convergence_masks,
                           patch_size=(11, 11), top_k=4, target_view=0, return_patches=False):
    """main.py:783-851 in one call: the multi-view patch-correlation photometric loss of one frame (include/vsrd_hip.h has what is
    computed, the reference's quirks and the two stated deviations: gray before interpolation, loss 0 when no ray converged).

    `images` [V,3,H,W] (converted on every call) or the gray planes [V,H,W] of `grayscale_images`; `intrinsic_matrices` [V,3,3];
    `extrinsic_matrices` [V,4,4]; `pixel_indices` the reference's flat target_ray_indices (x = i % W, y = i // W); `positions`,
    `normals` [R,3] or with the reference's leading dimensions [1,R,3], in the frame of the extrinsics' input; `convergence_masks` [R],
    [R,1] or [1,R,1]; `patch_size` (width, height).  Returns the loss as a 0-dim tensor with gradients to `positions` and `normals`
    (none to images or cameras), and with `return_patches` the sampled patches [V,R,P] beside it.  The workspace is the active
    `rendering.workspace_scope`'s."""
    gray = images if images.dim() == 3 else grayscale_images(images)
    gray = gray.detach().to(torch.float32).contiguous()
    V, H, W = gray.shape
    intrinsics = intrinsic_matrices.detach().reshape(-1, 3, 3).to(torch.float32).contiguous()
    extrinsics = extrinsic_matrices.detach().reshape(-1, 4, 4).to(torch.float32).contiguous()
    if intrinsics.shape[0] != V or extrinsics.shape[0] != V:
        raise ValueError(f"{V} images need {V} intrinsic and extrinsic matrices, got {intrinsics.shape[0]} and {extrinsics.shape[0]}")
    indices = pixel_indices.detach().reshape(-1)
    pixels = torch.stack([indices % W, indices // W], dim=-1).to(torch.int32).contiguous()
    R = pixels.shape[0]
    positions, normals = positions.reshape(-1, 3).to(torch.float32), normals.reshape(-1, 3).to(torch.float32)
    converged = convergence_masks.detach().reshape(-1).to(torch.uint8).contiguous()
    if positions.shape[0] != R or normals.shape[0] != R or converged.shape[0] != R:
        raise ValueError(f"{R} pixels need {R} positions, normals and convergence flags")
    meta = (int(patch_size[0]), int(patch_size[1]), int(top_k), int(target_view))
    loss, patches = _PatchCorrelation.apply(positions, normals, gray, intrinsics, extrinsics, pixels, converged, meta, bool(return_patches))
    loss = loss.reshape(())
    return (loss, patches) if return_patches else loss
