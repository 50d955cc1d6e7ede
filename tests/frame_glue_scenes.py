"""Scenes of the frame-glue tests (test_frame_glue_reference.py on the host, test_hip_frame_glue.py on the GPU): deterministic, built from
vsrd_amd.synthetic.synthetic_frame at 376 x 1408.  The ground truth is the frame's own boxes in a permuted instance order with ~15 % of the
(view, instance) pairs invisible; the raw parameters handed to the kernels are those boxes perturbed by ~3e-2, with orientation norms in
0.5 .. 2.  A few ground-truth boxes are placed by hand (see `build`)."""
import torch

from oracle import frame_glue as ref
from vsrd_amd import synthetic

IMAGE_SIZE = (376, 1408)
WEIGHTS = (0.1, 1.0)                       # iou, l1 projection loss (config.json:120-127)

# (V, N): seed.  8x32 and 4x64 are the LDS path at its limit of 256 pairs; the rest runs through the global scratch.
SHAPES = {(8, 32): 1, (4, 64): 3, (17, 16): 2, (17, 20): 1, (32, 9): 1, (17, 64): 1, (32, 64): 2, (1, 64): 0}
UNMATCHABLE = (17, 64, 2)                  # (V, N, seed) of the scene whose target-view costs hold NaN


def box_tolerance(floor):
    """How far a float32 2-D box coordinate may be from the float64 one: twice the float32 oracle's own distance plus the float32 spacing
    of the largest coordinate (1408 px: 2^-13)."""
    return 2.0 * floor + 2.0 ** -13


def build(V, N, seed, matchable=True):
    """-> dict of float64 host tensors: raw [N,8], E [V,4,4], K [V,3,3], gt_boxes [V,N,4], visible [V,N] (bool)."""
    K, E, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(seed, V, *IMAGE_SIZE, N)
    K, E = K.double(), E.double()
    truth = torch.cat([raw_loc[0], raw_dim[0], raw_ori[0]], dim=-1).double()
    if V >= 17:
        # placed by hand: box 1 stands 3 m in front of the target camera, near its axis -- behind the source cameras that stand 4 .. 8 m
        # further along z, and across z = 0 of the one that stands 3 m further (17 views reach no box of the frame's own 8 .. 60 m)
        truth[1, 2] = torch.logit(torch.tensor(0.03, dtype=torch.float64))
        truth[1, 0:2] *= 0.1
    if matchable:
        # a box that the target view does not see at all has a zero-area ground truth AND a zero-area prediction there: their DIoU is
        # 0 / 0 and the reference's matcher raises.  Such boxes are pulled towards the optical axis until the target view sees them.
        for _ in range(8):
            boxes = ref.forward(truth, E[:1], K[:1], IMAGE_SIZE)["boxes"][0]
            empty = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) <= 0
            if not bool(empty.any()):
                break
            truth[empty, 0:2] *= 0.5
    g = torch.Generator().manual_seed(1000 + seed)
    order = torch.randperm(N, generator=g)                     # ground-truth column c holds box order[c]
    visible = torch.rand(V, N, generator=g) > 0.15
    raw = truth + 3.0e-2 * torch.randn(N, 8, generator=g, dtype=torch.float64)
    raw[:, 6:8] *= 0.5 + 1.5 * torch.rand(N, 1, generator=g, dtype=torch.float64)
    gt_boxes = ref.forward(truth, E, K, IMAGE_SIZE)["boxes"]
    # Placed by hand, on the prediction's own float64 boxes: (a) every fourth box gets a ground truth a fraction of a pixel from its
    # prediction, so that smooth-L1 is in its quadratic branch there; (b) no ground-truth coordinate lies within 0.05 px of its
    # prediction's unless both sit on the image border -- the DIoU gradient jumps where a predicted and a ground-truth coordinate
    # swap order, and float32 (3e-4 .. 1e-3 px off) may not be asked on which side of such a jump it is.
    limit = torch.tensor([IMAGE_SIZE[1], IMAGE_SIZE[0], IMAGE_SIZE[1], IMAGE_SIZE[0]], dtype=torch.float64)
    predicted = ref.forward(raw, E, K, IMAGE_SIZE)["boxes"]
    offsets = torch.tensor([0.3, -0.4, 0.5, -0.25], dtype=torch.float64)
    gt_boxes[:, ::4] = torch.minimum(torch.maximum(predicted[:, ::4] + offsets, torch.zeros(4, dtype=torch.float64)), limit)
    difference = (gt_boxes - predicted).abs()
    close = (difference > 0) & (difference < 0.05)
    gt_boxes = torch.where(close, torch.where(gt_boxes + 0.25 <= limit, gt_boxes + 0.25, gt_boxes - 0.25), gt_boxes)
    gt_boxes = gt_boxes[:, order] * visible[..., None]
    return dict(raw=raw, E=E, K=K, gt_boxes=gt_boxes.contiguous(), visible=visible)


def conditions(scene, forward, assignment):
    """What the scene holds, on the float64 reference: counts of (view, box) pairs of every kind."""
    cam_z = forward["cam"][..., 2]
    boxes = forward["boxes"]
    area = (boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1])
    kept = scene["visible"][:, assignment]
    difference = (boxes - scene["gt_boxes"][:, assignment]).abs()[kept]
    return dict(behind=int(forward["behind"].sum()),
                straddling=int(((cam_z.min(-1).values < 0) & (cam_z.max(-1).values > 0)).sum()),
                outside=int((~forward["behind"] & (area == 0)).sum()),
                invisible=int((~kept).sum()),
                quadratic=int(((difference > 0) & (difference < 1.0)).sum()), linear=int((difference > 1.0).sum()),
                near_ties=int(((difference > 0) & (difference < 0.01)).sum()))
