"""Synthetic KITTI-360-shaped frames: what bench.py, the frame launcher and the full-size tests optimise when no
dataset is mounted.  Seeded, host-side, no GPU work: camera matrices and raw box parameters only."""
import math

import torch


def kitti_intrinsics(height, width):
    """The KITTI-360 perspective intrinsics of the 376 x 1408 images, scaled to the image size."""
    sx, sy = width / 1408.0, height / 376.0
    return torch.tensor([[552.554261 * sx, 0.0, 682.049453 * sx], [0.0, 552.554261 * sy, 238.769549 * sy], [0.0, 0.0, 1.0]])


_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))      # main.py:26-30


def clipped_boxes_2d(camera_corners, intrinsic_matrices, height, width, epsilon=1.0e-6):
    """project_box_3d + clip_boxes_to_image on the host, float64: camera-frame corners [L,N,8,3], K [L,3,3] -> boxes [L,N,4] (xmin, ymin,
    xmax, ymax); every edge is clipped to the front of the camera from its far end, a box without an edge in front is all zeros."""
    corners, K = camera_corners.double(), intrinsic_matrices.double()
    a, b = corners[:, :, [e[0] for e in _EDGES]], corners[:, :, [e[1] for e in _EDGES]]                     # [L,N,12,3]
    a_far = (a[..., 2] > b[..., 2])[..., None]
    far, near = torch.where(a_far, a, b), torch.where(a_far, b, a)
    t = (far[..., 2] / (far[..., 2] - near[..., 2]).clamp_min(epsilon)).clamp_max(1.0)[..., None]
    near = far + (near - far) * t
    front = far[..., 2] > 0.0                                                                               # [L,N,12]
    points = torch.stack([far, near], dim=-2) @ K[:, None, None].transpose(-1, -2)                          # [L,N,12,2,3]
    image = points[..., :2] / points[..., 2:3].clamp_min(epsilon)
    keep = front[..., None, None].expand_as(image)
    lo = torch.where(keep, image, torch.full_like(image, float("inf"))).flatten(2, 3).min(dim=2).values     # [L,N,2]
    hi = torch.where(keep, image, torch.full_like(image, float("-inf"))).flatten(2, 3).max(dim=2).values
    boxes = torch.cat([lo, hi], dim=-1)
    boxes = torch.where(front.any(dim=-1)[..., None], boxes, torch.zeros_like(boxes))
    limit = torch.tensor([width, height, width, height], dtype=torch.float64)
    return torch.minimum(boxes.clamp_min(0.0), limit)


def synthetic_group(frame, height, width, label_views, corners):
    """The GROUP of synthetic frame number `frame` (what a dataset's grouped_image_filenames.txt gives a real one: the frames that get the
    target's labels): `label_views` cameras on the frame's trajectory, the target first and the others at the half-metre marks
    -+0.5, -+1.5, ... along z -- never a source's position, which are whole metres -- with the trajectory's yaw of 0.5 degrees per metre.
    Their 2-D boxes are the true boxes `corners` [N,8,3] (target camera frame) projected and clipped; an instance is visible in a view
    where no corner comes closer than 0.1 m and the clipped box has area, and its box is zero elsewhere.  -> the five ``label_*`` members
    of a FrameInputs / FramePack as host tensors (ids int64: frame * 10000 + view)."""
    L = int(label_views)
    offsets = [0.0] + [sign * (i - 0.5) for i in range(1, L // 2 + 2) for sign in (1.0, -1.0)]
    K = kitti_intrinsics(height, width).expand(L, 3, 3).contiguous()
    E = torch.eye(4).repeat(L, 1, 1)
    for v, k in enumerate(offsets[:L]):
        yaw = math.radians(0.5 * k)
        E[v, :3, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
        E[v, 2, 3] = k
    camera = corners.double().cpu() @ E[:, None, :3, :3].double().transpose(-1, -2) + E[:, None, None, :3, 3].double()      # [L,N,8,3]
    boxes = clipped_boxes_2d(camera, K, height, width)
    visible = (camera[..., 2].min(dim=-1).values >= 0.1) & ((boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1]) > 0)
    boxes = boxes * visible[..., None]
    return dict(label_frame_ids=int(frame) * 10000 + torch.arange(L, dtype=torch.int64), label_intrinsic_matrices=K, label_extrinsic_matrices=E,
                label_boxes_2d=boxes.float(), label_visible=visible.to(torch.uint8))


def synthetic_frame(seed, num_views, height, width, num_instances):
    """KITTI-360 intrinsics, target E = I, sources shifted along z with a small yaw; raw box parameters ~ N(0, 0.5^2) with depth
    forced into 8-60 m.  Returns (K [V,3,3], E [V,4,4], raw locations [1,N,3], raw dimensions [1,N,3], raw orientations [1,N,2])."""
    g = torch.Generator().manual_seed(seed)
    K = kitti_intrinsics(height, width).expand(num_views, 3, 3).contiguous()
    E = torch.eye(4).repeat(num_views, 1, 1)
    half = (num_views - 1) // 2
    offsets = [0] + [k for i in range(1, half + 1) for k in (i, -i)]
    for v, k in enumerate(offsets[:num_views]):
        yaw = math.radians(0.5 * k)
        E[v, :3, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
        E[v, 2, 3] = 1.0 * k
    raw_loc = torch.randn(1, num_instances, 3, generator=g) * 0.5
    depth = torch.empty(num_instances).uniform_(8.0, 60.0, generator=g) / 100.0
    raw_loc[0, :, 2] = torch.log(depth / (1.0 - depth))            # sigmoid^-1, decoded z = 100 * sigmoid(raw)
    raw_dim = torch.randn(1, num_instances, 3, generator=g) * 0.5
    raw_ori = torch.nn.functional.normalize(torch.randn(1, num_instances, 2, generator=g), dim=-1)
    return K, E, raw_loc, raw_dim, raw_ori


def synthetic_images(frame, views, height, width):
    """Smooth deterministic colour images of synthetic frame number `frame` for the photometric term: per view and channel a sum of six
    sinusoids of period 24-64 px (texture a patch correlation can hold on to), quantised as image files are -- [V,3,H,W] uint8.  On the
    device they are x / 255 (optimization.FrameInputs.images; frames.pack_images for a pack that carries them)."""
    g = torch.Generator().manual_seed(7919 * int(frame) + 13)
    y, x = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    images = torch.zeros(views, 3, height, width)
    for _ in range(6):
        period = torch.empty(views, 3, 1, 1).uniform_(24.0, 64.0, generator=g)
        angle = torch.empty(views, 3, 1, 1).uniform_(0.0, 2.0 * math.pi, generator=g)
        phase = torch.empty(views, 3, 1, 1).uniform_(0.0, 2.0 * math.pi, generator=g)
        images += torch.sin(2.0 * math.pi * (x * torch.cos(angle) + y * torch.sin(angle)) / period + phase)
    return ((images / 12.0 + 0.5).clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
