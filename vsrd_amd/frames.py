"""Compact frame packs: what a dataset keeps per target frame -- one polygon and one binary mask per (view, instance), camera
matrices -- as one ``.npz`` file, and its way onto the device.

The reference does not store soft masks either: its dataset keeps the masks, ``SoftRasterizer`` builds the soft masks from their
polygons (vsrd/transforms/geometric_transforms.py:233-317), ``BoxGenerator`` the 2-D boxes (:140-167), and scripts/main.py:204-265
re-indexes every source view to the target's instance order.  A materialised ``FrameInputs`` is 36 MB per instance at 17 x 376 x 1408;
a pack is the polygons plus one BIT per pixel and entry (about 9 MB for 136 entries).  ``vsrd_frame_ingest`` (csrc/frame_ingest.h) turns
a pack into soft masks, importance weights, boxes and visibility in one call: ``ingest`` materialises a ``FrameInputs`` with it, and
``FrameOptimizer.reset`` / ``FrameBatch.reset`` let it write straight into a persistent row (``ingest_into``)."""
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_VIEWS = 32                 # the frame glue's limit (csrc/host_checks.h: kFrameMaxViews)
TEMPERATURE = 10.0             # SoftRasterizer's default (geometric_transforms.py:235)

_FIELDS = ("image_size", "intrinsic_matrices", "extrinsic_matrices", "view_offsets", "instance_ids", "polygon_offsets", "polygon_vertices",
           "inside")
# optional members (3-D ground truth for FrameOptimizer.metrics): written only when present; a pack without them loads with None
_OPTIONAL = ("boxes_3d", "rectification_matrix")
# optional members, all or none: the frame's GROUP (tools/kitti_360/make_predictions.py:50-60: the frames whose filtered instance-id set equals
# the target's -- the frames that get labels, FrameOptimizer.group_labels), L label views with their cameras and 2-D boxes; (field, dtype)
_GROUP = (("label_frame_ids", np.int64), ("label_intrinsic_matrices", np.float32), ("label_extrinsic_matrices", np.float32),
          ("label_boxes_2d", np.float32), ("label_visible", np.uint8))
MAX_LABEL_VIEWS = _lib.MAX_LABEL_VIEWS         # VSRD_MAX_LABEL_VIEWS


@dataclass
class FramePack:
    """One target frame, host side, numeric arrays only.  An ENTRY is one (view, instance) pair; the entries of all views are
    concatenated, view 0 being the target.  The target's entries define N and the instance order; a source entry whose id the target
    does not have is ignored, a target id missing from a view is invisible there."""
    image_size: Sequence[int]               # (H, W)
    intrinsic_matrices: np.ndarray          # [V,3,3] float32
    extrinsic_matrices: np.ndarray          # [V,4,4] float32, relative to the target as FrameInputs defines them
    view_offsets: np.ndarray                # [V+1] int64: view v's entries are view_offsets[v] .. view_offsets[v+1] - 1
    instance_ids: np.ndarray                # [M] int64
    polygon_offsets: np.ndarray             # [M+1] int64: entry m's vertices are polygon_offsets[m] .. polygon_offsets[m+1] - 1
    polygon_vertices: np.ndarray            # [sum P,2] int32 (x, y): cv.findContours' output (SoftRasterizer.make_polygon)
    inside: np.ndarray                      # [M,H,ceil(W/8)] uint8: np.packbits(binary mask, axis=-1), most significant bit first
    boxes_3d: Optional[np.ndarray] = None               # [N,8,3] float32 or None: 3-D ground truth in the target's instance order, NaN rows = no annotation
    rectification_matrix: Optional[np.ndarray] = None   # [3,3] float32 or None (identity)
    # the frame's group (all five, or none): the frames make_predictions.py labels, the target among them
    label_frame_ids: Optional[np.ndarray] = None            # [L] int64, unique: the files' names (<id:010d>)
    label_intrinsic_matrices: Optional[np.ndarray] = None   # [L,3,3] float32
    label_extrinsic_matrices: Optional[np.ndarray] = None   # [L,4,4] float32, relative to the rectified target like extrinsic_matrices
    label_boxes_2d: Optional[np.ndarray] = None             # [L,N,4] float32 (xmin, ymin, xmax, ymax) in the target's instance order, zeros where invisible
    label_visible: Optional[np.ndarray] = None              # [L,N] uint8
    # the views' colour images, for the photometric term (optimization.FrameInputs.images); written only when present
    images: Optional[np.ndarray] = None                     # [V,3,H,W] uint8; on the device float32 x / 255 (pack_images)

    @property
    def num_label_views(self):
        """L, or 0 for a pack without a group."""
        return 0 if self.label_frame_ids is None else len(self.label_frame_ids)

    @property
    def num_views(self):
        return len(self.view_offsets) - 1

    @property
    def num_instances(self):
        return int(self.view_offsets[1] - self.view_offsets[0])


def unpack_masks(inside, width):
    """Bit-packed masks [M,H,ceil(W/8)] (FramePack.inside; also what vsrd_frame_masks writes) as booleans [M,H,W]."""
    inside = np.asarray(inside, dtype=np.uint8)
    if inside.shape[-1] != (int(width) + 7) // 8:
        raise ValueError(f"rows of {inside.shape[-1]} bytes do not hold {width} pixels")
    return np.unpackbits(inside, axis=-1)[..., :int(width)].astype(bool)


def _normalised(pack):
    height, width = (int(x) for x in np.asarray(pack.image_size).reshape(-1))
    return FramePack((height, width),
                     np.ascontiguousarray(pack.intrinsic_matrices, dtype=np.float32), np.ascontiguousarray(pack.extrinsic_matrices, dtype=np.float32),
                     np.ascontiguousarray(pack.view_offsets, dtype=np.int64), np.ascontiguousarray(pack.instance_ids, dtype=np.int64),
                     np.ascontiguousarray(pack.polygon_offsets, dtype=np.int64), np.ascontiguousarray(pack.polygon_vertices, dtype=np.int32),
                     np.ascontiguousarray(pack.inside, dtype=np.uint8),
                     *[None if getattr(pack, field) is None else np.ascontiguousarray(getattr(pack, field), dtype=np.float32) for field in _OPTIONAL],
                     *[None if getattr(pack, field) is None else np.ascontiguousarray(getattr(pack, field), dtype=dtype) for field, dtype in _GROUP],
                     images=None if pack.images is None else np.ascontiguousarray(pack.images))


def validate(pack, name="frame pack"):
    """ValueError (naming `name`) unless the pack is well formed: shapes, monotone offsets, every polygon with at least one vertex,
    1 <= N <= VSRD_MAX_INSTANCES, V within the frame glue's limit, no id twice in a view."""
    def bad(why):
        raise ValueError(f"{name}: malformed frame pack: {why}")
    for field in _FIELDS[1:]:
        array = getattr(pack, field)
        if not isinstance(array, np.ndarray) or array.dtype == object:
            bad(f"{field} is not a numeric array")
    if len(pack.image_size) != 2 or min(pack.image_size) < 1:
        bad(f"image_size {tuple(pack.image_size)}")
    height, width = (int(x) for x in pack.image_size)
    offsets, ids, sides = pack.view_offsets, pack.instance_ids, pack.polygon_offsets
    if offsets.ndim != 1 or len(offsets) < 2:
        bad(f"view_offsets of shape {offsets.shape}")
    views = len(offsets) - 1
    if views > MAX_VIEWS:
        bad(f"{views} views, at most {MAX_VIEWS}")
    if pack.intrinsic_matrices.shape != (views, 3, 3) or pack.extrinsic_matrices.shape != (views, 4, 4):
        bad(f"camera matrices of shapes {pack.intrinsic_matrices.shape}, {pack.extrinsic_matrices.shape} for {views} views")
    if ids.ndim != 1:
        bad(f"instance_ids of shape {ids.shape}")
    entries = len(ids)
    if offsets[0] != 0 or offsets[-1] != entries or np.any(np.diff(offsets) < 0):
        bad(f"view_offsets {offsets.tolist()} do not partition {entries} entries")
    if not 1 <= int(offsets[1]) <= _lib.MAX_INSTANCES:
        bad(f"{int(offsets[1])} target instances, 1..{_lib.MAX_INSTANCES}")
    if sides.ndim != 1 or len(sides) != entries + 1:
        bad(f"polygon_offsets of shape {sides.shape} for {entries} entries")
    if pack.polygon_vertices.ndim != 2 or pack.polygon_vertices.shape[1] != 2:
        bad(f"polygon_vertices of shape {pack.polygon_vertices.shape}")
    if sides[0] != 0 or sides[-1] != len(pack.polygon_vertices) or np.any(np.diff(sides) < 1):
        bad("polygon_offsets are not increasing from 0 to the vertex count (every polygon needs at least one vertex)")
    if len(pack.polygon_vertices) >= 2 ** 31:
        bad("too many vertices")
    if pack.inside.shape != (entries, height, (width + 7) // 8):
        bad(f"inside of shape {pack.inside.shape}, expected {(entries, height, (width + 7) // 8)}")
    for view in range(views):
        own = ids[offsets[view]:offsets[view + 1]]
        if len(np.unique(own)) != len(own):
            bad(f"view {view} lists an instance id twice")
    for field, shape in zip(_OPTIONAL, ((int(offsets[1]), 8, 3), (3, 3))):
        array = getattr(pack, field)
        if array is None:
            continue
        if not isinstance(array, np.ndarray) or array.dtype.kind not in "iuf":
            bad(f"{field} is not a numeric array")
        if array.shape != shape:
            bad(f"{field} of shape {array.shape}, expected {shape}")
    group = {field: getattr(pack, field) for field, _ in _GROUP}
    present = [field for field, array in group.items() if array is not None]
    if present and len(present) != len(_GROUP):
        bad(f"a group needs all of {', '.join(field for field, _ in _GROUP)}: only {', '.join(present)} given")
    if present:
        for field, array in group.items():
            if not isinstance(array, np.ndarray) or array.dtype.kind not in "iuf":
                bad(f"{field} is not a numeric array")
        label_ids = group["label_frame_ids"]
        if label_ids.ndim != 1 or label_ids.dtype.kind not in "iu":
            bad(f"label_frame_ids of shape {label_ids.shape}, dtype {label_ids.dtype}: expected [L] integers")
        count, instances = len(label_ids), int(offsets[1])
        if not 1 <= count <= MAX_LABEL_VIEWS:
            bad(f"{count} label views, 1..{MAX_LABEL_VIEWS}")
        if len(np.unique(label_ids)) != count:
            bad("label_frame_ids lists a frame id twice")
        shapes = dict(label_intrinsic_matrices=(count, 3, 3), label_extrinsic_matrices=(count, 4, 4), label_boxes_2d=(count, instances, 4),
                      label_visible=(count, instances))
        for field, shape in shapes.items():
            if group[field].shape != shape:
                bad(f"{field} of shape {group[field].shape}, expected {shape}")
    if pack.images is not None:
        if not isinstance(pack.images, np.ndarray) or pack.images.dtype != np.uint8:
            bad(f"images is not a uint8 array (dtype {getattr(pack.images, 'dtype', type(pack.images))})")
        if pack.images.shape != (views, 3, height, width):
            bad(f"images of shape {pack.images.shape}, expected {(views, 3, height, width)}")
    return pack


def save_pack(path, pack):
    """Write `pack` as an .npz, atomically (a reader sees the old file or the whole new one)."""
    pack = validate(_normalised(pack), str(path))
    staged = f"{path}.tmp.{os.getpid()}"
    try:
        with open(staged, "wb") as handle:
            members = _FIELDS + _OPTIONAL + tuple(field for field, _ in _GROUP) + ("images",)
            np.savez(handle, **{field: np.asarray(getattr(pack, field)) for field in members if getattr(pack, field) is not None})
        os.replace(staged, path)
    finally:
        if os.path.exists(staged):
            os.remove(staged)


def _open(path):
    try:
        return np.load(path, allow_pickle=False)
    except Exception as error:          # (not a zip archive, truncated, ...)
        raise ValueError(f"{path}: not a readable frame pack: {error}") from error


def _member(data, path, field):
    if field not in data.files:
        raise ValueError(f"{path}: malformed frame pack: no {field}")
    try:
        return data[field]
    except Exception as error:          # (an object array: allow_pickle=False refuses it)
        raise ValueError(f"{path}: malformed frame pack: {field} cannot be read without pickle: {error}") from error


def load_pack(path):
    """Read and validate a pack; ValueError naming the file when it is malformed."""
    with _open(path) as data:
        arrays = {field: _member(data, path, field) for field in _FIELDS}
        arrays.update({field: _member(data, path, field) for field in _OPTIONAL + tuple(f for f, _ in _GROUP) + ("images",) if field in data.files})
    if arrays["image_size"].size != 2:
        raise ValueError(f"{path}: malformed frame pack: image_size of shape {arrays['image_size'].shape}")
    for field in arrays:
        if arrays[field].dtype.kind not in "iuf":
            raise ValueError(f"{path}: malformed frame pack: {field} has dtype {arrays[field].dtype}")
    return validate(_normalised(FramePack(**arrays)), str(path))


def pack_counts(path):
    """(V, H, W, N) of the pack at `path` without loading its masks."""
    with _open(path) as data:
        size, offsets = _member(data, path, "image_size"), _member(data, path, "view_offsets")
    if size.size != 2 or offsets.ndim != 1 or len(offsets) < 2 or offsets.dtype.kind not in "iu":
        raise ValueError(f"{path}: malformed frame pack: image_size {size.shape}, view_offsets {offsets.shape}")
    height, width = (int(x) for x in size.reshape(-1))
    return len(offsets) - 1, height, width, int(offsets[1] - offsets[0])


def pack_label_views(path):
    """L of the pack at `path` -- the label views of its group -- without loading anything else; 0 for a pack without a group."""
    with _open(path) as data:
        if "label_frame_ids" not in data.files:
            return 0
        label_ids = _member(data, path, "label_frame_ids")
    if label_ids.ndim != 1:
        raise ValueError(f"{path}: malformed frame pack: label_frame_ids of shape {label_ids.shape}")
    return len(label_ids)


def pack_has_images(path):
    """Whether the pack at `path` carries the views' images, without loading anything."""
    with _open(path) as data:
        return "images" in data.files


def pack_images(pack, device):
    """The pack's images on `device` as FrameInputs.images defines them -- [V,3,H,W] float32, x / 255 -- or None for a pack without them.
    The ONE conversion: frames.ingest and a row's reset(FramePack) both come through here, so the two routes give the same gray planes."""
    if pack.images is None:
        return None
    return torch.from_numpy(pack.images).to(device).to(torch.float32) / 255.0


def collate_tables(pack):
    """[V,N] int32: the entry of (view, target slot), -1 where the view does not have the target's instance -- the re-indexing of
    scripts/main.py:204-255 (every view's masks and boxes selected by the index of the target's id, index -1 being the zero padding)."""
    offsets, ids = pack.view_offsets, pack.instance_ids
    target = ids[offsets[0]:offsets[1]]
    table = np.full((pack.num_views, len(target)), -1, dtype=np.int32)
    for view in range(pack.num_views):
        where = {int(instance): int(offsets[view]) + j for j, instance in enumerate(ids[offsets[view]:offsets[view + 1]])}
        for slot, instance in enumerate(target):
            table[view, slot] = where.get(int(instance), -1)
    return table


def staging_chunk():
    """Polygon sides the ingest kernel stages per round (csrc/frame_ingest.h, kIngestChunk)."""
    return int(_lib.load().vsrd_frame_ingest_chunk())


def ingest_into(pack, device, target_stride, soft_masks=None, sampling_weights=None, gt_boxes=None, visible=None, temperature=TEMPERATURE):
    """ONE ``vsrd_frame_ingest`` call on the current stream: the pack's polygons, table and bits go to the device (four small copies)
    and the kernel writes instances 0..N-1 of the given device buffers -- soft_masks [V*H*W, target_stride] float32, sampling_weights
    [V*H*W] float32, gt_boxes [V, target_stride, 4] float32, visible [V, target_stride] uint8; any may be None."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.VsrdHipError("vsrd_amd operates on HIP device tensors only; there is no CPU fallback")
    height, width = (int(x) for x in pack.image_size)
    views, instances, stride = pack.num_views, pack.num_instances, int(target_stride)
    pixels = views * height * width
    expected = dict(soft_masks=(soft_masks, pixels * stride, torch.float32), sampling_weights=(sampling_weights, pixels, torch.float32),
                    gt_boxes=(gt_boxes, views * stride * 4, torch.float32), visible=(visible, views * stride, torch.uint8))
    for name, (tensor, count, dtype) in expected.items():
        if tensor is not None and (tensor.device != device or tensor.dtype != dtype or tensor.numel() != count or not tensor.is_contiguous()):
            raise ValueError(f"{name}: a contiguous {dtype} tensor of {count} elements on {device} (row stride {stride})")
    vertices = torch.from_numpy(pack.polygon_vertices).to(device)
    offsets = torch.from_numpy(pack.polygon_offsets.astype(np.int32)).to(device)
    table = torch.from_numpy(collate_tables(pack)).to(device)
    bits = torch.from_numpy(pack.inside).to(device)
    pointer = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().vsrd_frame_ingest(vertices.data_ptr(), int(vertices.shape[0]), offsets.data_ptr(), int(offsets.shape[0]) - 1, table.data_ptr(),
                                             bits.data_ptr(), height, width, views, instances, stride, float(temperature), pointer(soft_masks),
                                             pointer(sampling_weights), pointer(gt_boxes), pointer(visible), _lib.stream()))
    for staged in (vertices, offsets, table, bits):          # (the kernel may still be running: the allocator must not hand the block to another stream)
        staged.record_stream(torch.cuda.current_stream(device))


def ground_truth_3d(pack, device):
    """(boxes_3d [N,8,3], rectification_matrix [3,3]) of the pack on `device`, None where the pack has none."""
    return tuple(None if array is None else torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(device)
                 for array in (pack.boxes_3d, pack.rectification_matrix))


def group_tables(pack, device):
    """The pack's group on `device` as FrameInputs' keyword arguments (label_frame_ids, ... label_visible); {} for a pack without one."""
    if pack.label_frame_ids is None:
        return {}
    return {field: torch.from_numpy(np.ascontiguousarray(getattr(pack, field), dtype=dtype)).to(device) for field, dtype in _GROUP}


def camera_matrices(pack, device):
    return (torch.from_numpy(pack.intrinsic_matrices).to(device=device, dtype=torch.float32),
            torch.from_numpy(pack.extrinsic_matrices).to(device=device, dtype=torch.float32))


def ingest(pack, device, temperature=TEMPERATURE):
    """The pack as a materialised ``FrameInputs`` on `device`: soft masks [V,H,W,N], boxes [V,N,2,2] and visibility [V,N] from one
    ``vsrd_frame_ingest`` call (eager loops, the construction of a ``FrameOptimizer``, founders of slots and batches)."""
    from .optimization import FrameInputs
    device = torch.device(device)
    height, width = (int(x) for x in pack.image_size)
    views, instances = pack.num_views, pack.num_instances
    soft = torch.empty(views, height, width, instances, dtype=torch.float32, device=device)
    boxes = torch.empty(views, instances, 4, dtype=torch.float32, device=device)
    visible = torch.empty(views, instances, dtype=torch.uint8, device=device)
    ingest_into(pack, device, instances, soft_masks=soft, gt_boxes=boxes, visible=visible, temperature=temperature)
    intrinsics, extrinsics = camera_matrices(pack, device)
    return FrameInputs((height, width), intrinsics, extrinsics, soft, boxes.reshape(views, instances, 2, 2), visible.bool(),
                       *ground_truth_3d(pack, device), **group_tables(pack, device), images=pack_images(pack, device))
