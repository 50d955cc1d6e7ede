"""On-disk formats on either side of the hot path: the per-frame checkpoint the loop writes and the
pseudo-label files derived from it.  Host-side I/O only.

  checkpoint dict           scripts/main.py:1109-1121 (`Saver.save` = torch.save of this dict, vsrd/utils.py:191-198);
                            consumer tools/kitti_360/make_predictions.py:61-66 loads models.detector only
  prediction JSON           tools/kitti_360/make_predictions.py:158-169   {boxes_3d, boxes_2d, confidences} per class
  multi-view confidences    tools/kitti_360/make_predictions.py:86-176    mean box IoU over source views + Hungarian (maximise)
  KITTI label line          tools/kitti_360/convert_predictions.py:16-78
  per-frame label files     save_frame_labels: what optimization.FrameOptimizer.labels() returns (vsrd_frame_labels), as the two above
  per-frame log             save_frame_history (history.json, the reference's scalar names, scripts/main.py:926-939), save_frame_snapshots
                            (step_{step}.pt: step, models, metrics) and select_model (tools/select_model.py's rule -> model.pt) over what
                            optimization.FrameOptimizer.history() / snapshots() return (vsrd_frame_log)
  per-frame metrics         frame_metrics: the summary of optimization.FrameOptimizer.metrics() (vsrd_frame_metrics) under the reference's
                            six names (scripts/main.py:908-924)
"""
import json
import math
import operator
import os
import re
import shutil

import torch


def to_host(value):
    """A checkpoint payload with every tensor copied to host memory (containers rebuilt, everything else as it is)."""
    if isinstance(value, torch.Tensor):
        return value.detach().cpu()
    if isinstance(value, dict):
        return type(value)((k, to_host(v)) for k, v in value.items())
    if isinstance(value, (list, tuple)):
        return type(value)(to_host(v) for v in value)
    return value


def checkpoint_payload(frame_optimizer, step, metrics=None, host=False):
    """``host=True``: the tensors already in host memory -- what a frame optimised next to others must hand to ``torch.save``: serialising
    device tensors copies them with calls that HIP refuses while another frame's thread captures a graph (launcher.main takes the copies
    under optimization.exclusive_device_access())."""
    models = {"detector": frame_optimizer.detector.state_dict(),
              "hyper_distance_field": frame_optimizer.hyper_distance_field.state_dict()}
    # eager and hipGraph mode write the same layout (FrameOptimizer.optimizer_state_dict / scheduler_state_dict)
    payload = dict(step=step, models=models, optimizer=frame_optimizer.optimizer_state_dict(),
                   scheduler=frame_optimizer.scheduler_state_dict(), metrics=metrics or {})
    return to_host(payload) if host else payload


def atomic_torch_save(payload, path):
    """torch.save to ``path`` through a temporary file and os.replace: a process killed mid-write leaves no truncated file that
    the "skip if the final checkpoint exists" restart guard (main.py:134-136) would take for a finished frame."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    temporary = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(payload, temporary)
        os.replace(temporary, path)
    finally:
        if os.path.exists(temporary):
            os.remove(temporary)


def save_checkpoint(path, frame_optimizer, step, metrics=None):
    atomic_torch_save(checkpoint_payload(frame_optimizer, step, metrics), path)


def prediction_record(boxes_3d, boxes_2d, confidences, class_name="car"):
    """make_predictions.py:158-163: camera-frame corners [N,8,3], 2-D boxes [N,2,2], confidences [N]."""
    return dict(boxes_3d={class_name: boxes_3d.tolist()}, boxes_2d={class_name: boxes_2d.tolist()},
                confidences={class_name: confidences.tolist()})


def save_prediction(path, boxes_3d, boxes_2d, confidences, class_name="car"):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as file:
        json.dump(prediction_record(boxes_3d, boxes_2d, confidences, class_name), file, indent=4, sort_keys=False)


def box_iou(boxes1, boxes2):
    """torchvision.ops.box_iou on [N,4] x [M,4]."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[None, :, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(-1)
    return inter / (area1[:, None] + area2[None, :] - inter)


def multi_view_confidences(pd_boxes_2d, gt_boxes_2d, gt_to_target):
    """make_predictions.py:86-176.  Per source view v: pd_boxes_2d[v] [N,2,2] (already clipped), gt_boxes_2d[v] [M_v,2,2],
    gt_to_target[v] [M_v] = index of each source instance among the target's instances (-1 = absent).
    Returns (confidences [K], matched_pd [K], matched_gt [K])."""
    from scipy.optimize import linear_sum_assignment
    num_pd = pd_boxes_2d[0].shape[0]
    num_gt = 1 + max(int(t.max()) for t in gt_to_target)
    iou_sum, count = torch.zeros(num_pd, num_gt), torch.zeros(num_pd, num_gt)
    for pd, gt, index in zip(pd_boxes_2d, gt_boxes_2d, gt_to_target):
        iou = torch.nan_to_num(box_iou(pd.flatten(-2, -1).cpu(), gt.flatten(-2, -1).cpu()))
        keep = index >= 0
        iou_sum[:, index[keep]] += iou[:, keep]
        count[:, index[keep]] += 1
    mean = iou_sum / count
    pd_idx, gt_idx = linear_sum_assignment(mean.numpy(), maximize=True)
    return mean[pd_idx, gt_idx], torch.as_tensor(pd_idx), torch.as_tensor(gt_idx)


def kitti_label_line(class_name, box_3d, box_2d, score):
    """convert_predictions.py:16-78: one KITTI-3D label line from camera-frame corners [8,3], a 2-D box [2,2] and a score."""
    location = box_3d.mean(-2)

    def mean_edge(a, b):
        return (box_3d[a, :] - box_3d[b, :]).norm(dim=-1).mean(-1)
    width, height, length = mean_edge([1, 2, 6, 5], [0, 3, 7, 4]), mean_edge([4, 5, 6, 7], [0, 1, 2, 3]), mean_edge([1, 0, 4, 5], [2, 3, 7, 6])
    forward = (box_3d[[1, 0, 4, 5], :] - box_3d[[2, 3, 7, 6], :]).mean(-2)
    heading = torch.nn.functional.normalize(forward[[2, 0]], dim=-1)
    orientation = torch.atan2(heading[1], heading[0])
    location = location.clone()
    location[1] += height / 2.0
    dimension = torch.stack([height, width, length])
    ray_orientation = torch.atan2(location[0], location[2])
    global_orientation = orientation - math.pi / 2.0
    local_orientation = global_orientation - ray_orientation
    return (f"{class_name.capitalize()} {0.0} {0} {local_orientation} "
            f"{' '.join(map(str, box_2d.flatten().tolist()))} {' '.join(map(str, dimension.tolist()))} "
            f"{' '.join(map(str, location.tolist()))} {global_orientation} {score}\n")


def save_kitti_labels(path, class_names, boxes_3d, boxes_2d, scores):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as file:
        for name, box_3d, box_2d, score in zip(class_names, boxes_3d, boxes_2d, scores):
            file.write(kitti_label_line(name, box_3d, box_2d, score))


def _atomic_write(path, write):
    """``write(temporary name)`` and os.replace onto ``path``, like atomic_torch_save; what a killed process left under this name goes first."""
    folder, stem = os.path.dirname(path) or ".", os.path.basename(path) + ".tmp."
    os.makedirs(folder, exist_ok=True)
    for name in os.listdir(folder):
        if name.startswith(stem):
            os.remove(os.path.join(folder, name))
    temporary = f"{path}.tmp.{os.getpid()}"
    try:
        write(temporary)
        os.replace(temporary, path)
    finally:
        if os.path.exists(temporary):
            os.remove(temporary)


def save_frame_labels(folder, labels, class_name="car"):
    """One frame's pseudo-labels as files.  ``labels``: the dictionary of ``FrameOptimizer.labels()`` (host or device tensors) -- boxes_3d
    [V,n,8,3] camera-frame corners per view, boxes_2d [V,n,2,2], confidences [n].  Writes ``folder/predictions/view_VV.json`` for every view
    (that view's corners and 2-D boxes, the same confidences in every file: make_predictions.py:164-192) and ``folder/labels/view_00.txt``,
    the KITTI label lines of the target view (convert_predictions.py:16-78).  Every file is written under a temporary name and renamed."""
    boxes_3d, boxes_2d, confidences = (labels[key].detach().cpu() for key in ("boxes_3d", "boxes_2d", "confidences"))
    for view in range(boxes_3d.shape[0]):
        _atomic_write(os.path.join(folder, "predictions", f"view_{view:02d}.json"),
                      lambda name, view=view: save_prediction(name, boxes_3d[view], boxes_2d[view], confidences, class_name))
    _atomic_write(os.path.join(folder, "labels", "view_00.txt"),
                  lambda name: save_kitti_labels(name, [class_name] * len(confidences), boxes_3d[0], boxes_2d[0], confidences.tolist()))


def save_frame_group_labels(folder, labels, class_name="car"):
    """One frame's pseudo-labels in the frames of its GROUP as files -- what the reference's second pass leaves for a detector to be trained
    on.  ``labels``: the dictionary of ``FrameOptimizer.group_labels()`` (host or device tensors) -- boxes_3d [L,n,8,3] camera-frame corners
    per group frame, boxes_2d [L,n,2,2], confidences [n], frame_ids [L].  Writes, for every group frame, ``folder/group/predictions/<id:010d>.json``
    (that frame's corners and 2-D boxes, the same confidences in every file: make_predictions.py:164-192) and
    ``folder/group/labels/<id:010d>.txt``, its KITTI label lines (convert_predictions.py:16-78).  Every file is written under a temporary
    name and renamed."""
    boxes_3d, boxes_2d, confidences, frame_ids = (labels[key].detach().cpu() for key in ("boxes_3d", "boxes_2d", "confidences", "frame_ids"))
    if len(set(frame_ids.tolist())) != len(frame_ids) or boxes_3d.shape[0] != len(frame_ids):
        raise ValueError(f"frame_ids {frame_ids.tolist()} for {boxes_3d.shape[0]} group frames: one id per frame, none twice")
    for view, frame_id in enumerate(frame_ids.tolist()):
        _atomic_write(os.path.join(folder, "group", "predictions", f"{int(frame_id):010d}.json"),
                      lambda name, view=view: save_prediction(name, boxes_3d[view], boxes_2d[view], confidences, class_name))
        _atomic_write(os.path.join(folder, "group", "labels", f"{int(frame_id):010d}.txt"),
                      lambda name, view=view: save_kitti_labels(name, [class_name] * len(confidences), boxes_3d[view], boxes_2d[view], confidences.tolist()))


FRAME_METRIC_NAMES = ("iou_3d", "iou_bev", "accuracy_3d_25", "accuracy_bev_25", "accuracy_3d_50", "accuracy_bev_50")     # main.py:917-924


def frame_metrics_summary(ious_3d, ious_bev):
    """The summary vsrd_frame_metrics writes, computed on the host from per-pair IoUs (any sequence; a NaN pair has no annotation and is
    left out): [count, mean iou_3d, mean iou_bev, the shares of pairs with IoU > 0.25 (3-D, BEV) and > 0.5 (3-D, BEV), 0] as Python
    floats, summed in the given order in double; eight zeros without a pair (scripts/main.py:908-915)."""
    pairs = [(float(a), float(b)) for a, b in zip(ious_3d, ious_bev) if not (math.isnan(float(a)) or math.isnan(float(b)))]
    if not pairs:
        return [0.0] * 8
    count = float(len(pairs))
    columns = [[a for a, _ in pairs], [b for _, b in pairs]]
    sums = [sum(columns[0]), sum(columns[1])] + [float(sum(1 for v in columns[j] if v > bound)) for bound in (0.25, 0.5) for j in (0, 1)]
    return [count] + [value / count for value in sums] + [0.0]


def frame_metrics(summary):
    """``metrics()["summary"]`` (vsrd_frame_metrics: count, then the six values) as the dictionary the reference logs
    (scripts/main.py:917-924: iou_3d, iou_bev, accuracy_3d_25, accuracy_bev_25, accuracy_3d_50, accuracy_bev_50), Python floats; {} when
    the count is 0 -- no pair had ground truth, and the reference logs no metrics then."""
    values = [float(v) for v in (summary.detach().cpu().tolist() if isinstance(summary, torch.Tensor) else summary)]
    if len(values) != 8:
        raise ValueError(f"a metrics summary has 8 entries, got {len(values)}")
    if values[0] == 0.0:
        return {}
    return dict(zip(FRAME_METRIC_NAMES, values[1:7]))


def save_frame_masks(folder, masks, shape, view=0):
    """One view's dense predicted instance masks as a file.  ``masks``: the dictionary of ``FrameOptimizer.masks()`` (host or device tensors)
    -- inside [n,H,ceil(W/8)] uint8, counts [n,3], mask_iou [n], threshold; ``shape`` = (H, W).  Writes ``folder/masks/view_VV.npz`` with
    `inside` (numpy.packbits along W, most significant bit first: the frame packs' mask format, frames.unpack_masks), `shape`, `threshold`,
    `counts` and `mask_iou`, under a temporary name and renamed."""
    import numpy as np
    arrays = {key: torch.as_tensor(masks[key]).detach().cpu().numpy() for key in ("inside", "counts", "mask_iou")}
    height, width = (int(x) for x in shape)
    if arrays["inside"].ndim != 3 or arrays["inside"].shape[1:] != (height, (width + 7) // 8):
        raise ValueError(f"inside of shape {arrays['inside'].shape} does not hold masks of {height} x {width} pixels")
    path = os.path.join(folder, "masks", f"view_{int(view):02d}.npz")

    def write(name):
        with open(name, "wb") as file:         # (a file object: numpy appends no suffix to the temporary name)
            np.savez(file, inside=arrays["inside"].astype(np.uint8), shape=np.asarray([height, width], dtype=np.int64),
                     threshold=np.float32(masks.get("threshold", 0.5)), counts=arrays["counts"].astype(np.int32),
                     mask_iou=arrays["mask_iou"].astype(np.float32))
    _atomic_write(path, write)
    return path


def load_frame_masks(path):
    """What save_frame_masks wrote (a folder: its masks/view_00.npz): a dictionary of numpy arrays, `shape` as a tuple (H, W) and `threshold` as a float."""
    import numpy as np
    if os.path.isdir(path):
        path = os.path.join(path, "masks", "view_00.npz")
    with np.load(path) as data:
        return dict(inside=data["inside"], shape=tuple(int(x) for x in data["shape"]), threshold=float(data["threshold"]), counts=data["counts"],
                    mask_iou=data["mask_iou"])


def png_bytes(image):
    """An 8-bit RGB image [H,W,3] uint8 as the bytes of a PNG file: the signature, IHDR, one IDAT (every row with filter 0, deflated by the
    standard library's zlib) and IEND.  Nothing but the standard library: the project grows no imaging dependency for one picture."""
    import struct
    import zlib
    import numpy as np
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"an RGB image is [H,W,3], got {image.shape}")
    height, width = int(image.shape[0]), int(image.shape[1])

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    rows = np.concatenate([np.zeros((height, 1), dtype=np.uint8), image.reshape(height, width * 3)], axis=1)       # (filter type 0 in front of every row)
    header = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)                 # bit depth 8, colour type 2 (RGB), deflate, adaptive filtering, no interlace
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", header) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")


def save_frame_surface(folder, surface, view=0):
    """One view's dense surface render as files.  ``surface``: the dictionary of ``FrameOptimizer.surface()`` (host or device tensors) --
    converged_bits / shadow_bits [H,ceil(W/8)] uint8, instance [H,W] uint8, range [H,W], colors [H,W,3] uint8, light [3], shape.  Writes
    ``folder/surface/view_VV.npz`` with `converged_bits` and `shadow_bits` (numpy.packbits along W, most significant bit first:
    frames.unpack_masks reads them), `instance` (255: none), `range`, `shape` and `light`, and ``folder/surface/view_VV.png``, the colour
    image (png_bytes); each under a temporary name and renamed.  Returns the two paths."""
    import numpy as np
    arrays = {key: torch.as_tensor(surface[key]).detach().cpu().numpy() for key in ("converged_bits", "shadow_bits", "instance", "range", "colors", "light")}
    height, width = (int(x) for x in surface["shape"])
    for key in ("converged_bits", "shadow_bits"):
        if arrays[key].shape != (height, (width + 7) // 8):
            raise ValueError(f"{key} of shape {arrays[key].shape} does not hold {height} x {width} pixels")
    if arrays["instance"].shape != (height, width) or arrays["range"].shape != (height, width) or arrays["colors"].shape != (height, width, 3):
        raise ValueError(f"instance, range and colors of shapes {arrays['instance'].shape}, {arrays['range'].shape}, {arrays['colors'].shape} "
                         f"for an image of {height} x {width} pixels")
    stem = os.path.join(folder, "surface", f"view_{int(view):02d}")

    def write_arrays(name):
        with open(name, "wb") as file:         # (a file object: numpy appends no suffix to the temporary name)
            np.savez(file, converged_bits=arrays["converged_bits"].astype(np.uint8), shadow_bits=arrays["shadow_bits"].astype(np.uint8),
                     instance=arrays["instance"].astype(np.uint8), range=arrays["range"].astype(np.float32),
                     shape=np.asarray([height, width], dtype=np.int64), light=arrays["light"].astype(np.float32).reshape(3))

    def write_image(name):
        with open(name, "wb") as file:
            file.write(png_bytes(arrays["colors"]))
    _atomic_write(stem + ".npz", write_arrays)
    _atomic_write(stem + ".png", write_image)
    return stem + ".npz", stem + ".png"


def load_frame_surface(path):
    """What save_frame_surface wrote in its npz (a folder: its surface/view_00.npz): a dictionary of numpy arrays, `shape` as a tuple (H, W)."""
    import numpy as np
    if os.path.isdir(path):
        path = os.path.join(path, "surface", "view_00.npz")
    with np.load(path) as data:
        return dict(converged_bits=data["converged_bits"], shadow_bits=data["shadow_bits"], instance=data["instance"], range=data["range"],
                    shape=tuple(int(x) for x in data["shape"]), light=data["light"])


# ---- the per-frame log: scalar history and step snapshots (optimization.FrameOptimizer.history / snapshots, vsrd_frame_log) ---------------
HISTORY_LOSSES = ("iou_projection_loss", "l1_projection_loss", "silhouette_loss", "eikonal_loss", "loss")
# config.optimization.param_group_names of the reference's configs, the order of the optimiser's groups (scripts/main.py:929-933)
HISTORY_LEARNING_RATES = ("detector/locations", "detector/dimensions", "detector/orientations", "detector/embeddings", "hyper_distance_field")
HISTORY_HYPERPARAMETERS = ("sdf_union_temperature", "sdf_std_deviation", "cosine_ratio")


def frame_history_records(history):
    """``FrameOptimizer.history()`` (host or device tensors) as a list of dictionaries, one per logged step, under the reference's scalar
    names (scripts/main.py:926-939): ``step``, ``losses/<name>`` (and ``losses/loss``, the weighted total; ``losses/eikonal_loss`` is left
    out where it is NaN -- a box-only step, for which the reference's dictionary has no such key), ``metrics/<name>`` only when the row has
    metrics and the value is finite, ``learning_rates/<group>``, ``hyperparameters/<name>``.  Python ints and floats."""
    host = {key: torch.as_tensor(value).detach().cpu() for key, value in history.items()}
    records = []
    for row in range(int(host["steps"].shape[0])):
        record = {"step": int(host["steps"][row])}
        for name in HISTORY_LOSSES:
            value = float(host[name][row])
            if name != "eikonal_loss" or not math.isnan(value):
                record[f"losses/{name}"] = value
        summary = [float(v) for v in host["metrics"][row].tolist()]
        for name, value in frame_metrics(summary).items():        # (a row without metrics holds NaN, one without a pair a count of 0: neither names any)
            if math.isfinite(value):
                record[f"metrics/{name}"] = value
        record.update({f"learning_rates/{name}": float(v) for name, v in zip(HISTORY_LEARNING_RATES, host["learning_rates"][row].tolist())})
        record.update({f"hyperparameters/{name}": float(v) for name, v in zip(HISTORY_HYPERPARAMETERS, host["hyperparameters"][row].tolist())})
        records.append(record)
    return records


def save_frame_history(folder, history):
    """One frame's scalar history as ``folder/history.json``: the list of ``frame_history_records``, written under a temporary name and renamed."""
    records = frame_history_records(history)
    path = os.path.join(folder, "history.json")

    def write(name):
        with open(name, "w") as file:
            json.dump(records, file, indent=1)
    _atomic_write(path, write)
    return path


def snapshot_payloads(snapshots):
    """``FrameOptimizer.snapshots()`` as checkpoint payloads in host memory: ``step`` (int), ``models`` (the state dicts, copied: a slot's
    views change with the frame's next reset) and ``metrics`` by name -- the reference's six from the slot's summary (none when no pair had
    ground truth) and ``mask_iou``, the mean over the instances, as the final checkpoint carries them.  What tools/select_model.py and
    make_predictions.py read of a step_{step}.pt; optimiser and scheduler state stay with the final checkpoint.  Payloads pass through
    unchanged (a named metric stays, the mean of one number is that number)."""
    payloads = []
    for snapshot in snapshots:
        host = to_host(snapshot)
        metrics = {name: float(value) for name, value in host["metrics"].items() if name not in ("summary", "mask_iou")}
        if "summary" in host["metrics"]:
            metrics.update(frame_metrics(host["metrics"]["summary"]))
        if "mask_iou" in host["metrics"]:
            metrics["mask_iou"] = float(torch.as_tensor(host["metrics"]["mask_iou"], dtype=torch.float32).mean())
        models = {module: {key: value.clone() for key, value in state.items()} for module, state in host["models"].items()}
        payloads.append(dict(step=int(host["step"]), models=models, metrics=metrics))
    return payloads


def save_frame_snapshots(folder, snapshots, skip_steps=()):
    """``FrameOptimizer.snapshots()`` (or their ``snapshot_payloads``) as ``folder/step_{step}.pt`` files, each written under a temporary
    name and renamed.  ``skip_steps``: steps whose file somebody else writes (the launcher's final checkpoint, which holds the same models
    and metrics and marks the frame as done).  Returns the paths."""
    paths = []
    for payload in snapshot_payloads(snapshots):
        if payload["step"] in skip_steps:
            continue
        paths.append(os.path.join(folder, f"step_{payload['step']}.pt"))
        atomic_torch_save(payload, paths[-1])
    return paths


_CONSTRAINT = re.compile(r"\s*(\w+)\s*(<=|>=|==|!=|<|>)\s*([+-]?(?:\d+\.?\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?))\s*")
_COMPARISONS = {"<": operator.lt, "<=": operator.le, "==": operator.eq, "!=": operator.ne, ">=": operator.ge, ">": operator.gt}


def select_model(folder, metrics, maximum=False, constraints=(), step_range=()):
    """The selection rule of the reference's tools/select_model.py over one frame's folder: of the ``*.pt`` checkpoints directly in
    ``folder`` -- ``model.pt`` itself aside -- those whose ``metrics`` hold every name in ``metrics``, meet every constraint
    (``name<op>value`` with <, <=, ==, !=, >=, >; a checkpoint lacking the constrained metric does not meet it) and whose ``step`` lies in
    ``range(*step_range)`` (empty: any) compete; the mean over the named metrics decides, by a strict comparison (smallest, or with
    ``maximum`` largest); the winner is copied to ``folder/model.pt`` (under a temporary name, then renamed).  One stated difference: the
    candidates are visited in ascending step order, so a tie keeps the EARLIEST step; the reference visits them in glob order, which is
    unspecified.  Returns (path of the winner, its named metrics), or (None, {}) when nothing competes (model.pt is then left alone)."""
    metrics = [metrics] if isinstance(metrics, str) else list(metrics)
    if not metrics:
        raise ValueError("select_model: name at least one metric")
    tests = []
    for constraint in constraints:
        match = _CONSTRAINT.fullmatch(constraint)
        if not match:
            raise ValueError(f"constraint {constraint!r}: expected name<op>value with one of < <= == != >= >")
        tests.append((match.group(1), _COMPARISONS[match.group(2)], float(match.group(3))))
    candidates = []
    for name in os.listdir(folder):
        path = os.path.join(folder, name)
        if not name.endswith(".pt") or name == "model.pt" or not os.path.isfile(path):
            continue
        checkpoint = torch.load(path, map_location="cpu", weights_only=False)
        candidates.append((int(checkpoint.get("step", 0)), name, path, checkpoint.get("metrics") or {}))
    better = operator.gt if maximum else operator.lt
    best = None
    for step, name, path, stored in sorted(candidates, key=lambda c: (c[0], c[1])):
        if not all(metric in stored for metric in metrics):
            continue
        if not all(key in stored and compare(float(stored[key]), value) for key, compare, value in tests):
            continue
        if step_range and step not in range(*step_range):
            continue
        mean = sum(float(stored[metric]) for metric in metrics) / len(metrics)
        if best is None or better(mean, best[0]):
            best = (mean, path, {metric: float(stored[metric]) for metric in metrics})
    if best is None:
        return None, {}
    _atomic_write(os.path.join(folder, "model.pt"), lambda temporary: shutil.copyfile(best[1], temporary))
    return best[1], best[2]
