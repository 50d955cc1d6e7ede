"""csrc/frame_labels.h -- vsrd_frame_labels, a frame's pseudo-labels in one single-workgroup launch (camera-frame corners and clipped 2-D
boxes of every view, the mean box IoU of every (prediction, ground-truth slot) pair over the views that see the slot, the assignment that
maximises it, the matched mean IoU as confidence) -- through the C ABI with buffers of the test's own, up to the ABI's 32 views x 64 boxes.

Every call works on ONE arena of the test's own, laid out like a frame batch's rows (every buffer at the same offset of its frame's row,
rows `stride` bytes apart, 256 spare bytes between them), filled with NaN bits (the int64 output with -7) before the inputs are written:
what a call did not write is found by comparing bytes.

Where the bounds come from.  camera_corners and boxes_2d are compared with oracle/frame_glue.py in float64; the same oracle in float32
is the floor, and the device may be at 2 x floor + the float32 spacing of the quantity's largest magnitude (the rule of
test_hip_frame_glue.py for quantities without a project bound; frame_glue_scenes.box_tolerance for the boxes).  mean_iou is compared with
formats.box_iou evaluated in float64 on the device's OWN boxes and the float32 ground truth: one IoU <= 1 is about ten float32 roundings, and
the sum of at most V terms <= 1 divided by its count adds at most V half-spacings of 1 -- (V + 16) 2^-24; the views are summed in ascending
order, so the float32 accumulation order is fixed.  End to end (float64 boxes, float64 ground truth) it may be at 2 x floor + that bound.
The assignment is scipy's on the device's own matrix, exactly (a float64 matrix may break a near-tie the other way, which is no kernel
error), and the confidences are the matched entries bit for bit."""
import math

import pytest
import torch
from scipy.optimize import linear_sum_assignment

import frame_glue_scenes as scenes
from conftest import margin
from frame_rows import RowArena
from oracle import frame_glue as ref

pytestmark = pytest.mark.gpu

NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()
HALF_SPACING = 2.0 ** -24
GAP = 256                                  # bytes between the rows that no buffer covers
INPUTS = ("loc", "dim", "ori", "E", "K", "gt", "visible", "header")
OUTPUTS = ("camera_corners", "boxes_2d", "mean_iou", "matched_gt", "confidences")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


class Arena(RowArena):
    """B rows laid out for V views and a capacity of N boxes, filled with NaN bits (the int64 output with -7)."""

    def __init__(self, V, N, B=1):
        f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
        fields = [("loc", (N, 3), f32), ("dim", (N, 3), f32), ("ori", (N, 2), f32), ("E", (V, 16), f32), ("K", (V, 9), f32), ("gt", (V, N, 4), f32),
                  ("visible", (V, N), u8), ("header", (2,), i32), ("camera_corners", (V, N, 8, 3), f32), ("boxes_2d", (V, N, 4), f32),
                  ("mean_iou", (N, N), f32), ("matched_gt", (N,), i64), ("confidences", (N,), f32)]
        super().__init__(fields, B, NAN_BITS, GAP)
        self.V, self.N = V, N
        for f in range(B):
            self.view("matched_gt", f).fill_(-7)

    def put(self, f, scene, header=True):
        """Frame f's inputs: the scene's n boxes in the first n instances of the row (the pad instances keep the fill)."""
        V, n = scene["visible"].shape
        raw = scene["raw"].float()
        self.view("loc", f)[:n], self.view("dim", f)[:n], self.view("ori", f)[:n] = raw[:, 0:3], raw[:, 3:6], raw[:, 6:8]
        self.view("E", f).copy_(scene["E"].float().reshape(V, 16))
        self.view("K", f).copy_(scene["K"].float().reshape(V, 9))
        self.view("gt", f)[:, :n] = scene["gt_boxes"].float()
        self.view("visible", f)[:, :n] = scene["visible"].to(torch.uint8)
        if header:
            self.write_header(f, n)


def _frame_config(V, N, B=1, stride=0, num_steps=3000):
    from oracle import geometry
    from vsrd_amd import _lib
    return _lib.make_frame_config(N, V, scenes.IMAGE_SIZE, 1.0e-6, geometry.LOCATION_RANGE, geometry.DIMENSION_RANGE, num_steps=num_steps, frames=(B, stride))


def _call(dev, arena, header=True, frame=None, null=(), expect_ok=True):
    """One vsrd_frame_labels call on the arena -> (return code, the arena's bytes afterwards, on the host)."""
    from vsrd_amd import _lib
    lib = _lib.load()
    device = arena.host.to(dev)
    pointer = arena.pointers(device, null)
    if frame is None:
        frame = _frame_config(arena.V, arena.N, arena.B, arena.stride if arena.B > 1 else 0)
    code = lib.vsrd_frame_labels(frame, *[pointer(name) for name in INPUTS[:-1]], *[pointer(name) for name in OUTPUTS],
                                 pointer("header") if header else None, _lib.stream())
    torch.cuda.synchronize()
    if expect_ok:
        _lib.check(code)
    return code, device.cpu()


def _alone(dev, scene):
    """The scene in a call of its own: by-value N = n, no header -> {output name: host tensor}."""
    V, n = scene["visible"].shape
    arena = Arena(V, n)
    arena.put(0, scene, header=False)
    _, after = _call(dev, arena, header=False)
    before = arena.host
    for name in INPUTS:                                            # nothing but the outputs changed
        assert torch.equal(arena.view(name, 0, after), arena.view(name, 0, before)), name
    assert torch.equal(after[-GAP:], before[-GAP:])
    return {name: arena.view(name, 0, after).clone() for name in OUTPUTS}


def _float32(scene):
    return {key: value.float() if value.dtype == torch.float64 else value for key, value in scene.items()}


def _mean_iou(boxes, gt_boxes, visible):
    """make_predictions.py:111-176 in the dtype of `boxes`: formats.box_iou per view, NaN -> 0, summed over the views (ascending) that see
    the ground-truth slot, divided by their number; 0 where no view sees it (the kernel's stated deviation) -> ([n,n], count [n])."""
    from vsrd_amd import formats
    n = boxes.shape[1]
    total, count = torch.zeros(n, n, dtype=boxes.dtype), torch.zeros(n, dtype=boxes.dtype)
    for v in range(boxes.shape[0]):
        iou = torch.nan_to_num(formats.box_iou(boxes[v], gt_boxes[v].to(boxes.dtype)), nan=0.0)
        total = total + iou * visible[v].to(boxes.dtype)
        count = count + visible[v].to(boxes.dtype)
    return torch.where(count > 0, total / count.clamp_min(1.0), torch.zeros_like(total)), count


def _spacing(value):
    """The float32 spacing at magnitude `value`."""
    return 2.0 ** (math.floor(math.log2(max(float(value), 2.0 ** -126))) - 23)


def _check(label, scene, out):
    V, n = scene["visible"].shape
    s32 = _float32(scene)
    forward = ref.forward(scene["raw"], scene["E"], scene["K"], scenes.IMAGE_SIZE)
    forward32 = ref.forward(s32["raw"], s32["E"], s32["K"], scenes.IMAGE_SIZE)
    assert bool(torch.isfinite(out["camera_corners"]).all()) and bool(torch.isfinite(out["boxes_2d"]).all()) and bool(torch.isfinite(out["mean_iou"]).all())
    # ---- camera corners, 2-D boxes against float64 ---------------------------------------------------------------------------------
    floor = float((forward32["cam"].double() - forward["cam"]).abs().max())
    tolerance = 2.0 * floor + _spacing(forward["cam"].abs().max())
    observed = float((out["camera_corners"].double() - forward["cam"]).abs().max())
    margin(label, "camera corners [m]", observed, tolerance)
    assert observed <= tolerance, (label, "camera corners", observed, tolerance, floor)
    floor = float((forward32["boxes"].double() - forward["boxes"]).abs().max())
    tolerance = scenes.box_tolerance(floor)
    observed = float((out["boxes_2d"].double() - forward["boxes"]).abs().max())
    margin(label, "2-D boxes [px]", observed, tolerance)
    assert observed <= tolerance, (label, "2-D boxes", observed, tolerance, floor)
    # ---- mean IoU: the formula in float64 on the device's own boxes and the float32 ground truth ------------------------------------------
    bound = (V + 16) * HALF_SPACING
    formula, count = _mean_iou(out["boxes_2d"].double(), s32["gt_boxes"].double(), scene["visible"])
    observed = float((out["mean_iou"].double() - formula).abs().max())
    margin(label, "mean IoU - formula", observed, bound)
    assert observed <= bound, (label, "mean IoU - formula", observed, bound)
    exact_zero = (formula == 0) | (count == 0)[None, :]            # no view sees the slot, or every IoU is 0 or 0 / 0
    assert bool((out["mean_iou"][exact_zero].view(torch.int32) == 0).all())          # +0.0, bit for bit
    # ---- mean IoU end to end ------------------------------------------------------------------------------------------------------
    reference, _ = _mean_iou(forward["boxes"], scene["gt_boxes"], scene["visible"])
    oracle32, _ = _mean_iou(forward32["boxes"], s32["gt_boxes"], scene["visible"])
    floor = float((oracle32.double() - reference).abs().max())
    tolerance = 2.0 * floor + bound
    observed = float((out["mean_iou"].double() - reference).abs().max())
    margin(label, "mean IoU end to end", observed, tolerance)
    assert observed <= tolerance, (label, "mean IoU end to end", observed, tolerance, floor)
    # ---- assignment (at the device's own matrix), confidences ------------------------------------------------------------------------
    rows, cols = linear_sum_assignment(out["mean_iou"].double().numpy(), maximize=True)
    assert rows.tolist() == list(range(n))
    assert out["matched_gt"].tolist() == cols.tolist(), (label, out["matched_gt"].tolist(), cols.tolist())
    matched = out["mean_iou"][torch.arange(n), out["matched_gt"]]
    assert torch.equal(out["confidences"].view(torch.int32), matched.view(torch.int32))
    return forward


SHAPES = [(1, 1, 0), (3, 5, 4), (8, 32, 1), (17, 16, 2), (32, 64, 2)]            # (V, N, seed); 32 x 64: 2048 pairs, every strided loop takes several trips


@pytest.mark.parametrize("V,N,seed", SHAPES, ids=[f"{v}x{n}" for v, n, _ in SHAPES])
def test_labels_match_the_float64_reference(dev, V, N, seed):
    scene = scenes.build(V, N, seed)
    forward = _check(f"test_labels_match_the_float64_reference[{V}x{N}]", scene, _alone(dev, scene))
    if V >= 17:                                # box 1 stands behind source cameras: clipped boxes without area
        area = (forward["boxes"][:, 1, 2] - forward["boxes"][:, 1, 0]) * (forward["boxes"][:, 1, 3] - forward["boxes"][:, 1, 1])
        assert bool((area == 0).any())


def _hand_made_scene():
    """3 views, 4 boxes: ground-truth boxes of zero area (xmin = xmax: slot 0 in view 1, slot 3 in every view), a slot no view sees (2), and
    a prediction (3) whose clipped box has zero area in every view: 49 m to the left at 3 m depth, both of its x coordinates are clamped to
    0.  Row 3 and columns 2 and 3 of the matrix are all zero: predictions 2 and 3 can take slots 2 and 3 either way round at the same
    total, and the tie rule decides."""
    scene = scenes.build(3, 4, 5)
    scene["visible"][:] = True
    scene["gt_boxes"] = ref.forward(scene["raw"], scene["E"], scene["K"], scenes.IMAGE_SIZE)["boxes"][:, torch.tensor([1, 0, 3, 2])] + 2.5
    scene["raw"][3, 0] = torch.logit(torch.tensor(0.01, dtype=torch.float64))
    scene["raw"][3, 2] = torch.logit(torch.tensor(0.03, dtype=torch.float64))
    scene["gt_boxes"][1, 0, 2] = scene["gt_boxes"][1, 0, 0]
    scene["gt_boxes"][:, 3, 2] = scene["gt_boxes"][:, 3, 0]
    scene["visible"][:, 2] = False
    scene["gt_boxes"][:, 2] = 0.0
    return scene


def test_labels_of_the_hand_made_scene(dev):
    scene = _hand_made_scene()
    out = _alone(dev, scene)
    forward = _check("test_labels_of_the_hand_made_scene", scene, out)
    boxes = forward["boxes"]
    assert bool(((boxes[:, 3, 2] - boxes[:, 3, 0]) == 0).all())                      # the prediction without area, in every view
    assert bool((out["mean_iou"][3].view(torch.int32) == 0).all()) and bool((out["mean_iou"][:, 2:].view(torch.int32) == 0).all())
    assert float(out["mean_iou"][0, 1]) > 0.3 and float(out["mean_iou"][1, 0]) > 0.3          # the others overlap their ground truth
    assert float(out["confidences"][3]) == 0.0


@pytest.mark.parametrize("capacity,n", [(8, 5), (16, 13)])
def test_header_twin_leaves_the_pad_instances_alone(dev, capacity, n):
    """A row laid out for `capacity` boxes whose header says n: the n instances' outputs are the bits of a call with by-value N = n on
    buffers laid out for n, and every entry of instances n .. capacity - 1 -- rows AND columns of mean_iou -- keeps the fill."""
    V = 17
    scene = scenes.build(V, n, 1)
    alone = _alone(dev, scene)
    arena = Arena(V, capacity)
    arena.put(0, scene)
    expected = arena.host.clone()
    for name in ("camera_corners", "boxes_2d"):
        arena.view(name, 0, expected)[:, :n] = alone[name]
    arena.view("mean_iou", 0, expected)[:n, :n] = alone["mean_iou"]
    for name in ("matched_gt", "confidences"):
        arena.view(name, 0, expected)[:n] = alone[name]
    _, after = _call(dev, arena)
    assert not torch.equal(after, arena.host)
    assert torch.equal(after, expected)                           # bytes: the n instances' bits, the fill everywhere else


def test_batch_of_three_frames(dev):
    """B = 3 frames with (3, 8, 13) boxes in rows of capacity 13: every frame's outputs are the bits of its own single-frame call, and
    the pad instances and the bytes between the rows keep the fill."""
    V, capacity, counts = 4, 13, (3, 8, 13)
    arena = Arena(V, capacity, B=len(counts))
    assert arena.stride % 256 == 0
    frames = [scenes.build(V, n, 10 + k) for k, n in enumerate(counts)]
    for f, scene in enumerate(frames):
        arena.put(f, scene)
    expected = arena.host.clone()
    for f, (scene, n) in enumerate(zip(frames, counts)):
        alone = _alone(dev, scene)
        for name in ("camera_corners", "boxes_2d"):
            arena.view(name, f, expected)[:, :n] = alone[name]
        arena.view("mean_iou", f, expected)[:n, :n] = alone["mean_iou"]
        for name in ("matched_gt", "confidences"):
            arena.view(name, f, expected)[:n] = alone[name]
    _, after = _call(dev, arena)
    for f in range(len(counts)):
        assert torch.equal(after[f * arena.stride:(f + 1) * arena.stride], expected[f * arena.stride:(f + 1) * arena.stride]), f


def test_null_outputs_are_skipped(dev):
    """Any output pointer may be NULL: the others are written as before."""
    scene = scenes.build(3, 5, 4)
    full = _alone(dev, scene)
    for skipped in OUTPUTS:
        arena = Arena(3, 5)
        arena.put(0, scene, header=False)
        _, after = _call(dev, arena, header=False, null=(skipped,))
        for name in OUTPUTS:
            got = arena.view(name, 0, after)
            if name == skipped:                                    # (bytes: the fill is NaN, which equals nothing as a float)
                assert torch.equal(got.contiguous().view(torch.uint8), arena.view(name, 0).contiguous().view(torch.uint8)), name
            else:
                assert torch.equal(got.contiguous().view(torch.uint8), full[name].contiguous().view(torch.uint8)), (skipped, name)


def test_invalid_arguments_are_refused(dev):
    """V = 33, N = 65, a null gt_boxes, and two frames with a stride of 100 bytes: a negative code each, and nothing is written (the call
    returns before any launch)."""
    scene = scenes.build(3, 5, 4)
    arena = Arena(3, 5)
    arena.put(0, scene, header=False)
    cases = {"V = 33": dict(frame=_frame_config(33, 5)), "N = 65": dict(frame=_frame_config(3, 65)), "null gt_boxes": dict(null=("gt",)),
             "stride 100": dict(frame=_frame_config(3, 5, B=2, stride=100))}
    for label, arguments in cases.items():
        code, after = _call(dev, arena, header=False, expect_ok=False, **arguments)
        assert code < 0, label
        assert torch.equal(after, arena.host), label


def test_a_config_without_steps_is_accepted(dev):
    """Of its config the call reads the sizes, the image, the guard, the ranges and the batch fields: num_steps = 0, which the prologues and
    the epilogue refuse, is accepted and writes the bytes of the call with a fully filled config (one frame, V = 1, N = 1)."""
    arena = Arena(1, 1)
    arena.put(0, scenes.build(1, 1, 0), header=False)
    _, full = _call(dev, arena, header=False)
    code, lenient = _call(dev, arena, header=False, frame=_frame_config(1, 1, num_steps=0))
    assert code == 0 and not torch.equal(full, arena.host)
    assert torch.equal(lenient, full)
