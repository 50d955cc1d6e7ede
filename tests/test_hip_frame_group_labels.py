"""csrc/frame_group_labels.h -- vsrd_frame_group_labels, a frame's pseudo-labels in the views of its GROUP (label views of the call's own,
up to VSRD_MAX_LABEL_VIEWS, three kernels inside the one call) -- through the C ABI with buffers of the test's own, and through the loops.

Every ABI call works on ONE arena of the test's own, laid out like a frame batch's rows (every buffer at the same offset of its frame's row,
rows `stride` bytes apart, 256 spare bytes between them), filled with NaN bits (the int64 output with -7) before the inputs are written:
what a call did not write is found by comparing bytes.

Where the bounds come from: they are the rules of tests/test_hip_frame_labels.py (its `_check` is the function that applies them here) with
the label-view count L in place of V -- camera corners 2 x the float32 oracle's own distance + the float32 spacing of the largest magnitude,
boxes frame_glue_scenes.box_tolerance(floor), mean_iou against the float64 formula on the device's own boxes (L + 16) 2^-24 (one IoU <= 1
is about ten float32 roundings, the sum of at most L terms <= 1 divided by its count adds at most L half-spacings of 1; the views are summed
in ascending order), end to end 2 x floor + that bound, exact +0.0 where the formula is 0 or no view sees the slot, the assignment scipy's on
the device's own matrix, the confidences the matched entries bit for bit.  With a row's own views as label views nothing is bounded: the
five outputs are vsrd_frame_labels' bits."""
import pytest
import torch

import frame_glue_scenes as scenes
import test_hip_frame_labels as labels_test
from conftest import margin
from frame_rows import RowArena
from oracle import frame_glue as ref

pytestmark = pytest.mark.gpu

NAN_BITS = labels_test.NAN_BITS
GAP = labels_test.GAP
INPUTS = ("loc", "dim", "ori", "count", "E", "K", "gt", "visible", "header")
OUTPUTS = labels_test.OUTPUTS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


class Arena(RowArena):
    """B rows laid out for L label views and a capacity of N boxes, filled with NaN bits (the int64 output with -7)."""

    def __init__(self, L, N, B=1):
        f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
        fields = [("loc", (N, 3), f32), ("dim", (N, 3), f32), ("ori", (N, 2), f32), ("count", (1,), i32), ("E", (L, 16), f32), ("K", (L, 9), f32),
                  ("gt", (L, N, 4), f32), ("visible", (L, N), u8), ("header", (2,), i32), ("camera_corners", (L, N, 8, 3), f32),
                  ("boxes_2d", (L, N, 4), f32), ("mean_iou", (N, N), f32), ("matched_gt", (N,), i64), ("confidences", (N,), f32)]
        super().__init__(fields, B, NAN_BITS, GAP)
        self.L, self.N = L, N
        for f in range(B):
            self.view("matched_gt", f).fill_(-7)

    def put(self, f, scene, header=True, count=True):
        """Frame f's inputs: the scene's l views and n boxes in the leading corner of the row's tables (the rest keeps the fill)."""
        l, n = scene["visible"].shape
        raw = scene["raw"].float()
        self.view("loc", f)[:n], self.view("dim", f)[:n], self.view("ori", f)[:n] = raw[:, 0:3], raw[:, 3:6], raw[:, 6:8]
        self.view("E", f)[:l] = scene["E"].float().reshape(l, 16)
        self.view("K", f)[:l] = scene["K"].float().reshape(l, 9)
        self.view("gt", f)[:l, :n] = scene["gt_boxes"].float()
        self.view("visible", f)[:l, :n] = scene["visible"].to(torch.uint8)
        if count:
            self.view("count", f)[0] = l
        if header:
            self.write_header(f, n)


def _call(dev, arena, header=True, count=True, frame=None, L=None, null=(), expect_ok=True):
    """One vsrd_frame_group_labels call on the arena -> (return code, the arena's bytes afterwards, on the host)."""
    from vsrd_amd import _lib
    lib = _lib.load()
    device = arena.host.to(dev)
    pointer = arena.pointers(device, null)
    if frame is None:           # (num_views is not read: 1 would do as well as anything)
        frame = labels_test._frame_config(1, arena.N, arena.B, arena.stride if arena.B > 1 else 0)
    code = lib.vsrd_frame_group_labels(frame, pointer("loc"), pointer("dim"), pointer("ori"), arena.L if L is None else L,
                                       pointer("count") if count else None, pointer("E"), pointer("K"), pointer("gt"), pointer("visible"),
                                       *[pointer(name) for name in OUTPUTS], pointer("header") if header else None, _lib.stream())
    torch.cuda.synchronize()
    if expect_ok:
        _lib.check(code)
    return code, device.cpu()


def _alone(dev, scene):
    """The scene in a call of its own: by-value L = l and N = n, no count, no header -> {output name: host tensor}."""
    l, n = scene["visible"].shape
    arena = Arena(l, n)
    arena.put(0, scene, header=False, count=False)
    _, after = _call(dev, arena, header=False, count=False)
    before = arena.host
    for name in INPUTS:                                            # nothing but the outputs changed
        assert torch.equal(arena.view(name, 0, after).view(torch.uint8), arena.view(name, 0, before).view(torch.uint8)), name
    assert torch.equal(after[-GAP:], before[-GAP:])
    return {name: arena.view(name, 0, after).clone() for name in OUTPUTS}


def _bits(tensor):
    return tensor.contiguous().view(torch.uint8)


# ---- 1. the row's own views as label views: vsrd_frame_labels' bits --------------------------------------------------------------------
SAME = [(1, 1, 0), (3, 5, 4), (17, 16, 2), (32, 64, 2)]            # (V, N, seed)


@pytest.mark.parametrize("V,N,seed", SAME, ids=[f"{v}x{n}" for v, n, _ in SAME])
def test_same_views_same_bits(dev, V, N, seed):
    scene = scenes.build(V, N, seed)
    expected, got = labels_test._alone(dev, scene), _alone(dev, scene)
    for name in OUTPUTS:
        assert torch.equal(_bits(got[name]), _bits(expected[name])), name


# ---- 2. beyond the frame glue's 32 views, against the float64 oracle -----------------------------------------------------------------
BEYOND = [(33, 5, 4), (100, 16, 2), (257, 64, 1)]                  # (L, N, seed)


@pytest.mark.parametrize("L,N,seed", BEYOND, ids=[f"{l}x{n}" for l, n, _ in BEYOND])
def test_beyond_32_views_against_the_float64_reference(dev, L, N, seed):
    scene = scenes.build(L, N, seed)
    label = f"test_beyond_32_views_against_the_float64_reference[{L}x{N}]"
    forward = labels_test._check(label, scene, _alone(dev, scene))
    # what the comparison relies on: most of the pairs have a clipped box with area in the float64 reference (the IoUs are not all 0)
    boxes = forward["boxes"]
    with_area = ((boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1]) > 0).double().mean()
    margin(label, "share of pairs without area", 1.0 - float(with_area), 0.5)
    assert float(with_area) >= 0.5, (label, float(with_area))
    assert bool(scene["visible"].any(dim=0).all())                 # no slot is unseen


# ---- 3. per-frame counts in a batch ----------------------------------------------------------------------------------------------------
def _expect(arena, f, expected, alone, l, n):
    for name in ("camera_corners", "boxes_2d"):
        arena.view(name, f, expected)[:l, :n] = alone[name]
    arena.view("mean_iou", f, expected)[:n, :n] = alone["mean_iou"]
    for name in ("matched_gt", "confidences"):
        arena.view(name, f, expected)[:n] = alone[name]


def test_batch_with_per_frame_counts(dev):
    """B = 3 frames with (1, 40, 100) label views and (3, 8, 13) boxes in rows of capacity L = 100, N = 13: every frame's outputs are the bits
    of its call alone; views l_f .. 99, instances n_f .. 12 and the bytes between the rows keep the fill."""
    capacity_l, capacity_n, views, counts = 100, 13, (1, 40, 100), (3, 8, 13)
    arena = Arena(capacity_l, capacity_n, B=len(counts))
    frames = [scenes.build(l, n, 10 + k) for k, (l, n) in enumerate(zip(views, counts))]
    for f, scene in enumerate(frames):
        arena.put(f, scene)
    expected = arena.host.clone()
    for f, (scene, l, n) in enumerate(zip(frames, views, counts)):
        _expect(arena, f, expected, _alone(dev, scene), l, n)
    _, after = _call(dev, arena)
    assert not torch.equal(after, arena.host)
    for f in range(len(counts)):
        assert torch.equal(after[f * arena.stride:(f + 1) * arena.stride], expected[f * arena.stride:(f + 1) * arena.stride]), f


def test_null_count_means_every_view(dev):
    """label_view_count = NULL in a row with a header: all L views of the row, the header's n boxes."""
    l, capacity, n = 40, 13, 8
    scene = scenes.build(l, n, 11)
    arena = Arena(l, capacity)
    arena.put(0, scene, count=False)
    expected = arena.host.clone()
    _expect(arena, 0, expected, _alone(dev, scene), l, n)
    _, after = _call(dev, arena, count=False)
    assert torch.equal(after, expected)


# ---- 4. the hand-made scene at L = 40 --------------------------------------------------------------------------------------------------
def _hand_made_scene(L=40):
    """tests/test_hip_frame_labels.py::_hand_made_scene with L label views, 4 boxes: ground-truth boxes of zero area (xmin = xmax: slot 0 in
    view 1, slot 3 in every view), a slot no view sees (2), and a prediction (3) whose clipped box has zero area in every view (49 m to the
    left at 3 m depth).  Row 3 and columns 2 and 3 of the matrix are all zero: predictions 2 and 3 can take slots 2 and 3 either way round
    at the same total, and the tie rule decides."""
    scene = scenes.build(L, 4, 5)
    scene["visible"][:] = True
    scene["gt_boxes"] = ref.forward(scene["raw"], scene["E"], scene["K"], scenes.IMAGE_SIZE)["boxes"][:, torch.tensor([1, 0, 3, 2])] + 2.5
    scene["raw"][3, 0] = torch.logit(torch.tensor(0.01, dtype=torch.float64))
    scene["raw"][3, 2] = torch.logit(torch.tensor(0.03, dtype=torch.float64))
    scene["gt_boxes"][1, 0, 2] = scene["gt_boxes"][1, 0, 0]
    scene["gt_boxes"][:, 3, 2] = scene["gt_boxes"][:, 3, 0]
    scene["visible"][:, 2] = False
    scene["gt_boxes"][:, 2] = 0.0
    return scene


def test_hand_made_scene(dev):
    scene = _hand_made_scene()
    out = _alone(dev, scene)
    forward = labels_test._check("test_hand_made_scene", scene, out)            # (the assignment is scipy's: the tie included)
    boxes = forward["boxes"]
    assert bool(((boxes[:, 3, 2] - boxes[:, 3, 0]) == 0).all())                 # the prediction without area, in every view
    assert bool((out["mean_iou"][3].view(torch.int32) == 0).all()) and bool((out["mean_iou"][:, 2:].view(torch.int32) == 0).all())
    assert float(out["mean_iou"][0, 1]) > 0.3 and float(out["mean_iou"][1, 0]) > 0.3         # the others overlap their ground truth
    assert float(out["confidences"][3]) == 0.0


# ---- 5. rejections: argument checks on the host side of the ABI ----------------------------------------------------------------------
def test_invalid_arguments_are_refused(dev):
    """NULL boxes_2d, mean_iou or label_gt_boxes, L = 0 and L = 4097, N = 65: VSRD_E_INVALID_ARGUMENT each, and nothing is written (the call
    returns before any launch)."""
    from vsrd_amd import _lib
    scene = scenes.build(3, 5, 4)
    arena = Arena(3, 5)
    arena.put(0, scene, header=False)
    cases = {"null boxes_2d": dict(null=("boxes_2d",)), "null mean_iou": dict(null=("mean_iou",)), "null label_gt_boxes": dict(null=("gt",)),
             "L = 0": dict(L=0), "L = 4097": dict(L=_lib.MAX_LABEL_VIEWS + 1), "N = 65": dict(frame=labels_test._frame_config(1, 65))}
    for label, arguments in cases.items():
        code, after = _call(dev, arena, header=False, expect_ok=False, **arguments)
        assert code == _lib.E_INVALID_ARGUMENT, label
        assert torch.equal(after, arena.host), label


def test_a_config_without_views_or_steps_is_accepted(dev):
    """Of its config the call reads num_boxes, the image, the guard, the ranges and the batch fields: num_views = 0 and num_steps = 0, which
    vsrd_frame_labels and the prologues refuse, are accepted and write the bytes of the call with a fully filled config (one frame, L = 1,
    N = 1)."""
    arena = Arena(1, 1)
    arena.put(0, scenes.build(1, 1, 0), header=False, count=False)
    _, full = _call(dev, arena, header=False, count=False)
    code, lenient = _call(dev, arena, header=False, count=False, frame=labels_test._frame_config(0, 1, num_steps=0))
    assert code == 0 and not torch.equal(full, arena.host)
    assert torch.equal(lenient, full)


# ---- 6. through the loops ----------------------------------------------------------------------------------------------------------------
KEYS = ("boxes_3d", "boxes_2d", "confidences", "matched_gt", "mean_iou", "frame_ids")


def _loop_config(**more):
    from vsrd_amd import optimization
    return optimization.OptimizationConfig(num_samples=40, num_rays=64, warmup_steps=3, num_steps=12, seed=3, mlp_adjoint_item_slots=8, **more)


def _loop_inputs(dev, frame, n, label_views):
    from vsrd_amd import launcher
    return launcher.synthetic_frame_inputs(dev, frame, 2, n, height=32, width=64, label_views=label_views)


def _snapshot(result):
    return {key: value.detach().cpu().clone() for key, value in result.items()}


def _same(got, want):
    assert tuple(got) == KEYS == tuple(want)
    for key in KEYS:
        assert got[key].shape == want[key].shape and torch.equal(_bits(got[key]), _bits(want[key])), key


def _direct(dev, loop):
    """vsrd_frame_group_labels through the C ABI on copies of the loop's parameters and of its frame's group -> what group_labels() returns."""
    from vsrd_amd import _lib
    inputs, det, n = loop.inputs, loop.detector, loop.num_instances
    l = int(inputs.label_frame_ids.shape[0])
    scene = dict(raw=torch.cat([det.locations.data[0], det.dimensions.data[0], det.orientations.data[0]], dim=-1).cpu(), E=inputs.label_extrinsic_matrices.cpu(),
                 K=inputs.label_intrinsic_matrices.cpu(), gt_boxes=inputs.label_boxes_2d.cpu(), visible=inputs.label_visible.cpu())
    arena = Arena(l, n)
    arena.put(0, scene, header=False, count=False)
    frame = _lib.FrameConfig.from_buffer_copy(loop._frame)         # (the loop's image size, guard and ranges)
    frame.num_boxes, frame.num_frames, frame.frame_stride = n, 1, 0
    _, after = _call(dev, arena, header=False, count=False, frame=frame)
    out = {name: arena.view(name, 0, after).clone() for name in OUTPUTS}
    return dict(boxes_3d=out["camera_corners"], boxes_2d=out["boxes_2d"].unflatten(-1, (2, 2)), confidences=out["confidences"], matched_gt=out["matched_gt"],
                mean_iou=out["mean_iou"], frame_ids=inputs.label_frame_ids.cpu())


def test_loops_a_loop_and_its_resets(dev):
    """FrameOptimizer.group_labels() after a few steps is a direct ABI call on copies of its tensors; a reset() to a frame with another group
    gives that frame's result (no step needed); a frame with more label views than the loop was laid out for, and a frame without a
    group, are ValueErrors."""
    from vsrd_amd import optimization
    first, second = _loop_inputs(dev, 3, 3, 5), _loop_inputs(dev, 4, 3, 9)
    with pytest.raises(ValueError):
        optimization.FrameOptimizer(second, _loop_config(init_seed=70), dev, graph=True, persistent=True, max_label_views=5)
    loop = optimization.FrameOptimizer(first, _loop_config(init_seed=70), dev, graph=True, persistent=True, max_label_views=9)
    loop.run(4, steps_per_graph=1)
    got = _snapshot(loop.group_labels())
    torch.cuda.synchronize()
    assert got["boxes_3d"].shape == (5, 3, 8, 3) and got["boxes_2d"].shape == (5, 3, 2, 2) and got["frame_ids"].tolist() == first.label_frame_ids.tolist()
    _same(got, _direct(dev, loop))
    # (four steps from a random start overlap nothing yet.)  With the frame's TRUE boxes as parameters every prediction meets its own ground
    # truth in the group's views: the assignment is the identity and the confidences are near 1
    from vsrd_amd import synthetic
    _, _, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(3, 2, 32, 64, 3)
    with torch.no_grad():
        loop.detector.locations.copy_(raw_loc); loop.detector.dimensions.copy_(raw_dim); loop.detector.orientations.copy_(raw_ori)
    true = _snapshot(loop.group_labels())
    torch.cuda.synchronize()
    _same(true, _direct(dev, loop))
    assert true["matched_gt"].tolist() == [0, 1, 2] and float(true["confidences"].min()) > 0.99, true["confidences"]
    assert loop.reset(second, init_seed=71)
    after = _snapshot(loop.group_labels())
    torch.cuda.synchronize()
    assert after["boxes_3d"].shape == (9, 3, 8, 3) and after["frame_ids"].tolist() == second.label_frame_ids.tolist()
    _same(after, _direct(dev, loop))
    with pytest.raises(ValueError):
        loop.reset(_loop_inputs(dev, 5, 3, 12), init_seed=72)
    assert loop.reset(_loop_inputs(dev, 5, 3, 0), init_seed=72)
    with pytest.raises(ValueError):
        loop.group_labels()
    loop.close()


def test_loops_a_batch_of_frames_with_different_groups(dev):
    """FrameBatch.group_labels(active) on frames of different L (and n): every frame gets what its own loop gives."""
    import dataclasses
    from vsrd_amd import optimization
    inputs = [_loop_inputs(dev, 3, 3, 5), _loop_inputs(dev, 4, 5, 9)]
    alone = []
    for k, frame in enumerate(inputs):
        loop = optimization.FrameOptimizer(frame, dataclasses.replace(_loop_config(), init_seed=70 + k), dev, graph=True, persistent=True)
        loop.run(4, steps_per_graph=1)
        alone.append(_snapshot(loop.group_labels()))
        torch.cuda.synchronize()
        loop.close()
    batch = optimization.FrameBatch(inputs, _loop_config(), dev, init_seeds=[70, 71], max_instances=8)
    assert batch.max_label_views == 9
    batch.run(4, steps_per_graph=1)
    got = [_snapshot(entry) for entry in batch.group_labels()]
    torch.cuda.synchronize()
    assert len(got) == 2 and got[0]["boxes_3d"].shape == (5, 3, 8, 3) and got[1]["boxes_3d"].shape == (9, 5, 8, 3)
    for f in range(2):
        _same(got[f], alone[f])
    _same(_snapshot(batch.group_labels(active=1)[0]), alone[0])
    batch.close()
