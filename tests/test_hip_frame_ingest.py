"""vsrd_frame_ingest (csrc/frame_ingest.h): a frame pack straight into soft masks, importance weights, ground-truth boxes and visibility,
against the reference's golden soft rasteriser data, against the CPU oracle with the re-indexing of scripts/main.py:204-255 restated here,
and through FrameBatch.reset.  Needs a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, margin
from oracle import geometry as ogeometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SENTINEL = -7.0
TEMPERATURE = 10.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _cameras(views):
    return np.tile(np.eye(3, dtype=np.float32), (views, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (views, 1, 1))


def _make_pack(image_size, view_entries):
    """view_entries: per view a list of (id, polygon [P,2] int, mask [H,W] bool)."""
    from vsrd_amd import frames
    offsets, ids, polygons, masks = [0], [], [], []
    for entries in view_entries:
        for instance, polygon, mask in entries:
            ids.append(instance); polygons.append(np.asarray(polygon, dtype=np.int32).reshape(-1, 2)); masks.append(np.packbits(mask, axis=-1))
        offsets.append(len(ids))
    intrinsics, extrinsics = _cameras(len(view_entries))
    return frames.validate(frames.FramePack(tuple(image_size), intrinsics, extrinsics, np.asarray(offsets, dtype=np.int64), np.asarray(ids, dtype=np.int64),
                                            np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int64),
                                            np.concatenate(polygons).astype(np.int32), np.stack(masks)))


def _run(dev, pack, capacity):
    """The four outputs of one call, every buffer pre-filled with the sentinel."""
    from vsrd_amd import frames
    H, W = pack.image_size
    V = pack.num_views
    soft = torch.full((V * H * W, capacity), SENTINEL, device=dev)
    weights = torch.full((V * H * W,), SENTINEL, device=dev)
    boxes = torch.full((V, capacity, 4), SENTINEL, device=dev)
    visible = torch.full((V, capacity), 9, dtype=torch.uint8, device=dev)
    frames.ingest_into(pack, dev, capacity, soft_masks=soft, sampling_weights=weights, gt_boxes=boxes, visible=visible, temperature=TEMPERATURE)
    torch.cuda.synchronize()
    return soft, weights, boxes, visible


def test_g11_through_the_ingest_kernel(dev):
    """The three golden polygons as the instances of one view, the golden inside masks packed: the soft masks meet the reference's own at the
    tolerance of test_hip_step.py::test_soft_rasterizer_g11."""
    g = load_golden("g11_soft_rasterizer")
    H, W = (int(v) for v in g["hw"])
    entries = [(k, g[f"polygon_{k}"].numpy(), g[f"inside_{k}"].numpy().astype(bool)) for k in range(3)]
    assert all(np.array_equal(np.asarray(p, dtype=np.int32), np.asarray(p)) for _, p, _ in entries)       # (contours are integer pixels)
    pack = _make_pack((H, W), [entries])
    assert abs(float(g["temperature"]) - TEMPERATURE) == 0.0
    soft, weights, boxes, visible = _run(dev, pack, 4)
    soft = soft.view(H, W, 4).cpu()
    for k in range(3):
        margin("frame_ingest_g11", f"soft_{k}", (soft[..., k] - g[f"soft_{k}"]).abs().max(), 1e-5)
        torch.testing.assert_close(soft[..., k], g[f"soft_{k}"], rtol=1e-5, atol=1e-5)
    assert bool((soft[..., 3] == SENTINEL).all()) and visible.cpu()[0].tolist() == [1, 1, 1, 9]


# ---- parity with the oracle --------------------------------------------------------------------------------------------------------------

HEIGHT, WIDTH = 40, 59            # neither a multiple of the 512 pixels of a workgroup nor of 8 bits


def _ellipse(cx, cy, a, b, vertices):
    angles = np.linspace(0.0, 2.0 * np.pi, vertices, endpoint=False)
    polygon = np.stack([np.clip(np.round(cx + a * np.cos(angles)), 0, WIDTH - 1), np.clip(np.round(cy + b * np.sin(angles)), 0, HEIGHT - 1)], -1).astype(np.int32)
    ys, xs = np.mgrid[0:HEIGHT, 0:WIDTH]
    return polygon, ((xs - cx) / a) ** 2 + ((ys - cy) / b) ** 2 <= 1.0


def _parity_pack(chunk, target_ids):
    """V = 3.  View 0: the target.  View 1 lacks 33, and its entry of 44 has no set bit (invisible as well).  View 2 lists its instances in
    another order, with an id (99) the target does not have.  One polygon has a single vertex, one has two, one has more than the kernel's
    staging chunk (consecutive vertices repeat at this image size: sides of length zero, which the + 1e-6 of the reference covers)."""
    single = (np.array([[17, 9]]), np.zeros((HEIGHT, WIDTH), dtype=bool))
    single[1][9, 17] = True
    line = (np.array([[5, 30], [50, 12]]), np.zeros((HEIGHT, WIDTH), dtype=bool))
    line[1][30, 5] = line[1][12, 50] = True
    shapes = {
        (0, 11): _ellipse(20, 18, 12, 9, 17), (0, 22): single, (0, 33): _ellipse(40, 25, 15, 10, chunk + 37), (0, 44): line, (0, 55): _ellipse(58, 0, 9, 7, 12),
        (1, 11): _ellipse(22, 18, 11, 9, 9), (1, 22): _ellipse(30, 8, 6, 5, 2 * chunk + 1), (1, 44): (_ellipse(8, 30, 5, 4, 6)[0], np.zeros((HEIGHT, WIDTH), dtype=bool)),
        (1, 55): _ellipse(50, 30, 7, 8, 5),
        (2, 55): _ellipse(45, 20, 10, 12, 31), (2, 99): _ellipse(10, 10, 8, 8, 8), (2, 22): line, (2, 11): single, (2, 44): _ellipse(0, 39, 14, 11, 23),
        (2, 33): _ellipse(30, 20, 25, 15, 64),
    }
    orders = [[11, 22, 33, 44, 55], [11, 22, 44, 55], [55, 99, 22, 11, 44, 33]]
    orders[0] = list(target_ids)
    return _make_pack((HEIGHT, WIDTH), [[(i, *shapes[(view, i)]) for i in order] for view, order in enumerate(orders)])


_EXPECTED = {}


def _distance_map_f64(polygon, image_size):
    """oracle.geometry.polygon_distance_map (SoftRasterizer.make_distance_map, geometric_transforms.py:265-290) restated in float64: the
    oracle's function casts to float32 itself, so the float64 reference repeats its formula term by term; _expected checks the two
    against each other."""
    height, width = image_size
    ys, xs = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
    pixels = torch.stack([xs.flatten(), ys.flatten()], dim=-1).to(torch.float64)
    start = polygon.to(torch.float64)
    side = torch.roll(start, shifts=-1, dims=0) - start
    rel = pixels[:, None, :] - start[None, :, :]
    ratio = ((side[None] * rel).sum(-1, keepdim=True) / ((side * side).sum(-1, keepdim=True)[None] + 1.0e-6)).clamp(0.0, 1.0)
    return (rel - side[None] * ratio).norm(dim=-1).min(dim=-1).values.reshape(height, width)


def _expected(pack):
    """The float64 CPU restatement: SoftRasterizer's distance map in float64 (checked against oracle.geometry.polygon_distance_map, which
    evaluates in float32: they agree to float32 rounding of distances of up to 72 pixels), oracle.geometry.soft_mask on it, BoxGenerator's
    extremes of the set pixels, and main.py:204-255's re-indexing -- index of the target's id in the view, zero padding where it is absent.
    Computed once per pack and shared."""
    key = tuple(pack.instance_ids[:pack.num_instances].tolist())
    if key in _EXPECTED:
        return _EXPECTED[key]
    H, W = pack.image_size
    V, N = pack.num_views, pack.num_instances
    target = pack.instance_ids[:N].tolist()
    soft = torch.zeros(V, H, W, N, dtype=torch.float64)
    boxes = torch.zeros(V, N, 4)
    visible = torch.zeros(V, N, dtype=torch.uint8)
    for view in range(V):
        first, last = int(pack.view_offsets[view]), int(pack.view_offsets[view + 1])
        own = pack.instance_ids[first:last].tolist()
        for slot, instance in enumerate(target):
            if instance not in own:
                continue
            entry = first + own.index(instance)
            mask = torch.from_numpy(np.unpackbits(pack.inside[entry], axis=-1)[:, :W].astype(bool))
            if not bool(mask.any()):
                continue
            polygon = torch.from_numpy(pack.polygon_vertices[pack.polygon_offsets[entry]:pack.polygon_offsets[entry + 1]])
            distances = _distance_map_f64(polygon, (H, W))
            torch.testing.assert_close(ogeometry.polygon_distance_map(polygon, (H, W)).to(torch.float64), distances, rtol=1e-5, atol=1e-5)
            soft[view, :, :, slot] = ogeometry.soft_mask(distances, mask, TEMPERATURE)
            assert soft.dtype == torch.float64
            ys, xs = torch.nonzero(mask, as_tuple=True)
            boxes[view, slot] = torch.tensor([xs.min(), ys.min(), xs.max(), ys.max()], dtype=torch.float32)
            visible[view, slot] = 1
    _EXPECTED[key] = (soft, boxes, visible)
    return _EXPECTED[key]


@pytest.mark.parametrize("instances,capacity", [(5, 8), (5, 5), (1, 8), (1, 1)], ids=["n5_cap8_vector", "n5_cap5_scalar", "n1_cap8", "n1_cap1"])
def test_parity_with_the_oracle(dev, instances, capacity):
    from vsrd_amd import frames
    chunk = frames.staging_chunk()
    assert 1 <= chunk <= 4096
    pack = _parity_pack(chunk, [11, 22, 33, 44, 55][:instances])
    counts = np.diff(pack.polygon_offsets)
    assert pack.num_instances == instances and counts.max() > 2 * chunk
    if instances == 5:
        assert 1 in counts and 2 in counts and counts[2] > chunk
    want_soft, want_boxes, want_visible = _expected(pack)
    N, V = instances, 3
    soft, weights, boxes, visible = _run(dev, pack, capacity)
    got = soft.view(V, HEIGHT, WIDTH, capacity)
    margin(f"frame_ingest_parity[{instances}-{capacity}]", "soft masks", (got[..., :N].cpu().to(torch.float64) - want_soft).abs().max(), 1e-5)
    torch.testing.assert_close(got[..., :N].cpu().to(torch.float64), want_soft, rtol=1e-5, atol=1e-5)
    # invisible pairs: exact zeros (the reference's zero padding)
    hidden = want_visible == 0
    if instances == 5:
        assert hidden.tolist() == [[False] * 5, [False, False, True, True, False], [False] * 5]
    for view, slot in torch.nonzero(hidden).tolist():
        assert bool((got[view, :, :, slot] == 0.0).all()) and not bool(torch.signbit(got[view, :, :, slot]).any())
    # the importance weights: bit-equal to amax over the written columns
    assert torch.equal(weights, soft[:, :N].amax(dim=-1))
    # the row's other columns still hold what they held
    assert bool((soft[:, N:] == SENTINEL).all()) and bool((boxes[:, N:] == SENTINEL).all()) and bool((visible[:, N:] == 9).all())
    assert torch.equal(boxes[:, :N].cpu(), want_boxes) and torch.equal(visible[:, :N].cpu(), want_visible)
    # the materialised form is the same call at stride N
    inputs = frames.ingest(pack, dev, temperature=TEMPERATURE)
    assert inputs.soft_masks.shape == (V, HEIGHT, WIDTH, N) and torch.equal(inputs.soft_masks, got[..., :N])
    assert torch.equal(inputs.boxes_2d.reshape(V, N, 4).cpu(), want_boxes) and torch.equal(inputs.visible_masks.cpu(), want_visible.bool())
    # outputs are optional
    frames.ingest_into(pack, dev, capacity, sampling_weights=weights.fill_(SENTINEL), temperature=TEMPERATURE)
    torch.cuda.synchronize()
    assert torch.equal(weights, soft[:, :N].amax(dim=-1))


def test_invalid_arguments_are_refused(dev):
    from vsrd_amd import _lib, frames
    pack = _parity_pack(frames.staging_chunk(), [11, 22, 33, 44, 55])
    soft = torch.zeros(3 * HEIGHT * WIDTH, 4, device=dev)
    with pytest.raises(ValueError):
        frames.ingest_into(pack, dev, 8, soft_masks=soft)                 # a buffer that does not match the stride
    with pytest.raises(_lib.VsrdHipError):
        frames.ingest_into(pack, dev, 4, soft_masks=soft)                 # a stride below N
    with pytest.raises(_lib.VsrdHipError):
        frames.ingest_into(pack, "cpu", 8)


# ---- through FrameBatch.reset ------------------------------------------------------------------------------------------------------------

def _config():
    from vsrd_amd import optimization
    return optimization.OptimizationConfig(num_samples=40, num_rays=64, warmup_steps=2, num_steps=8, seed=3, mlp_adjoint_item_slots=8)


def _synthetic_pack(frame, instances):
    import make_frame_packs
    return make_frame_packs.make_pack(frame, 2, 24, 40, instances, drop=[(1, 0)] if instances > 2 else (), shuffle=True)


def _state(member):
    det, b, n = member.detector, member._glue, member.num_instances
    tensors = [det.locations, det.dimensions, det.orientations, det.embeddings, *member.hyper_distance_field.parameters()]
    tensors += [b["record"], b["ray_indices"], b["gt_boxes"][:, :n], b["visible"][:, :n], member.flat_masks[:, :n], member.sampling_weights, member.ray_directions,
                b["extrinsics"], b["intrinsics"]]
    return [t.detach().clone() for t in tensors]


def _batch(dev, pack):
    from vsrd_amd import frames, optimization
    founder = frames.ingest(pack, dev)
    return optimization.FrameBatch([founder, founder], _config(), dev, init_seeds=[1, 2], max_instances=4)


def test_reset_in_place_equals_reset_from_materialised_inputs(dev):
    """Row 0 is reset from the pack (the kernel writes into the row), row 1 from frames.ingest(pack) (the strided copy and amax of the
    FrameInputs path): four steps, across the phase switch, give the same parameters and the same loss, bit for bit."""
    from vsrd_amd import frames
    pack = _synthetic_pack(8, 3)
    batch = _batch(dev, pack)
    assert batch.reset(0, pack, init_seed=11)
    assert batch.reset(1, frames.ingest(pack, dev), init_seed=11)
    member = batch.frames[0]
    assert member.num_instances == 3 and member.capacity == 4 and tuple(member.inputs.image_size) == (24, 40)
    assert member.inputs.soft_masks.shape == (2, 24, 40, 3) and member.inputs.soft_masks.data_ptr() == member.flat_masks.data_ptr()
    assert member.inputs.visible_masks.cpu()[1].tolist() == [False, True, True]
    for index, (a, b) in enumerate(zip(_state(batch.frames[0]), _state(batch.frames[1]))):
        assert torch.equal(a, b), index
    batch.run(4)
    torch.cuda.synchronize()
    assert batch.frames[0].step_index == 4
    for index, (a, b) in enumerate(zip(_state(batch.frames[0]), _state(batch.frames[1]))):
        assert torch.equal(a, b), index
    assert torch.equal(batch.outputs(0)["loss"], batch.outputs(1)["loss"]) and bool(torch.isfinite(batch.outputs(0)["loss"]))
    # what a reset from a pack leaves in `inputs` (views of the row) starts the same frame again: capture_all() ends with reset(self.inputs)
    member = batch.frames[0]
    assert member.inputs.soft_masks.data_ptr() == member.flat_masks.data_ptr()
    assert batch.reset(0, member.inputs, init_seed=11) and batch.reset(1, frames.ingest(pack, dev), init_seed=11)
    for index, (a, b) in enumerate(zip(_state(batch.frames[0]), _state(batch.frames[1]))):
        assert torch.equal(a, b), index
    with pytest.raises(ValueError):
        batch.reset(0, _synthetic_pack(8, 5))                              # more instances than the row's capacity
    batch.close()


def test_resetting_a_row_twice_equals_resetting_a_fresh_row_once(dev):
    big, small = _synthetic_pack(3, 4), _synthetic_pack(8, 2)
    batch = _batch(dev, big)
    assert batch.reset(0, big, init_seed=21)
    assert batch.reset(0, small, init_seed=22)
    assert batch.reset(1, small, init_seed=22)
    assert batch.frames[0].num_instances == batch.frames[1].num_instances == 2
    for index, (a, b) in enumerate(zip(_state(batch.frames[0]), _state(batch.frames[1]))):
        assert torch.equal(a, b), index
    batch.run(2)
    torch.cuda.synchronize()
    for index, (a, b) in enumerate(zip(_state(batch.frames[0]), _state(batch.frames[1]))):
        assert torch.equal(a, b), index
    batch.close()
