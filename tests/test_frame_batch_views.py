"""Frame batches over frames that differ in VIEW count (include/vsrd_hip.h, ABI 12): the rows of a FrameBatch(max_views=...) are laid out
for a view capacity, every per-view array is view-major, so a frame with fewer views fills a prefix of each, and its header carries its own
v_f and v_f H W.  Each frame must walk, bit for bit, the trajectory it walks alone in a frame slot of its own (V, N); the views beyond v_f
(and the instances beyond n_f) of a row must be neither read nor written; and the three kernels that see a view count -- the prologue, its
sampler half, the label kernel -- must give, under a header, the bits of the same call on contiguous [v_f, n_f] arrays."""
import ctypes
import math
import os
import sys

import pytest
import torch

import frame_glue_scenes as scenes
import test_hip_frame_glue as glue
import test_hip_frame_labels as labels_test

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

SHAPES = [(3, 4), (1, 2), (4, 6), (2, 1), (4, 5), (2, 3)]          # (views, instances): V = 1 (the target view alone) and v_f = V_cap on purpose
CAPACITY, VIEW_CAPACITY = 6, 4
STEPS = 26
NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _config(split_bf16):
    from vsrd_amd import optimization
    # (the configuration of tests/test_frame_batch_mixed.py: across the phase switch at step 9, the split-ray kernels of the batch)
    return optimization.OptimizationConfig(num_samples=40, num_rays=128, warmup_steps=9, num_steps=40, seed=3, mlp_adjoint_item_slots=8,
                                           mlp_split_bf16=split_bf16)


def _inputs(dev, frame, views, n, height=128, width=128, label_views=0):
    from vsrd_amd import launcher
    return launcher.synthetic_frame_inputs(dev, frame, views, n, height=height, width=width, label_views=label_views)


def _state(loop):
    det, b = loop.detector, loop._glue
    n = loop.num_instances
    tensors = [det.locations, det.dimensions, det.orientations, det.embeddings]
    tensors += [loop.optimizer.state[p][key] for p in (det.locations, det.dimensions, det.orientations) for key in ("exp_avg", "exp_avg_sq", "step")]
    tensors += [g["lr"] for g in loop.optimizer.param_groups]
    tensors += [loop.optimizer.state[det.embeddings][key] for key in ("exp_avg", "exp_avg_sq", "step")]
    tensors += list(loop.hyper_distance_field.parameters())
    tensors += [b["record"], b["raw_gradients"][:n], b["ray_indices"], b["instances"][:n], b["grad_mlp"][:n], b["grad_instances"][:n], b["mlp_weights"][:n]]
    return [t.detach().clone() for t in tensors]


def _pads(member):
    """(tensor, fill) pairs over what a row holds beyond its frame's own counts: the views v_f .. V_cap - 1 of every per-view buffer (the label
    outputs included), and the instances n_f .. N_cap - 1 of the frame's own views and of the per-instance tensors."""
    from vsrd_amd import optimization
    v, n, cap = member.num_views, member.num_instances, member.capacity
    pixels = v * member.pixels_per_view
    det, full, labels = member.detector, member._full, member._outputs["labels"]
    assert full["extrinsics"].shape[0] == member.view_capacity == VIEW_CAPACITY and full["flat_masks"].shape == (VIEW_CAPACITY * member.pixels_per_view, cap)
    pads = [(full[name][v:], "nan") for name in ("camera_positions", "extrinsics", "intrinsics", "gt_boxes")]
    pads += [(full[name][pixels:], "nan") for name in ("ray_directions", "flat_masks", "sampling_weights")]
    pads += [(full["visible"][v:], 1), (labels["camera_corners"][v:], "nan"), (labels["boxes_2d"][v:], "nan")]
    pads += [(full["flat_masks"][:pixels, n:], "nan"), (full["gt_boxes"][:v, n:], "nan"), (full["visible"][:v, n:], 1)]
    pads += [(labels["camera_corners"][:v, n:], "nan"), (labels["boxes_2d"][:v, n:], "nan"), (labels["mean_iou"][n:], "nan"), (labels["mean_iou"][:n, n:], "nan"),
             (labels["confidences"][n:], "nan")]
    for p in (det.locations, det.dimensions, det.orientations, det.embeddings):
        pads.append((optimization._instance_prefix(p.data, cap)[:, n:], "nan"))
        state = member.optimizer.state[p]
        for key in ("exp_avg", "exp_avg_sq"):
            pads.append((optimization._instance_prefix(state[key], cap)[:, n:], "nan"))
    return pads


def _fill_pads(member):
    for t, fill in _pads(member):
        t.fill_(float("nan") if fill == "nan" else fill)


def _pads_untouched(member):
    for index, (t, fill) in enumerate(_pads(member)):
        if fill == "nan":
            assert bool((t.contiguous().view(torch.int32) == NAN_BITS).all()), (index, t.shape)
        else:
            assert bool((t == fill).all()), (index, t.shape)


def _equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("split_bf16", [True, False], ids=["split_bf16", "fp32_mfma"])
def test_frames_of_different_view_counts_walk_their_own_trajectories(dev, split_bf16):
    """1 + 2 + 7: every frame alone in a slot of its own (V, N), then the six in a batch of four rows of capacity (4 views, 6 instances) as
    groups of 4 and 2; everything beyond a frame's own counts pre-filled and found unchanged after the run and after labels(); the refusals."""
    from vsrd_amd import formats, optimization
    config = _config(split_bf16)
    frames, alone, payloads, labels = [], [], [], []
    frame_number = 100
    for k, (views, n) in enumerate(SHAPES):
        while True:          # (frames whose soft masks do not suit the table sampler are skipped)
            inputs = _inputs(dev, frame_number, views, n)
            frame_number += 1
            try:
                slot = optimization.FrameOptimizer(inputs, config, dev, graph=True, persistent=True)
            except optimization.UnsuitableFrameError:
                continue
            break
        slot.capture_all()
        assert slot.reset(inputs, init_seed=70 + k)
        slot.run(STEPS)
        torch.cuda.synchronize()
        frames.append(inputs)
        alone.append(_state(slot))
        payloads.append(formats.checkpoint_payload(slot, STEPS, host=True))
        labels.append(formats.to_host(slot.labels()))
        slot.close()

    batch = optimization.FrameBatch(frames[:4], config, dev, init_seeds=[70, 71, 72, 73], max_instances=CAPACITY, max_views=VIEW_CAPACITY)
    assert all(row.layout == batch.arena.rows[0].layout for row in batch.arena.rows)
    assert [(m.num_views, m.num_instances) for m in batch.frames] == SHAPES[:4]
    assert all(m.capacity == CAPACITY and m.view_capacity == VIEW_CAPACITY for m in batch.frames)
    batch.capture_all(actives=[4, 2])
    for m in batch.frames:
        m._output_state("labels")                 # (the label outputs exist in every row before the pads are filled)
    for group, active in (([0, 1, 2, 3], 4), ([4, 5], 2)):
        for row, k in enumerate(group):
            assert batch.reset(row, frames[k], init_seed=70 + k)
            _fill_pads(batch.frames[row])
        batch.run(STEPS, active=active)
        torch.cuda.synchronize()
        group_labels = formats.to_host(batch.labels(active=active))
        torch.cuda.synchronize()
        for row, k in enumerate(group):
            member = batch.frames[row]
            assert member.step_index == STEPS and (member.num_views, member.num_instances) == SHAPES[k]
            for index, (a, b) in enumerate(zip(_state(member), alone[k])):
                assert a.shape == b.shape and torch.equal(a, b), (k, index)
            _pads_untouched(member)
            assert _equal(formats.checkpoint_payload(member, STEPS, host=True), payloads[k]), k
            assert batch.outputs(row)["raw_gradients"][0].shape == (1, SHAPES[k][1], 3)
            assert group_labels[row]["boxes_3d"].shape == (SHAPES[k][0], SHAPES[k][1], 8, 3)
            assert _equal(group_labels[row], labels[k]), k

    # refusals (ValueError naming the limit): 0 views, more views than the capacity, another image size
    first = frames[0]
    no_views = optimization.FrameInputs(first.image_size, first.intrinsic_matrices[:0], first.extrinsic_matrices[:0], first.soft_masks[:0],
                                        first.boxes_2d[:0], first.visible_masks[:0])
    for refused, word in ((no_views, "views"), (_inputs(dev, 7, VIEW_CAPACITY + 1, 3), "views"), (_inputs(dev, 7, 3, 3, height=96), "image size")):
        with pytest.raises(ValueError, match=word):
            batch.reset(0, refused, init_seed=1)
    batch.close()
    with pytest.raises(ValueError, match="max_views"):          # frames of different V without max_views
        optimization.FrameBatch(frames[:2], config, dev, max_instances=CAPACITY)
    with pytest.raises(ValueError, match="max_views"):          # a capacity below a frame's own count
        optimization.FrameBatch(frames[:2], config, dev, max_instances=CAPACITY, max_views=2)
    for outside in (0, 33):
        with pytest.raises(ValueError, match="max_views: 1..32"):
            optimization.FrameBatch(frames[:2], config, dev, max_instances=CAPACITY, max_views=outside)


ROWS = [  # (shapes (views, instances) of the two frames, width, label views of each frame's group, log, the batch's capacities)
    pytest.param([(2, 2), (3, 3)], 128, 2, True, dict(max_instances=4, max_views=3, max_label_views=2), id="capacities_group_log"),
    pytest.param([(2, 2), (3, 3)], 128, 2, True, dict(max_instances=4, max_views=3, max_label_views=2, surface=True), id="all_five_outputs"),
    pytest.param([(3, 3), (3, 3)], 128, 0, False, {}, id="one_shape"),
    pytest.param([(3, 3), (3, 3)], 100, 0, False, {}, id="width_100"),         # (the bit-packed masks round the width up to 13 bytes)
]


@pytest.mark.parametrize("shapes, width, label_views, log, capacities", ROWS)
def test_a_row_is_exactly_as_large_as_planned(dev, shapes, width, label_views, log, capacities):
    """FrameBatch._row_bytes is the sum over the declarations the rows are allocated from: once every output a row can hold has been asked
    for -- no step, no capture -- every row's cursor stands exactly at the size the arena was planned with, nothing to spare and nothing
    short, and the rows' layouts are equal."""
    import dataclasses
    from vsrd_amd import optimization
    config = _config(True)
    if log:
        config = dataclasses.replace(config, scalar_interval=5, checkpoint_interval=20)
    for first in range(100, 180, 10):          # (a batch needs ONE frame that suits the table sampler to found its rows on)
        frames = [_inputs(dev, first + k, views, n, width=width, label_views=label_views) for k, (views, n) in enumerate(shapes)]
        try:
            batch = optimization.FrameBatch(frames, config, dev, **capacities)
        except optimization.UnsuitableFrameError:
            continue
        break
    else:
        pytest.fail("no frame that suits the table sampler")
    if log:
        batch.log_outputs(metrics=True, masks=True)
    founder = batch.frames[0]
    switches = dict(label_views=batch.max_label_views, headed=founder._headed, photometric=False, surface=batch.surface_rows)
    assert switches["headed"] == bool(capacities) and switches["surface"] == capacities.get("surface", False)
    names = [name for name, output in optimization._OUTPUTS.items() if output.held(switches)]       # (the table and its row switches say what a row holds)
    assert names == ["labels", "masks", "metrics"] + (["group_labels"] if label_views else []) + (["surface"] if switches["surface"] else [])
    for member in batch.frames:
        for name in names:
            member._output_state(name)
    planned = optimization.FrameBatch._row_bytes((founder.view_capacity, 128, width, founder.capacity), batch.config, **switches)
    assert batch.arena.stride == optimization.FrameArena.aligned(planned)
    for row in batch.arena.rows:
        print(f"row {row.index}: cursor {row.cursor}, planned {planned}, {len(row.layout)} buffers")
        assert row.cursor == planned
        assert row.layout == batch.arena.rows[0].layout
    batch.close()


# ---- the kernels under a header, through the C ABI with buffers of the test's own -------------------------------------------------------

def _header(dev, n, views=None, pixels=0, scale=1.0):
    """A vsrd_frame_header on the device: with `views` the full ABI-12 struct, without it an ABI-9 header followed by a tail that must not
    be read (NaN bits: as a view count it would be clamped to the capacity, as a pixel count it is refused -- so a read would show)."""
    from vsrd_amd import _lib
    if views is None:
        header = torch.full((6,), NAN_BITS, dtype=torch.int32)
        header[0] = n
        header.view(torch.float32)[1] = scale
    else:
        struct = _lib.FrameHeader(n | _lib.FRAME_HEADER_HAS_VIEWS, scale, views, 0, pixels)
        header = torch.frombuffer(bytearray(bytes(struct)), dtype=torch.int32).clone()
    return header.to(dev)


def _prologue(dev, scene, step, capacity=None, header=None, sample=None):
    """One prologue launch on buffers of the test's own, everything the kernel reads beyond the scene's own [v, n] and everything it writes
    pre-filled with NaN bits (integers with -7; visibility with 1).  `capacity` = (V_cap, N_cap): the row's layout; `header(dev)` -> the
    header tensor; `sample` = (table tensor, by-value count, rays): the _sample twin."""
    from vsrd_amd import _lib
    lib = _lib.load()
    v, n = scene["visible"].shape
    VC, NC = (v, n) if capacity is None else capacity
    nan = float("nan")
    raw = torch.full((NC, 8), nan)
    raw[:n] = scene["raw"].float()
    E, K, gt = torch.full((VC, 16), nan), torch.full((VC, 9), nan), torch.full((VC, NC, 4), nan)
    E[:v], K[:v], gt[:v, :n] = scene["E"].float().reshape(v, 16), scene["K"].float().reshape(v, 9), scene["gt_boxes"].float()
    visible = torch.ones(VC, NC, dtype=torch.uint8)
    visible[:v, :n] = scene["visible"].to(torch.uint8)
    t = dict(loc=raw[:, 0:3].contiguous().to(dev), dim=raw[:, 3:6].contiguous().to(dev), ori=raw[:, 6:8].contiguous().to(dev), E=E.to(dev), K=K.to(dev),
             gt=gt.to(dev), visible=visible.to(dev), step=torch.tensor([step], dtype=torch.int64, device=dev))
    scratch_bytes = lib.vsrd_frame_scratch_bytes(VC, NC)
    assert scratch_bytes == VC * NC * 36 * 4                                       # (sized by the capacities)
    out = dict(scratch=torch.full((scratch_bytes // 4 + glue.GUARD,), nan, device=dev), instances=torch.full((NC, 16), nan, device=dev),
               pd_indices=torch.full((NC,), -7, dtype=torch.int64, device=dev), gt_indices=torch.full((NC,), -7, dtype=torch.int64, device=dev),
               target_columns=torch.full((NC,), -7, dtype=torch.int32, device=dev), instance_weights=torch.full((NC,), nan, device=dev),
               schedule=torch.full((3,), nan, device=dev), losses=torch.full((2,), nan, device=dev), grad_raw=torch.full((NC, 8), nan, device=dev))
    args = [glue._frame_config(VC, NC), _lib.ptr(t["loc"]), _lib.ptr(t["dim"]), _lib.ptr(t["ori"]), _lib.ptr(t["E"]), _lib.ptr(t["K"]), _lib.ptr(t["gt"]),
            t["visible"].data_ptr(), t["step"].data_ptr(), out["scratch"].data_ptr(), scratch_bytes, _lib.ptr(out["instances"]),
            out["pd_indices"].data_ptr(), out["gt_indices"].data_ptr(), out["target_columns"].data_ptr(), _lib.ptr(out["instance_weights"]),
            _lib.ptr(out["schedule"]), _lib.ptr(out["losses"]), _lib.ptr(out["grad_raw"])]
    name = "vsrd_frame_prologue"
    if sample is not None:
        table, count, rays = sample
        out["rays"] = torch.full((rays,), -7, dtype=torch.int64, device=dev)
        args += [table.data_ptr(), count, rays, 5, None, out["rays"].data_ptr()]
        name += "_sample"
    if header is not None:
        keep = header(dev)
        args.append(keep.data_ptr())
        name += "_with_header"
    _lib.check(getattr(lib, name)(*args, _lib.stream()))
    torch.cuda.synchronize()
    return {key: value.cpu() for key, value in out.items()}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_prologue(twin, alone, v, n, capacity):
    VC, NC = capacity
    for name in ("instances", "pd_indices", "gt_indices", "target_columns", "instance_weights", "grad_raw"):
        assert torch.equal(_bits(twin[name][:n]), _bits(alone[name])), name
        fill = twin[name][n:]
        assert bool((fill == -7).all()) if fill.dtype in (torch.int32, torch.int64) else glue._is_fill(fill), name
    for name in ("schedule", "losses"):
        assert torch.equal(_bits(twin[name]), _bits(alone[name])), name
    # the scratch: the frame's own v n pairs at the offsets of a [v, n] launch (above 256 pairs), nothing on the LDS path, nothing behind
    used = v * n * 36 if v * n > 256 else 0
    assert torch.equal(_bits(twin["scratch"][:used]), _bits(alone["scratch"][:used]))
    assert glue._is_fill(twin["scratch"][used:]) and glue._is_fill(alone["scratch"][used:])
    assert twin["scratch"].numel() == VC * NC * 36 + glue.GUARD


@pytest.mark.parametrize("v,n", [(5, 50), (5, 52), (1, 1), (32, 64)], ids=["250_pairs", "260_pairs", "1x1", "32x64"])
def test_prologue_twin_across_the_lds_scratch_switch(dev, v, n):
    """3: a row of capacity 32 views x 64 boxes whose header says (v, n) gives every output of vsrd_frame_prologue on contiguous [v, n]
    arrays, on either side of the 256-pair switch between LDS and the global scratch -- which follows the frame's own v n."""
    scene = scenes.build(v, n, scenes.SHAPES.get((v, n), 1))
    alone = _prologue(dev, scene, 7)
    twin = _prologue(dev, scene, 7, capacity=(32, 64), header=lambda d: _header(d, n, views=v))
    _same_prologue(twin, alone, v, n, (32, 64))


def test_sampler_takes_the_frames_own_pixel_count(dev):
    """4: the table of a 2-view frame inside an allocation sized for 4 views (their guides differ in size: 13 and 14 bits); the sampler half
    of vsrd_frame_prologue_sample_with_header with num_pixels = v_f H W draws what vsrd_sample_rays_table draws from that table alone."""
    from vsrd_amd import _lib
    lib = _lib.load()
    pixels, views, capacity, rays = 64 * 64, 2, 4, 96
    count, count_capacity = views * pixels, capacity * pixels
    weights = (torch.rand(count, generator=torch.Generator().manual_seed(2)) + 0.05).to(dev)
    nbytes = lib.vsrd_ray_table_bytes(count_capacity)
    assert nbytes > lib.vsrd_ray_table_bytes(count)
    table = torch.full((nbytes // 4,), NAN_BITS, dtype=torch.int32, device=dev)
    _lib.check(lib.vsrd_ray_table_build(_lib.ptr(weights), count, table.data_ptr(), nbytes, _lib.stream()))
    torch.cuda.synchronize()
    own = lib.vsrd_ray_table_bytes(count)
    assert bool((table[own // 4:] == NAN_BITS).all())                              # (the build wrote the frame's own table, nothing behind it)
    scene = scenes.build(views, 3, 4)
    for step in (0, 7, 1234):
        expected = torch.full((rays,), -7, dtype=torch.int64, device=dev)
        counter = torch.tensor([step], dtype=torch.int64, device=dev)
        _lib.check(lib.vsrd_sample_rays_table(table.data_ptr(), count, rays, 5, 0, counter.data_ptr(), None, expected.data_ptr(), _lib.stream()))
        torch.cuda.synchronize()
        twin = _prologue(dev, scene, step, capacity=(capacity, 6), header=lambda d: _header(d, 3, views=views, pixels=count),
                         sample=(table, count_capacity, rays))
        assert torch.equal(twin["rays"], expected.cpu()), step
        assert bool(((twin["rays"] >= 0) & (twin["rays"] < count)).all())
        assert len(set(twin["rays"].tolist())) == rays


class _Arena(labels_test.Arena):
    """tests/test_hip_frame_labels.py's arena with the full vsrd_frame_header (24 bytes) in its header slot."""

    def __init__(self, V, N, B=1):
        super().__init__(V, N, B)
        offset, _, _, dtype = self.layout["header"]
        self.layout["header"] = (offset, 24, (6,), dtype)                         # (the slot is 256 bytes: the struct fits)

    def put_prefix(self, f, scene):
        from vsrd_amd import _lib
        v, n = scene["visible"].shape
        raw = scene["raw"].float()
        self.view("loc", f)[:n], self.view("dim", f)[:n], self.view("ori", f)[:n] = raw[:, 0:3], raw[:, 3:6], raw[:, 6:8]
        self.view("E", f)[:v] = scene["E"].float().reshape(v, 16)
        self.view("K", f)[:v] = scene["K"].float().reshape(v, 9)
        self.view("gt", f)[:v, :n] = scene["gt_boxes"].float()
        self.view("visible", f)[:v, :n] = scene["visible"].to(torch.uint8)
        struct = _lib.FrameHeader(n | _lib.FRAME_HEADER_HAS_VIEWS, 1.0, v, 0, 0)
        self.view("header", f).copy_(torch.frombuffer(bytearray(bytes(struct)), dtype=torch.int32))


def test_labels_under_a_header_of_views_and_instances(dev):
    """5: vsrd_frame_labels with a header (v_f = 2, n_f = 3) on a row of capacity (4, 6) writes the bits of the call on contiguous [2, 3]
    arrays and nothing else -- and that contiguous result is within the label tolerances of tests/test_hip_frame_labels.py."""
    v, n = 2, 3
    scene = scenes.build(v, n, 6)
    alone = labels_test._alone(dev, scene)
    labels_test._check("test_labels_under_a_header_of_views_and_instances", scene, alone)
    arena = _Arena(4, 6)
    arena.put_prefix(0, scene)
    expected = arena.host.clone()
    for name in ("camera_corners", "boxes_2d"):
        arena.view(name, 0, expected)[:v, :n] = alone[name]
    arena.view("mean_iou", 0, expected)[:n, :n] = alone["mean_iou"]
    for name in ("matched_gt", "confidences"):
        arena.view(name, 0, expected)[:n] = alone[name]
    _, after = labels_test._call(dev, arena)
    assert not torch.equal(after, arena.host)
    assert torch.equal(after, expected)                           # bytes: the frame's bits, the fill everywhere else (views 2, 3 included)


def test_ingest_into_a_row_of_more_views(dev):
    """6: a 2-view pack ingested into a row laid out for 4 views equals the ingest into a 2-view row on the first 2 H W rows -- soft masks,
    weights, boxes, visibility -- and leaves the rest untouched."""
    import make_frame_packs
    from vsrd_amd import frames
    pack = make_frame_packs.make_pack(8, 2, 24, 40, 3, drop=[(1, 0)], shuffle=True)
    H, W = pack.image_size
    pixels, capacity, views = 2 * H * W, 4, 4
    def buffers(v):
        return (torch.full((v * H * W, capacity), -7.0, device=dev), torch.full((v * H * W,), -7.0, device=dev), torch.full((v, capacity, 4), -7.0, device=dev),
                torch.full((v, capacity), 9, dtype=torch.uint8, device=dev))
    small, large = buffers(2), buffers(views)
    frames.ingest_into(pack, dev, capacity, *small)
    frames.ingest_into(pack, dev, capacity, large[0][:pixels], large[1][:pixels], large[2][:2], large[3][:2])
    torch.cuda.synchronize()
    assert bool((small[0][:, :3] != -7.0).all()) and bool((small[1] != -7.0).all())
    for a, b, rows in zip(small, large, (pixels, pixels, 2, 2)):
        assert torch.equal(_bits(b[:rows]), _bits(a))
        assert bool((b[rows:] == (9 if b.dtype == torch.uint8 else -7.0)).all())


def test_an_abi_9_header_still_means_what_it_meant(dev):
    """8: a header without the views bit -- 8 bytes, whatever lies behind them -- on a batch of two frames of one V reproduces the headerless
    batched call bit for bit: the prologue with its sampler half, and the label kernel."""
    from vsrd_amd import _lib
    lib = _lib.load()
    V, N, rays, pixels = 3, 5, 64, 4096
    stride = 1 << 20
    frames_ = [scenes.build(V, N, 10 + f) for f in range(2)]
    weights = [(torch.rand(pixels, generator=torch.Generator().manual_seed(20 + f)) + 0.05).to(dev) for f in range(2)]
    table_bytes = lib.vsrd_ray_table_bytes(pixels)
    # one arena of two rows, `stride` bytes apart: every buffer of a row at the same offset
    fields = [("loc", (N, 3), torch.float32), ("dim", (N, 3), torch.float32), ("ori", (N, 2), torch.float32), ("E", (V, 16), torch.float32),
              ("K", (V, 9), torch.float32), ("gt", (V, N, 4), torch.float32), ("visible", (V, N), torch.uint8), ("step", (1,), torch.int64),
              ("header", (6,), torch.int32), ("table", (table_bytes,), torch.uint8), ("scratch", (V * N * 36,), torch.float32),
              ("instances", (N, 16), torch.float32), ("pd_indices", (N,), torch.int64), ("gt_indices", (N,), torch.int64),
              ("target_columns", (N,), torch.int32), ("instance_weights", (N,), torch.float32), ("schedule", (3,), torch.float32),
              ("losses", (2,), torch.float32), ("grad_raw", (N, 8), torch.float32), ("rays", (rays,), torch.int64),
              ("camera_corners", (V, N, 8, 3), torch.float32), ("boxes_2d", (V, N, 4), torch.float32), ("mean_iou", (N, N), torch.float32),
              ("matched_gt", (N,), torch.int64), ("confidences", (N,), torch.float32)]
    layout, cursor = {}, 0
    for name, shape, dtype in fields:
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        layout[name] = (cursor, nbytes, shape, dtype)
        cursor = (cursor + nbytes + 255) // 256 * 256
    assert cursor <= stride

    def run(with_header):
        arena = torch.zeros(2 * stride, dtype=torch.uint8, device=dev)
        view = lambda name, f: arena[f * stride + layout[name][0]:f * stride + layout[name][0] + layout[name][1]].view(layout[name][3]).view(layout[name][2])
        for f, scene in enumerate(frames_):
            raw = scene["raw"].float().to(dev)
            view("loc", f).copy_(raw[:, 0:3]); view("dim", f).copy_(raw[:, 3:6]); view("ori", f).copy_(raw[:, 6:8])
            view("E", f).copy_(scene["E"].float().reshape(V, 16)); view("K", f).copy_(scene["K"].float().reshape(V, 9))
            view("gt", f).copy_(scene["gt_boxes"].float()); view("visible", f).copy_(scene["visible"].to(torch.uint8))
            view("step", f).fill_(3 + f)
            view("header", f).copy_(_header(dev, N))
            _lib.check(lib.vsrd_ray_table_build(_lib.ptr(weights[f]), pixels, view("table", f).data_ptr(), table_bytes, _lib.stream()))
        pointer = lambda name: arena.data_ptr() + layout[name][0]
        frame = glue._frame_config(V, N)
        frame.num_frames, frame.frame_stride = 2, stride
        args = [frame, *[pointer(name) for name in ("loc", "dim", "ori", "E", "K", "gt", "visible", "step", "scratch")], V * N * 36 * 4,
                *[pointer(name) for name in ("instances", "pd_indices", "gt_indices", "target_columns", "instance_weights", "schedule", "losses", "grad_raw")],
                pointer("table"), pixels, rays, 5, None, pointer("rays")]
        label_args = [frame, *[pointer(name) for name in ("loc", "dim", "ori", "E", "K", "gt", "visible", "camera_corners", "boxes_2d", "mean_iou",
                                                          "matched_gt", "confidences")]]
        if with_header:
            _lib.check(lib.vsrd_frame_prologue_sample_with_header(*args, pointer("header"), _lib.stream()))
            _lib.check(lib.vsrd_frame_labels(*label_args, pointer("header"), _lib.stream()))
        else:
            _lib.check(lib.vsrd_frame_prologue_sample(*args, _lib.stream()))
            _lib.check(lib.vsrd_frame_labels(*label_args, None, _lib.stream()))
        torch.cuda.synchronize()
        return arena.cpu()

    plain, twin = run(False), run(True)
    assert torch.equal(plain, twin)
    rays_drawn = plain[layout["rays"][0]:layout["rays"][0] + layout["rays"][1]].view(torch.int64)
    assert bool(((rays_drawn >= 0) & (rays_drawn < pixels)).all())
    assert ctypes.sizeof(_lib.FrameHeader) == 24
