"""vsrd_frame_log (csrc/frame_log.h): the scalar history and the step snapshots of the graph loop, gathered on the device between replays.

The call is pure gather and copy, so every comparison here is bit equality (floats are compared as the int32 they are: a NaN equals itself).

(a) the kernel alone through the C ABI, on hand-made buffers in a RowArena whose every word starts as a sentinel: what is written equals its
    source, and every other byte of the arena still holds what it held.  The issue's case has counters 6, 7 and 40 and says the third
    frame "counts two drops"; 40 is a multiple of the checkpoint interval 2 but not of the scalar interval 3, so that frame counts ONE drop.
    The test keeps 40 (one drop) and adds a fourth frame at 42, which sits on both boundaries beyond both capacities: two drops.
(b) one FrameOptimizer(graph=True) with the log against a twin without it that is stepped one step at a time and read on the host.
(c) a FrameBatch of three frames (2, 3, 2 instances in rows of 3) whose row 1 is reset after four steps, against each frame alone.  The phase
    of a replayed graph is the batch's, not a row's, so a row whose counter lags can only match its own lone run inside one phase: (c) stays
    in the box-only phase (warmup_steps = num_steps); (b) and (d) cross into the residual phase.
(d) a frame with 3-D ground truth, metrics and masks on, at intervals (4 / 8) between which run() replays its four-step graphs.

Shapes: V = 2, 16 x 24 pixels, 64 rays.  At that image size the synthetic frames' boxes cover about twenty pixels, fewer than a draw of 64
rays needs, so the soft masks are uniform random numbers (every pixel can be drawn); the log does not care what is optimised.  S = 33
samples per ray, the smallest the step accepts in every loop here: a batch of frames runs the box-only step in its split-ray form only,
which exists for two and four rounds of 64 merged samples, 2 S - 1 >= 65 (csrc/api.hip, vsrd_render_silhouette_step_with_header)."""
import dataclasses

import numpy as np
import pytest
import torch

from frame_rows import RowArena

pytestmark = pytest.mark.gpu

SENTINEL_BITS = int(np.array(-777.0, dtype=np.float32).view(np.int32))
GAP = 256
SIZE = (16, 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def bits(tensor):
    tensor = tensor.detach().cpu().contiguous()
    return tensor.view(torch.int32) if tensor.dtype == torch.float32 else tensor


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# ---- (a) the kernel alone ---------------------------------------------------------------------------------------------------------------
SEGMENTS = (1, 2, 3, 5, 1617, 70001)           # floats; the 1617 one is read from a source 4 bytes off 16-byte alignment
RESERVED = tuple((count + 3) // 4 * 4 for count in SEGMENTS)
SLOT = sum(RESERVED)
ROWS, SLOTS = 4, 3
COUNTERS = (6, 7, 40, 42)


def _arena():
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    fields = [("step", (1,), i64), ("record", (5,), f32), *[(f"rate{g}", (1,), f32) for g in range(5)], ("rates", (5,), i64), ("schedule", (3,), f32),
              ("summary", (8,), f32), ("table", (32 * 24,), torch.uint8), *[(f"source{k}", (count + 4,), f32) for k, count in enumerate(SEGMENTS)],
              ("history", (ROWS, 22), f32), ("snapshots", (SLOTS, SLOT), f32), ("snapshot_steps", (SLOTS,), i32), ("counters", (4,), i32)]
    return RowArena(fields, len(COUNTERS), SENTINEL_BITS, GAP)


def _source(arena, k, f, host=None):
    """Segment k's source of frame f: the holder's words 0.. (aligned), or 1.. for the 1617-float segment (4 bytes off)."""
    start = 1 if SEGMENTS[k] == 1617 else 0
    return arena.view(f"source{k}", f, host)[start:start + SEGMENTS[k]]


def _filled(arena, base):
    """The arena's host image with every input written (random bit patterns, NaNs among them) and the counters zeroed; `base`: the device
    address the image will have (the pointer list and the table hold absolute addresses of the frame's own buffers)."""
    from vsrd_amd import _lib
    generator = torch.Generator().manual_seed(5)
    for f, counter in enumerate(COUNTERS):
        arena.view("step", f)[0] = counter
        for name in ("record", "schedule", "summary", *[f"rate{g}" for g in range(5)]):
            arena.view(name, f).view(torch.int32).copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, arena.view(name, f).shape, generator=generator, dtype=torch.int64).to(torch.int32))
        row = base + f * arena.stride
        arena.view("rates", f).copy_(torch.tensor([row + arena.layout[f"rate{g}"][0] for g in range(5)], dtype=torch.int64))
        table, offset = (_lib.LogSegment * 32)(), 0
        for k, count in enumerate(SEGMENTS):
            _source(arena, k, f).view(torch.int32).copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (count,), generator=generator, dtype=torch.int64).to(torch.int32))
            address = row + arena.layout[f"source{k}"][0] + (4 if count == 1617 else 0)
            assert (address % 16 == 4) == (count == 1617)
            table[k] = _lib.LogSegment(address, count, offset)
            offset += RESERVED[k]
        arena.view("table", f).copy_(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))
        arena.view("counters", f).zero_()


def _call(arena, device_image, scalar_interval, checkpoint_interval, with_summary=True):
    from vsrd_amd import _lib
    at = arena.pointers(device_image)
    config = _lib.FrameLogConfig(scalar_interval, checkpoint_interval, ROWS, SLOTS, SLOT, len(SEGMENTS), arena.B, arena.stride, at("step"), at("record"),
                                 at("rates"), at("schedule"), at("summary") if with_summary else None, at("table"), at("history"), at("snapshots"),
                                 at("snapshot_steps"), at("counters"))
    _lib.check(_lib.load().vsrd_frame_log(config, _lib.stream()))
    torch.cuda.synchronize()
    return device_image.cpu()


def _expected(arena, image, scalar_interval, checkpoint_interval, with_summary=True):
    """What the call leaves of `image` (a host copy taken before the call), written the slow way."""
    expected = image.clone()
    for f, c in enumerate(COUNTERS):
        counters = arena.view("counters", f, expected)
        if scalar_interval and c % scalar_interval == 0:
            row = c // scalar_interval - 1
            if row < ROWS:
                target = arena.view("history", f, expected)[row].view(torch.int32)
                target[0] = c - 1
                target[1:6] = arena.view("record", f, image).view(torch.int32)
                for g in range(5):
                    target[6 + g] = arena.view(f"rate{g}", f, image).view(torch.int32)[0]
                target[11:14] = arena.view("schedule", f, image).view(torch.int32)
                target[14:22] = arena.view("summary", f, image).view(torch.int32) if with_summary else 0x7fc00000
                counters[0] = max(int(counters[0]), row + 1)
            else:
                counters[1] += 1
        if checkpoint_interval and c % checkpoint_interval == 0:
            slot = c // checkpoint_interval - 1
            if slot < SLOTS:
                words, offset = arena.view("snapshots", f, expected)[slot], 0
                for k, count in enumerate(SEGMENTS):
                    words[offset:offset + count].view(torch.int32).copy_(_source(arena, k, f, image).view(torch.int32))
                    offset += RESERVED[k]
                arena.view("snapshot_steps", f, expected)[slot] = c - 1
                counters[2] = max(int(counters[2]), slot + 1)
            else:
                counters[3] += 1
    return expected


@pytest.mark.parametrize("scalar_interval,checkpoint_interval,with_summary", [(3, 2, True), (3, 2, False), (0, 2, True), (3, 0, True)])
def test_kernel_alone(dev, scalar_interval, checkpoint_interval, with_summary):
    arena = _arena()
    device_image = torch.empty_like(arena.host, device=dev)
    assert device_image.data_ptr() % 256 == 0
    _filled(arena, device_image.data_ptr())
    device_image.copy_(arena.host)
    before = arena.host.clone()
    after = _call(arena, device_image, scalar_interval, checkpoint_interval, with_summary)
    expected = _expected(arena, before, scalar_interval, checkpoint_interval, with_summary)
    assert torch.equal(after, expected)                      # every byte of the arena: what was written, and the sentinel everywhere else
    # ... and spelled out: frame 0 logs both, frame 1 nothing, frame 2 (40) drops its snapshot, frame 3 (42) drops both
    counters = [arena.view("counters", f, after).tolist() for f in range(len(COUNTERS))]
    logs, snaps = int(scalar_interval > 0), int(checkpoint_interval > 0)
    assert counters == [[2 * logs, 0, 3 * snaps, 0], [0, 0, 0, 0], [0, 0, 0, snaps], [0, logs, 0, snaps]]
    assert arena.view("snapshot_steps", 0, after).tolist() == [SENTINEL_BITS, SENTINEL_BITS, 5 if snaps else SENTINEL_BITS]
    for f in (1, 2, 3):
        for name in ("history", "snapshots", "snapshot_steps"):
            assert torch.equal(arena.view(name, f, after), arena.view(name, f, before)), (f, name)
    if logs:
        assert int(arena.view("history", 0, after)[1].view(torch.int32)[0]) == 5
        assert (arena.view("history", 0, after)[[0, 2, 3]].view(torch.int32) == SENTINEL_BITS).all()
    if snaps:
        assert same(arena.view("snapshots", 0, after)[2][SLOT - RESERVED[-1]:SLOT - RESERVED[-1] + 70001], _source(arena, 5, 0, before))
        assert (arena.view("snapshots", 0, after)[:2].view(torch.int32) == SENTINEL_BITS).all()
    # a second call at the same counters writes the same bytes again and counts the drops again
    again = _call(arena, device_image, scalar_interval, checkpoint_interval, with_summary)
    assert torch.equal(again, _expected(arena, after, scalar_interval, checkpoint_interval, with_summary))


def test_kernel_refuses_what_it_cannot_serve(dev):
    from vsrd_amd import _lib
    P = 0x1000

    def config(**changes):
        values = dict(scalar_interval=3, checkpoint_interval=2, history_capacity=4, snapshot_capacity=3, snapshot_floats=64, num_segments=2, num_frames=1,
                      frame_stride=0, step=P, record=P, learning_rates=P, schedule=P, summary=None, segments=P, history=P, snapshots=P, snapshot_steps=P, counters=P)
        values.update(changes)
        return _lib.FrameLogConfig(**values)
    lib = _lib.load()
    for changes in (dict(scalar_interval=-1), dict(checkpoint_interval=-1), dict(history_capacity=-1), dict(step=None), dict(counters=None), dict(record=None),
                    dict(learning_rates=None), dict(history=None), dict(segments=None), dict(snapshots=None), dict(snapshot_steps=None), dict(num_segments=33),
                    dict(snapshot_floats=62), dict(snapshots=P + 4), dict(num_frames=2, frame_stride=100)):
        assert lib.vsrd_frame_log(config(**changes), None) == _lib.E_INVALID_ARGUMENT, changes
    assert lib.vsrd_frame_log(None, None) == _lib.E_INVALID_ARGUMENT
    assert lib.vsrd_frame_log(config(scalar_interval=0, checkpoint_interval=0), None) == 0           # both off: no launch (the pointers are dummies)


# ---- (b) - (d) the loops ------------------------------------------------------------------------------------------------------------------
def _inputs(dev, frame, n, views=2):
    """A frame of `n` instances at SIZE: the synthetic frame's cameras and boxes (its 2-D and 3-D ground truth), uniform random soft masks."""
    from vsrd_amd import models, operations, optimization, synthetic
    height, width = SIZE
    K, E, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(int(frame), views, height, width, n)
    K, E = K.to(dev), E.to(dev)
    det = models.BoxParameters3D(1, n).to(dev)
    with torch.no_grad():
        det.locations.copy_(raw_loc); det.dimensions.copy_(raw_dim); det.orientations.copy_(raw_ori)
        out = det()
        gt_boxes, _ = operations.project_boxes_multi_view(out["boxes_3d"][0], E, K, (height, width))
    soft = (torch.rand(views, height, width, n, generator=torch.Generator().manual_seed(100 + int(frame))) * 0.9 + 0.05).to(dev)
    return optimization.FrameInputs((height, width), K, E, soft, gt_boxes, torch.ones(views, n, dtype=torch.bool, device=dev), boxes_3d=out["boxes_3d"][0].contiguous())


def _config(**more):
    from vsrd_amd import optimization
    values = dict(num_samples=33, num_rays=64, warmup_steps=6, num_steps=12, seed=3, mlp_adjoint_item_slots=8, surface_num_iterations=32)
    values.update(more)
    return optimization.OptimizationConfig(**values)


def _state(loop):
    return {module: {key: value.detach().clone() for key, value in getattr(loop, module).state_dict().items()} for module in ("detector", "hyper_distance_field")}


def _adam(loop):
    return [state[key].detach().clone() for params in loop._module_parameters() for p in params for state in [loop.optimizer.state[p]]
            for key in ("exp_avg", "exp_avg_sq", "step")]


def _twin(dev, inputs, config, steps, scalar_interval, checkpoint_interval, metrics=False, masks=False):
    """The frame alone, without the log, one step() at a time; read on the host at the boundaries: (rows, snapshots, the loop)."""
    from vsrd_amd import optimization
    loop = optimization.FrameOptimizer(inputs, dataclasses.replace(config, scalar_interval=0, checkpoint_interval=0), dev, graph=True, persistent=True)
    rows, snapshots = [], []
    for step in range(steps):
        loop.step()
        count = step + 1
        summary = loop.metrics()["summary"].clone() if metrics and (count % scalar_interval == 0 or count % checkpoint_interval == 0) else None
        if count % scalar_interval == 0:
            rows.append(dict(step=step, record=loop._glue["record"].clone(), rates=torch.stack([group["lr"].clone() for group in loop.optimizer.param_groups]),
                             schedule=loop.schedule.clone(), summary=summary))
        if count % checkpoint_interval == 0:
            snapshots.append(dict(step=step, models=_state(loop), summary=summary, mask_iou=loop.masks()["mask_iou"].clone() if masks else None))
    torch.cuda.synchronize()
    return rows, snapshots, loop


def _check_against_twin(history, snapshots, rows, twin_snapshots, warmup_steps, metrics=False, masks=False):
    assert history["steps"].tolist() == [row["step"] for row in rows] and history["steps"].dtype == torch.int32
    names = ("iou_projection_loss", "l1_projection_loss", "silhouette_loss", "eikonal_loss", "loss")
    for j, row in enumerate(rows):
        for column, name in enumerate(names):
            if name == "eikonal_loss" and row["step"] < warmup_steps:
                assert bool(torch.isnan(history[name][j]))
            else:
                assert same(history[name][j], row["record"][column]), (j, name)
        assert same(history["learning_rates"][j], row["rates"]) and same(history["hyperparameters"][j], row["schedule"]), j
        if metrics:
            assert same(history["metrics"][j], row["summary"]), j
        else:
            assert bool(torch.isnan(history["metrics"][j]).all())
    assert [int(s["step"]) for s in snapshots] == [s["step"] for s in twin_snapshots]
    for mine, other in zip(snapshots, twin_snapshots):
        assert set(mine) == {"step", "models", "metrics"} and set(mine["models"]) == {"detector", "hyper_distance_field"}
        for module, state in other["models"].items():
            assert list(mine["models"][module]) and set(mine["models"][module]) == set(state)
            for key, value in state.items():
                assert same(mine["models"][module][key], value), (other["step"], module, key)
        assert set(mine["metrics"]) == ({"summary"} if metrics else set()) | ({"mask_iou"} if masks else set())
        if metrics:
            assert same(mine["metrics"]["summary"], other["summary"])
        if masks:
            assert same(mine["metrics"]["mask_iou"], other["mask_iou"])


def test_one_frame_against_a_twin_without_the_log(dev):
    from vsrd_amd import optimization
    inputs, config = _inputs(dev, 3, 2), _config(init_seed=70, scalar_interval=3, checkpoint_interval=4)
    rows, twin_snapshots, twin = _twin(dev, inputs, config, 12, 3, 4)
    loop = optimization.FrameOptimizer(inputs, config, dev, graph=True, persistent=True)
    loop.run(12, steps_per_graph=4)
    torch.cuda.synchronize()
    history, snapshots = loop.history(), loop.snapshots()
    assert [row["step"] for row in rows] == [2, 5, 8, 11] and [s["step"] for s in twin_snapshots] == [3, 7, 11]
    _check_against_twin(history, snapshots, rows, twin_snapshots, config.warmup_steps)
    assert torch.isnan(history["eikonal_loss"]).tolist() == [True, True, False, False]                 # (the run crosses the warm-up boundary)
    assert loop._log["counters"].tolist() == [4, 0, 3, 0]
    # logging changes nothing: the final parameters and Adam's state of the two loops
    for module, state in _state(twin).items():
        for key, value in state.items():
            assert same(_state(loop)[module][key], value), (module, key)
    assert all(same(a, b) for a, b in zip(_adam(loop), _adam(twin)))
    # reset() starts the log over; a loop that runs beyond its capacities drops, counts and says so when it is closed
    assert loop.reset(inputs, init_seed=70)
    assert loop._log["counters"].tolist() == [0, 0, 0, 0] and loop.history()["steps"].numel() == 0 and loop.snapshots() == []
    loop.run(12)
    loop.run(4)            # (steps 12 .. 15: one row and one slot beyond the capacities 12 // 3 and 12 // 4)
    torch.cuda.synchronize()
    assert loop._log["counters"].tolist() == [4, 1, 3, 1] and loop.history()["steps"].tolist() == [2, 5, 8, 11]
    with pytest.warns(RuntimeWarning, match="dropped 1 history rows and 1 snapshots"):
        loop.close()
    twin.close()
    # off by default: no buffer, no launch
    assert twin._log is None
    with pytest.raises(RuntimeError):
        twin.history()


def test_frame_batch_rows_log_by_their_own_counters(dev):
    from vsrd_amd import optimization
    counts = (2, 3, 2)
    inputs = [_inputs(dev, 3 + f, n) for f, n in enumerate(counts)]
    config = _config(warmup_steps=12, scalar_interval=3, checkpoint_interval=4)
    batch = optimization.FrameBatch(inputs, config, dev, init_seeds=[70, 71, 72], max_instances=3)
    batch.capture_all()
    for f in range(3):
        assert batch.reset(f, inputs[f], init_seed=70 + f)
    batch.run(4)
    assert batch.reset(1, inputs[1], init_seed=71)           # row 1 starts over: its counter lags by four
    batch.run(8)
    torch.cuda.synchronize()
    assert [m.step_index for m in batch.frames] == [12, 8, 12]
    histories, snapshots = batch.history(), batch.snapshots()
    for f, n in enumerate(counts):
        steps = batch.frames[f].step_index
        rows, twin_snapshots, twin = _twin(dev, inputs[f], dataclasses.replace(config, init_seed=70 + f), steps, 3, 4)
        twin.close()
        assert len(rows) == steps // 3 and len(twin_snapshots) == steps // 4
        _check_against_twin(histories[f], snapshots[f], rows, twin_snapshots, config.warmup_steps)
        member = batch.frames[f]
        assert member._log["counters"].tolist() == [steps // 3, 0, steps // 4, 0]
        # nothing beyond the frame's own n instances: the views have n, and the rest of what the slot reserves for the capacity was never written
        layout = {name: (offset, source) for name, offset, source in member._log["layout"]}
        for name, per_instance in (("detector.locations", 3), ("detector.dimensions", 3), ("detector.orientations", 2), ("detector.embeddings", 256)):
            offset, (shape, _) = layout[name]
            assert shape == (1, n, per_instance)
            for slot in range(steps // 4):
                assert tuple(snapshots[f][slot]["models"]["detector"][name.split(".")[1]].shape) == (1, n, per_instance)
                reserved = member._log["snapshots"][slot][offset + n * per_instance:offset + (3 * per_instance + 3) // 4 * 4]
                assert not bool(reserved.any())
    batch.close()


def test_metrics_and_masks_ride_in_the_log(dev):
    """Intervals 4 and 8 over 16 steps with the warm-up boundary at 8: run() replays the four-step graphs of both phases between the log's
    launches (steps 4 .. 7 and 12 .. 15)."""
    from vsrd_amd import optimization
    inputs, config = _inputs(dev, 5, 2), _config(init_seed=73, num_steps=16, warmup_steps=8, scalar_interval=4, checkpoint_interval=8)
    rows, twin_snapshots, twin = _twin(dev, inputs, config, 16, 4, 8, metrics=True, masks=True)
    loop = optimization.FrameOptimizer(inputs, config, dev, graph=True, persistent=True)
    loop.log_outputs(metrics=True, masks=True)
    loop.run(16, steps_per_graph=4)
    torch.cuda.synchronize()
    assert (False, False, 4) in loop._graphs and (True, False, 4) in loop._graphs
    assert [row["step"] for row in rows] == [3, 7, 11, 15] and [s["step"] for s in twin_snapshots] == [7, 15]
    _check_against_twin(loop.history(), loop.snapshots(), rows, twin_snapshots, config.warmup_steps, metrics=True, masks=True)
    assert float(rows[0]["summary"][0]) == 2.0               # (both pairs have ground truth: the summaries compared are real ones)
    for module, state in _state(twin).items():
        for key, value in state.items():
            assert same(_state(loop)[module][key], value), (module, key)
    loop.close()
    twin.close()


def test_a_frame_without_ground_truth_names_no_metrics(dev):
    """A slot (and a batch row) that served a frame WITH boxes_3d -- its founder, through capture_all(), and a whole run -- and is reset to a
    frame WITHOUT: every history row and snapshot of the second frame holds the summary of no pair (eight zeros, count 0), which names no
    metric in history.json or a step_*.pt -- never what the earlier frame left in the row's summary buffer."""
    from vsrd_amd import formats, optimization
    first, bare = _inputs(dev, 5, 2), dataclasses.replace(_inputs(dev, 6, 2), boxes_3d=None)
    config = _config(warmup_steps=12, scalar_interval=3, checkpoint_interval=4)

    def names_nothing(history, snapshots):
        assert history["steps"].tolist() == [2, 5, 8, 11] and len(snapshots) == 3
        assert not bool(history["metrics"].any()) and all(not bool(s["metrics"]["summary"].any()) for s in snapshots)
        assert not any(key.startswith("metrics/") for record in formats.frame_history_records(history) for key in record)
        assert [payload["metrics"] for payload in formats.snapshot_payloads(snapshots)] == [{}, {}, {}]

    def names_its_own(history, snapshots):
        assert history["metrics"][:, 0].tolist() == [2.0] * 4 and all(float(s["metrics"]["summary"][0]) == 2.0 for s in snapshots)
        assert all("metrics/iou_3d" in record for record in formats.frame_history_records(history))
        assert all("iou_3d" in payload["metrics"] for payload in formats.snapshot_payloads(snapshots))
    loop = optimization.FrameOptimizer(first, dataclasses.replace(config, init_seed=74), dev, graph=True, persistent=True)
    loop.log_outputs(metrics=True)
    loop.capture_all()
    assert loop.reset(first, init_seed=74)
    loop.run(12)
    torch.cuda.synchronize()
    names_its_own(loop.history(), loop.snapshots())
    assert loop.reset(bare, init_seed=75)
    loop.run(12)
    torch.cuda.synchronize()
    names_nothing(loop.history(), loop.snapshots())
    loop.close()
    # a batch of the two: the rows swap frames, so the row founded on the frame with ground truth serves the one without
    batch = optimization.FrameBatch([first, bare], config, dev, init_seeds=[74, 75])
    batch.log_outputs(metrics=True)
    batch.capture_all()
    assert batch.reset(0, bare, init_seed=75) and batch.reset(1, first, init_seed=74)
    batch.run(12)
    torch.cuda.synchronize()
    histories, snapshots = batch.history(), batch.snapshots()
    names_nothing(histories[0], snapshots[0])
    names_its_own(histories[1], snapshots[1])
    batch.close()
