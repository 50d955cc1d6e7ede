"""Mixed frame batches (include/vsrd_hip.h, ABI 9: vsrd_frame_header): frames whose instance counts differ share one FrameBatch whose rows
are laid out for a capacity, each row carrying its frame's own count.  Each frame must walk, bit for bit, the trajectory it walks alone in a
frame slot of its own N, and the pad instances of a row must be neither read nor written."""
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = [4, 2, 6, 1, 5, 3]
CAPACITY = 6
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
    # across the phase switch (step 9), the split-ray kernels of the batch (33..128 samples), eight slots per MLP-adjoint item alone and in the batch
    return optimization.OptimizationConfig(num_samples=40, num_rays=128, warmup_steps=9, num_steps=40, seed=3, mlp_adjoint_item_slots=8,
                                           mlp_split_bf16=split_bf16)


def _inputs(dev, frame, n, height=128, width=128):
    from vsrd_amd import launcher
    return launcher.synthetic_frame_inputs(dev, frame, 3, n, height=height, width=width)


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
    """The pad instances of a mixed batch's row: (tensor, fill) pairs over the capacity's rows beyond the frame's own."""
    from vsrd_amd import optimization
    n, cap = member.num_instances, member.capacity
    det, b = member.detector, member._glue
    pads = [(member.flat_masks[:, n:], "nan"), (b["gt_boxes"][:, n:], "nan"), (b["visible"][:, n:], 1)]
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
    for t, fill in _pads(member):
        if fill == "nan":
            assert bool((t.contiguous().view(torch.int32) == NAN_BITS).all()), t.shape
        else:
            assert bool((t == fill).all())


def _tensors_equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_tensors_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_tensors_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("split_bf16", [True, False], ids=["split_bf16", "fp32_mfma"])
def test_mixed_frame_batch_walks_each_frames_own_trajectory(dev, split_bf16):
    from vsrd_amd import formats, optimization
    config = _config(split_bf16)
    frames, alone, payloads = [], [], []
    # every frame alone, in a frame slot of its own N; frames whose soft masks do not suit the table sampler are skipped
    frame_number = 100
    for k, n in enumerate(COUNTS):
        while True:
            inputs = _inputs(dev, frame_number, n)
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
        slot.close()

    batch = optimization.FrameBatch(frames[:4], config, dev, init_seeds=[70, 71, 72, 73], max_instances=CAPACITY)
    assert all(row.layout == batch.arena.rows[0].layout for row in batch.arena.rows)
    assert [m.num_instances for m in batch.frames] == COUNTS[:4] and all(m.capacity == CAPACITY for m in batch.frames)
    batch.capture_all(actives=[4, 2])
    for group, active in (([0, 1, 2, 3], 4), ([4, 5], 2)):
        for row, k in enumerate(group):
            assert batch.reset(row, frames[k], init_seed=70 + k)
            _fill_pads(batch.frames[row])
        batch.run(STEPS, active=active)
        torch.cuda.synchronize()
        for row, k in enumerate(group):
            member = batch.frames[row]
            assert member.step_index == STEPS and member.num_instances == COUNTS[k]
            for index, (a, b) in enumerate(zip(_state(member), alone[k])):
                assert a.shape == b.shape and torch.equal(a, b), (k, index)
            _pads_untouched(member)
            assert _tensors_equal(formats.checkpoint_payload(member, STEPS, host=True), payloads[k]), k
            assert batch.outputs(row)["raw_gradients"][0].shape == (1, COUNTS[k], 3)

    # refusals: no instance, more than the capacity, another image size; a mixed batch without a capacity; the residual phase
    empty = optimization.FrameInputs(frames[0].image_size, frames[0].intrinsic_matrices, frames[0].extrinsic_matrices, frames[0].soft_masks[..., :0],
                                     frames[0].boxes_2d[:, :0], frames[0].visible_masks[:, :0])
    for refused in (empty, _inputs(dev, 7, CAPACITY + 1), _inputs(dev, 7, 3, height=96)):
        with pytest.raises(ValueError):
            batch.reset(0, refused, init_seed=1)
    batch.close()
    with pytest.raises(ValueError):
        optimization.FrameBatch(frames[:2], config, dev)
    with pytest.raises(ValueError):
        optimization.FrameBatch(frames[:2], config, dev, max_instances=3)


def test_silhouette_step_header_twin(dev):
    """vsrd_render_silhouette_step_with_header: a header with num_instances = N gives the bits of the old entry point (split-ray form); a
    header of n < N covers the first n instances only and matches a launch on those n; a header on the dense multi-ray form is refused."""
    from vsrd_amd import _lib
    lib = _lib.load()
    N, S, R = 4, 40, 96
    g = torch.Generator().manual_seed(5)
    instances = torch.zeros(N, 16)
    instances[:, 0:3] = torch.randn(N, 3, generator=g) * 0.5 + torch.tensor([0.0, 0.0, 6.0])
    instances[:, 3] = instances[:, 7] = instances[:, 11] = 1.0
    instances[:, 12:15] = 0.5 + torch.rand(N, 3, generator=g)
    instances = instances.to(dev)
    directions = torch.randn(R, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.0])
    directions = (directions / directions.norm(dim=-1, keepdim=True)).to(dev)
    origins = torch.zeros(R, 3, device=dev)
    targets = torch.rand(R, N, generator=g).to(dev)
    workspace = torch.empty(lib.vsrd_workspace_bytes(N, 0), dtype=torch.uint8, device=dev)

    def run(n, header_count=None, flags=_lib.FLAG_STEP_SPLIT_RAY, rows=None):
        field = _lib.make_field(instances if rows is None else rows, 0.5)
        config = _lib.make_config(R, S, (0.0, 20.0), 0.3, 1.0, 1.0e-6, 3, seed=9, flags=flags)
        loss = torch.zeros(1, device=dev)
        grads = torch.full((N if rows is None else rows.shape[0], 16), 7.0, device=dev)
        scale = 1.0 / (R * n)
        t = targets if rows is None else targets[:, :rows.shape[0]].contiguous()
        if header_count is None:
            code = lib.vsrd_render_silhouette_step(field, config, _lib.ptr(origins), _lib.ptr(directions), None, None, _lib.ptr(t), None, scale,
                                                   workspace.data_ptr(), workspace.numel(), _lib.ptr(loss), _lib.ptr(grads), None, _lib.stream())
        else:
            header = torch.zeros(2, dtype=torch.int32, device=dev)
            header[0] = header_count
            header.view(torch.float32)[1] = 1.0 / (R * header_count)
            code = lib.vsrd_render_silhouette_step_with_header(field, config, _lib.ptr(origins), _lib.ptr(directions), None, None, _lib.ptr(t), None,
                                                               123.0, workspace.data_ptr(), workspace.numel(), _lib.ptr(loss), _lib.ptr(grads), None,
                                                               header.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        return code, loss, grads

    code_old, loss_old, grads_old = run(N)
    code_new, loss_new, grads_new = run(N, header_count=N)
    assert code_old == code_new == 0
    assert torch.equal(loss_old, loss_new) and torch.equal(grads_old, grads_new)
    # a header of 3 on a row of 4: the first 3 instances, exactly what a field of those 3 gives alone (targets strided by 4); row 3 untouched
    _, loss_3, grads_3 = run(3, rows=instances[:3].contiguous())
    code, loss_h, grads_h = run(3, header_count=3)
    assert code == 0 and torch.equal(loss_h, loss_3) and torch.equal(grads_h[:3], grads_3)
    assert bool((grads_h[3] == 7.0).all())
    # the dense multi-ray form does not batch: a header there is refused
    code, _, _ = run(N, header_count=N, flags=0)
    assert code == _lib.E_UNSUPPORTED


def test_frame_prologue_and_epilogue_header_twins(dev):
    """vsrd_frame_prologue_with_header / vsrd_frame_epilogue_with_header with a header of num_instances = N give the bits of the old entry
    points on the same buffers."""
    from vsrd_amd import _lib, optimization
    lib = _lib.load()
    config = _config(True)
    inputs = None
    for frame in range(100, 140):
        try:
            loop = optimization.FrameOptimizer(_inputs(dev, frame, 4), config, dev, graph=True, persistent=True)
        except optimization.UnsuitableFrameError:
            continue
        break
    loop.step(); loop.step(); torch.cuda.synchronize()             # (moments and a step counter that are not all zero)
    b, det, N = loop._glue, loop.detector, loop.num_instances
    header = torch.zeros(2, dtype=torch.int32, device=dev)
    header[0] = N
    header.view(torch.float32)[1] = 1.0 / (config.num_rays * N)
    outs = ("instances", "pd_indices", "gt_indices", "target_columns", "instance_weights", "projection_losses", "grad_raw")
    args = (loop._frame, _lib.ptr(det.locations.data), _lib.ptr(det.dimensions.data), _lib.ptr(det.orientations.data), _lib.ptr(b["extrinsics"]),
            _lib.ptr(b["intrinsics"]), _lib.ptr(b["gt_boxes"]), b["visible"].data_ptr(), loop.step_tensor.data_ptr(), b["scratch"].data_ptr(),
            b["scratch"].numel(), _lib.ptr(b["instances"]), b["pd_indices"].data_ptr(), b["gt_indices"].data_ptr(), b["target_columns"].data_ptr(),
            _lib.ptr(b["instance_weights"]), _lib.ptr(loop.schedule), _lib.ptr(b["projection_losses"]), _lib.ptr(b["grad_raw"]))
    results = []
    for twin in (False, True):
        for name in outs:
            b[name].zero_()
        code = lib.vsrd_frame_prologue_with_header(*args, header.data_ptr(), _lib.stream()) if twin else lib.vsrd_frame_prologue(*args, _lib.stream())
        torch.cuda.synchronize()
        assert code == 0
        results.append([b[name].clone() for name in outs] + [loop.schedule.clone()])
    for a, c in zip(*results):
        assert torch.equal(a, c)
    # the epilogue updates the parameters in place: the same start for both
    tensors = [det.locations, det.dimensions, det.orientations, loop.step_tensor, b["record"], b["raw_gradients"]]
    tensors += [loop.optimizer.state[p][k] for p in (det.locations, det.dimensions, det.orientations) for k in ("exp_avg", "exp_avg_sq", "step")]
    tensors += [g["lr"] for g in loop.optimizer.param_groups]
    start = [t.detach().clone() for t in tensors]
    groups = loop.optimizer.param_groups
    args = (loop._frame, _lib.ptr(b["grad_instances"]), _lib.ptr(b["grad_raw"]), _lib.ptr(b["projection_losses"]), _lib.ptr(b["render_losses"]), 0.0,
            loop._adam[0], loop._adam[1], loop._adam[2], _lib.ptr(groups[3]["lr"]), _lib.ptr(groups[4]["lr"]), loop.step_tensor.data_ptr(),
            _lib.ptr(b["record"]), _lib.ptr(b["raw_gradients"]))
    results = []
    for twin in (False, True):
        with torch.no_grad():
            for t, s0 in zip(tensors, start):
                t.copy_(s0)
        code = lib.vsrd_frame_epilogue_with_header(*args, header.data_ptr(), _lib.stream()) if twin else lib.vsrd_frame_epilogue(*args, _lib.stream())
        torch.cuda.synchronize()
        assert code == 0
        results.append([t.detach().clone() for t in tensors])
    for a, c in zip(*results):
        assert torch.equal(a, c)
    loop.close()


def test_outputs_asked_in_any_order_equal_each_frame_alone(dev):
    """labels() / masks() / metrics() create their buffers at first use, in the order they are first asked for: a batch asked in the order
    metrics, masks, labels and one asked in the order labels, masks, metrics lay their rows out differently behind what a batch that never
    asks has, give -- bit for bit -- what each frame gives alone in a slot of its own, and leave the trajectory alone."""
    import dataclasses
    from vsrd_amd import launcher, optimization
    inputs = [launcher.synthetic_frame_inputs(dev, 3, 2, 3, height=32, width=64), launcher.synthetic_frame_inputs(dev, 4, 2, 5, height=32, width=64)]
    config = optimization.OptimizationConfig(num_samples=40, num_rays=64, warmup_steps=3, num_steps=12, seed=3, mlp_adjoint_item_slots=8)

    def snapshot(result):
        return {key: value.clone() if isinstance(value, torch.Tensor) else value for key, value in result.items()}

    def same(got, want):
        return got.keys() == want.keys() and all(torch.equal(got[key], want[key]) if isinstance(want[key], torch.Tensor) else got[key] == want[key] for key in want)

    alone = []
    for k, frame in enumerate(inputs):
        loop = optimization.FrameOptimizer(frame, dataclasses.replace(config, init_seed=70 + k), dev, graph=True, persistent=True)
        loop.run(4, steps_per_graph=1)                  # (one step into the residual phase)
        alone.append(dict(labels=snapshot(loop.labels()), masks=snapshot(loop.masks(soft=True)), metrics=snapshot(loop.metrics())))
        torch.cuda.synchronize()
        loop.close()

    def walk(order):
        batch = optimization.FrameBatch(inputs, config, dev, init_seeds=[70, 71], max_instances=8)
        prefix = list(batch.arena.rows[0].layout)
        batch.run(4, steps_per_graph=1)
        ask = dict(labels=batch.labels, masks=lambda: batch.masks(soft=True), metrics=batch.metrics)
        got = {name: [snapshot(entry) for entry in ask[name]()] for name in order}
        layout = list(batch.arena.rows[0].layout)
        assert all(row.layout == layout for row in batch.arena.rows) and layout[:len(prefix)] == prefix and list(batch.frames[0]._outputs) == list(order)
        batch.run(3, steps_per_graph=1)
        torch.cuda.synchronize()
        record = [[m._glue["record"].clone(), m._glue["raw_gradients"].clone(), batch.outputs(f)["loss"].clone()] for f, m in enumerate(batch.frames)]
        record += [[p.detach().clone() for p in m.detector.parameters()] for m in batch.frames]
        batch.close()
        return got, layout[len(prefix):], record

    got_a, tail_a, record_a = walk(("metrics", "masks", "labels"))
    got_b, tail_b, record_b = walk(("labels", "masks", "metrics"))
    got_c, tail_c, record_c = walk(())
    for name in ("labels", "masks", "metrics"):
        for f in range(2):
            assert same(got_a[name][f], alone[f][name]), (name, f)
            assert same(got_b[name][f], got_a[name][f]), (name, f)
    assert tail_c == [] and len(tail_a) == len(tail_b) == 13 and tail_a != tail_b
    assert sorted(nbytes for _, nbytes in tail_a) == sorted(nbytes for _, nbytes in tail_b)
    for other in (record_b, record_c):
        assert all(torch.equal(x, y) for mine, theirs in zip(record_a, other) for x, y in zip(mine, theirs))


def test_all_five_outputs_of_a_batch_equal_each_frame_alone(dev):
    """The one table's five outputs at the smallest shape that can still go wrong -- 2 views of 16 x 72 (two runs per image row, the second a
    tail of 8 pixels), 3 and 2 instances in rows of capacity 3 with 2 label views, surface=True, one step into the residual phase: the batch
    asked in the table's order and each frame alone, in a slot of its own, asked in the reverse order give the same tensors bit for bit.
    (Every loop starts from the boxes its frame was made of: from a fresh draw -- every box at 50 m, a pixel of this image -- four steps
    leave nothing for the dense outputs to show.)"""
    import dataclasses
    from vsrd_amd import launcher, optimization, synthetic
    config = optimization.OptimizationConfig(num_samples=40, num_rays=64, warmup_steps=3, num_steps=4, seed=3, mlp_adjoint_item_slots=8,
                                             surface_num_iterations=64)
    order = list(optimization._OUTPUTS)
    assert order == ["labels", "masks", "metrics", "group_labels", "surface"]
    photographs = [torch.arange(16 * 72 * 3, device=dev).mul(7 + k).remainder(251).to(torch.uint8).view(16, 72, 3) for k in range(2)]

    def ask(source, name, background, **batch):
        arguments = dict(masks=dict(soft=True), surface=dict(light=(0.2, 1.0, 0.4), background=background))
        return getattr(source, name)(**batch, **arguments.get(name, {}))

    def start_at_the_truth(loop, number):
        _, _, location, dimension, orientation = synthetic.synthetic_frame(number, 2, 16, 72, loop.num_instances)
        with torch.no_grad():
            loop.detector.locations.copy_(location); loop.detector.dimensions.copy_(dimension); loop.detector.orientations.copy_(orientation)

    def bits(tensor):        # (float32 as its bits: NaN equals NaN)
        return tensor.contiguous().view(torch.int32) if tensor.dtype == torch.float32 else tensor

    def snapshot(result):
        return {key: value.clone() if isinstance(value, torch.Tensor) else value for key, value in result.items()}

    inputs, numbers, alone, number = [], [], [], 3
    for k, n in enumerate((3, 2)):
        while True:          # (frames whose soft masks do not suit the table sampler are skipped)
            frame = launcher.synthetic_frame_inputs(dev, number, 2, n, height=16, width=72, label_views=2)
            number += 1
            try:
                loop = optimization.FrameOptimizer(frame, dataclasses.replace(config, init_seed=70 + k), dev, graph=True, persistent=True, max_label_views=2)
            except optimization.UnsuitableFrameError:
                assert number < 40
                continue
            break
        numbers.append(number - 1)
        start_at_the_truth(loop, numbers[-1])
        loop.run(config.num_steps, steps_per_graph=1)
        alone.append({name: snapshot(ask(loop, name, photographs[k])) for name in reversed(order)})
        assert list(loop._outputs) == order[::-1]
        torch.cuda.synchronize()
        loop.close()
        inputs.append(frame)

    batch = optimization.FrameBatch(inputs, config, dev, init_seeds=[70, 71], max_instances=3, max_label_views=2, surface=True)
    assert batch.unsuitable_founders == [] and [m.num_instances for m in batch.frames] == [3, 2]
    for member, made_of in zip(batch.frames, numbers):
        start_at_the_truth(member, made_of)
    batch.run(config.num_steps, steps_per_graph=1)
    assert all(m.step_index - 1 >= config.warmup_steps for m in batch.frames)          # (the last step was a residual one)
    got = {name: [snapshot(entry) for entry in ask(batch, name, photographs, active=2)] for name in order}
    torch.cuda.synchronize()
    assert list(batch.frames[0]._outputs) == order and all(row.layout == batch.arena.rows[0].layout for row in batch.arena.rows)
    compared = 0
    for name in order:
        for f in range(2):
            mine, theirs = got[name][f], alone[f][name]
            assert mine.keys() == theirs.keys(), (name, f)
            for key, value in theirs.items():
                if isinstance(value, torch.Tensor):
                    assert mine[key].shape == value.shape and mine[key].dtype == value.dtype, (name, f, key)
                    assert torch.equal(bits(mine[key]), bits(value)), (name, f, key)
                    compared += 1
                else:
                    assert mine[key] == value, (name, f, key)
    assert compared >= 2 * (5 + 4 + 4 + 6 + 6)
    owned = [int((entry["instance"] != 255).sum()) for entry in got["surface"]]
    inside = [int(entry["counts"][:, 0].sum()) for entry in got["masks"]]
    print("pixels of", 16 * 72, "that own an instance in the surface render:", owned, "and that lie inside a predicted mask:", inside)
    assert 0 < sum(owned) < 2 * 16 * 72 and sum(inside) > 0          # (the dense outputs show something, and not everything)
    batch.close()
