"""The photometric term in a FrameBatch (vsrd_amd/optimization.py: FrameBatch(..., photometric=True)): each row of a batch walks, bit for
bit, the trajectory its frame walks alone in a persistent FrameOptimizer slot -- which issues the one-frame symbols, as before -- while the
batch issues vsrd_sample_rays_table_frames, vsrd_frame_photometric_with_header and vsrd_frame_photometric_finish_with_header once per step
for all its frames.  Everything is equality of bits.

The scene is tests/test_hip_step_photometric.py's (V = 3, 128 x 128, N = 4, R = 256, with 40 samples per ray: a batch runs the split-ray kernels, 48 photometric rays, 11 x 11 patches, k = 3),
the term's rays are drawn on the device.  The frames differ in images and in the draw of their initial hypernetwork; every frame starts from
that file's start boxes (new_loop), which the target view's rays hit.  A comparison shows something only where the term acts: for every
frame the run ALONE is asserted to have stats[1] > 0 in at least one residual step.
"""
import dataclasses
import os
import sys

import pytest
import torch

from test_hip_step_photometric import N, config, frame, same_bits, start_parameters

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

SAMPLES = 40                            # (33..128 samples: the split-ray kernels a batch runs in, tests/test_hip_step.py)
WARMUP, STEPS = 4, 8                    # (capture_all captures a phase's one-step graph behind three eager steps: both phases need four)
SEEDS = [(400, 50), (401, 51), (402, 52), (403, 53), (404, 54)]         # (image seed, init seed) of the five frames


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def batch_config(weight=None):
    """The scene's config with a sample count a batch serves, and eight slots per work item of the MLP adjoint alone and in the batch (the
    order of summation of the weight adjoints depends on that number and on nothing else of the launch)."""
    cfg = config(warmup=WARMUP, mlp_adjoint_item_slots=8) if weight is None else config(weight=weight, warmup=WARMUP, mlp_adjoint_item_slots=8)
    return dataclasses.replace(cfg, num_samples=SAMPLES)


def narrowed(inputs, n):
    """The frame with its first n instances only."""
    if n == N:
        return inputs
    return dataclasses.replace(inputs, soft_masks=inputs.soft_masks[..., :n].contiguous(), boxes_2d=inputs.boxes_2d[:, :n].contiguous(),
                               visible_masks=inputs.visible_masks[:, :n].contiguous())


def place_start(loop):
    """tests/test_hip_step_photometric.py::new_loop: the start boxes, in place of the fresh detector's draw."""
    n = loop.num_instances
    with torch.no_grad():
        for p, v in zip((loop.detector.locations, loop.detector.dimensions, loop.detector.orientations), start_parameters()):
            p.copy_(v[None, :n].to(p.device))


def state_of(loop):
    params = list(loop.detector.parameters()) + list(loop.hyper_distance_field.parameters())
    out = [p.detach().clone() for p in params]
    for p in params:
        state = loop.optimizer.state.get(p)
        if state:
            out += [state[k].detach().clone() for k in ("exp_avg", "exp_avg_sq", "step")]
    out += [loop._glue["record"].clone(), loop._glue["ray_indices"].clone()]
    if loop._photometric is not None:
        out += [loop._photometric["ray_indices"].clone(), loop._photometric["loss"].clone(), loop._photometric["stats"].clone()]
    return out


_alone = {}


def alone(dev, cfg, frames, seeds, tag):
    """Every frame's trajectory in a persistent slot of its own shape, step by step: [frame][step] -> state (made once per `tag`)."""
    if tag not in _alone:
        from vsrd_amd import optimization
        slots, trajectories = {}, []
        for inputs, seed in zip(frames, seeds):
            n = int(inputs.soft_masks.shape[-1])
            if n not in slots:
                slots[n] = optimization.FrameOptimizer(inputs, cfg, dev, graph=True, persistent=True)
                slots[n].capture_all(steps_per_graph=1)
            slot = slots[n]
            assert slot.reset(inputs, init_seed=seed) is True
            place_start(slot)
            states = []
            for _ in range(STEPS):
                slot.step()
                torch.cuda.synchronize()
                states.append(state_of(slot))
            trajectories.append(states)
        for slot in slots.values():
            slot.close()
        _alone[tag] = trajectories
    return _alone[tag]


def acted(states):
    """The residual steps of a trajectory in which the term had a converged ray (stats[1] > 0)."""
    return [step for step in range(WARMUP, STEPS) if float(states[step][-1][1]) > 0]


def walk(batch, rows, trajectories, active):
    for row, k in enumerate(rows):
        place_start(batch.frames[row])
    for step in range(STEPS):
        batch.step(active=active)
        torch.cuda.synchronize()
        for row, k in enumerate(rows):
            member = batch.frames[row]
            for index, (a, b) in enumerate(zip(state_of(member), trajectories[k][step])):
                assert same_bits(a, b), (k, step, index)
            if step >= WARMUP:
                assert same_bits(batch.outputs(row)["photometric_loss"].reshape(1), trajectories[k][step][-2])


# ---- 6: each row of a batch walks the trajectory of its frame alone -------------------------------------------------------------------------
def test_each_row_walks_the_trajectory_of_its_frame_alone(dev):
    from vsrd_amd import optimization
    cfg = batch_config()
    frames = [frame(dev, image_seed) for image_seed, _ in SEEDS]
    seeds = [init_seed for _, init_seed in SEEDS]
    trajectories = alone(dev, cfg, frames, seeds, "uniform")
    for k, states in enumerate(trajectories):
        print(f"test_each_row_walks_the_trajectory_of_its_frame_alone: frame {k} alone: the term acts in steps {acted(states)}, "
              f"stats {[states[s][-1].tolist() for s in range(WARMUP, STEPS)]}")
        assert acted(states), k
    assert not same_bits(trajectories[0][-1][0], trajectories[1][-1][0])                  # (the frames ARE different problems)
    batch = optimization.FrameBatch(frames[:3], cfg, dev, init_seeds=seeds[:3], photometric=True)
    assert all(row.layout == batch.arena.rows[0].layout for row in batch.arena.rows)
    assert all(m._photometric is not None for m in batch.frames)
    batch.capture_all(steps_per_graph=1, actives=[3, 2])
    graphs = len(batch._graphs)
    for rows, active in (([0, 1, 2], 3), ([3, 4], 2)):
        for row, k in enumerate(rows):
            assert batch.reset(row, frames[k], init_seed=seeds[k]) is True
        walk(batch, rows, trajectories, active)
    assert len(batch._graphs) == graphs                                                   # a group of frames in a captured batch captures nothing
    batch.close()


# ---- 7: weight 0 ---------------------------------------------------------------------------------------------------------------------------
def test_weight_zero_changes_nothing(dev):
    from vsrd_amd import optimization
    cfg = batch_config(weight=0.0)
    frames = [frame(dev, image_seed) for image_seed, _ in SEEDS[:2]]
    batches = [optimization.FrameBatch(frames, cfg, dev, init_seeds=[50, 51], photometric=flag) for flag in (True, False)]
    assert batches[0].arena.stride == batches[1].arena.stride
    assert all(m._photometric is None for b in batches for m in b.frames) and not batches[0].photometric
    for batch in batches:
        for member in batch.frames:
            place_start(member)
    for step in range(STEPS):
        for batch in batches:
            batch.step()
        torch.cuda.synchronize()
        for a, b in zip(batches[0].frames, batches[1].frames):
            for x, y in zip(state_of(a), state_of(b)):
                assert same_bits(x, y), step
        assert "photometric_loss" not in batches[0].outputs(0)
    for batch in batches:
        batch.close()


# ---- 8: frames that differ in instance count -------------------------------------------------------------------------------------------------
def test_a_mixed_batch_walks_its_frames_trajectories(dev):
    """max_instances = 4, frames of 4 and 2 instances: each row equals its frame in a slot of its own N, over the phase switch."""
    from vsrd_amd import optimization
    cfg = batch_config()
    frames = [frame(dev, SEEDS[0][0]), narrowed(frame(dev, SEEDS[1][0]), 2)]
    seeds = [SEEDS[0][1], SEEDS[1][1]]
    trajectories = alone(dev, cfg, frames, seeds, "mixed")
    for k, states in enumerate(trajectories):
        print(f"test_a_mixed_batch_walks_its_frames_trajectories: frame {k} alone: the term acts in steps {acted(states)}")
        assert acted(states), k
    batch = optimization.FrameBatch(frames, cfg, dev, init_seeds=seeds, max_instances=4, photometric=True)
    assert [m.num_instances for m in batch.frames] == [4, 2] and all(m.capacity == 4 for m in batch.frames)
    for row in range(2):
        assert batch.reset(row, frames[row], init_seed=seeds[row]) is True
    walk(batch, [0, 1], trajectories, 2)
    batch.close()


# ---- 9: frames from packs with images ------------------------------------------------------------------------------------------------------
def pack_of(frame, images=True):
    """A synthetic frame pack of 3 views of 128 x 192 with 3 instances (frames 1, 4 and 8: a few hundred pixels in the target's masks)."""
    import make_frame_packs
    return make_frame_packs.make_pack(frame, 3, 128, 192, 3, images=images)


def pack_config():
    from vsrd_amd import losses, optimization
    return optimization.OptimizationConfig(num_samples=SAMPLES, num_rays=64, warmup_steps=2, num_steps=8, seed=3, mlp_adjoint_item_slots=8, surface_num_rays=16,
                                           surface_top_k=3, surface_patch_size=(5, 5), surface_num_iterations=50,
                                           loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": 0.05})


def test_a_row_reset_from_a_pack_holds_the_gray_planes_of_the_ingested_frame(dev):
    """reset(FramePack with images) into a row against reset(frames.ingest(pack)) into its neighbour: the same gray planes, hard-mask weights
    and, over the phase switch, the same trajectory, bit for bit; a pack without images is refused before the row is touched."""
    from vsrd_amd import frames, optimization
    founder = frames.ingest(pack_of(1), dev)
    assert founder.images.dtype == torch.float32 and tuple(founder.images.shape) == (3, 3, 128, 192)
    batch = optimization.FrameBatch([founder, founder], pack_config(), dev, init_seeds=[1, 2], photometric=True)
    for number in (8, 4):
        pack = pack_of(number)
        assert batch.reset(0, pack, init_seed=11) is True
        assert batch.reset(1, frames.ingest(pack, dev), init_seed=11) is True
        a, b = (m._photometric for m in batch.frames)
        expected = torch.from_numpy(pack.images).to(dev).to(torch.float32) / 255.0
        assert same_bits(batch.frames[0].inputs.images, expected) and same_bits(batch.frames[1].inputs.images, expected)
        assert same_bits(a["gray"], b["gray"]) and float(a["gray"].abs().max()) > 0.1
        assert same_bits(a["gray"], optimization.losses.grayscale_images(expected))
        assert same_bits(a["hard_weights"], b["hard_weights"]) and int(a["hard_weights"].sum()) >= 16
        assert not same_bits(a["gray"], optimization.losses.grayscale_images(founder.images))
        batch.run(4)
        torch.cuda.synchronize()
        for index, (x, y) in enumerate(zip(state_of(batch.frames[0]), state_of(batch.frames[1]))):
            assert same_bits(x, y), (number, index)
        assert "photometric_loss" in batch.outputs(0) and same_bits(batch.outputs(0)["photometric_loss"].reshape(1), batch.outputs(1)["photometric_loss"].reshape(1))
    # a frame the term cannot take is refused before anything of the row changes
    torch.cuda.synchronize()
    before = batch.arena.buffer.clone()
    with pytest.raises(ValueError, match="images"):
        batch.reset(0, pack_of(1, images=False), init_seed=5)
    with pytest.raises(ValueError, match="images"):
        batch.reset(1, dataclasses.replace(founder, images=None), init_seed=5)
    torch.cuda.synchronize()
    assert torch.equal(batch.arena.buffer, before)
    assert batch.frames[0].step_index == 4 and batch.frames[0].inputs.images is not None
    batch.close()
