"""The host side of the photometric term in frame batches and of what carries images to it (vsrd_amd/optimization.py: FrameBatch(..., photometric=True); include/vsrd_hip.h:
vsrd_frame_photometric_with_header, vsrd_frame_photometric_finish_with_header, vsrd_sample_rays_table_frames): the keyword and its default
refusal, the refusals that need no device, the C ABI's declarations and the size of a row that carries the term."""
import argparse
import ctypes
import dataclasses
import inspect
import os
import re
import sys

import numpy as np

import pytest
import torch

from test_frame_photometric_host import H, N, V, W, config, frame
from vsrd_amd import _lib, optimization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("vsrd_frame_photometric_with_header", "vsrd_frame_photometric_finish_with_header", "vsrd_sample_rays_table_frames")


def test_the_keyword_and_its_default_refusal():
    assert inspect.signature(optimization.FrameBatch.__init__).parameters["photometric"].default is False
    with pytest.raises(ValueError, match=r"not batched.*photometric=True"):
        optimization.FrameBatch([frame(), frame()], config(), "cuda:0")
    with pytest.raises(ValueError, match="not batched"):
        optimization.FrameBatch([frame(), frame()], config(), "cuda:0", photometric=False)


@pytest.mark.parametrize("what, inputs, cfg, capacities, match", [
    ("a frame without images", lambda: [frame(), frame(images=False)], lambda: config(), {}, "frame 1 of the batch.*images"),
    ("a frame with fewer views than top_k", lambda: [frame(), narrow_views(frame(), 2)], lambda: dataclasses.replace(config(), surface_top_k=3),
     dict(max_views=V), "frame 1 of the batch.*top_k"),
    ("too few hard pixels", lambda: [frame(hard_pixels=60), frame()], lambda: config(), {}, "frame 0 of the batch.*hard mask"),
    ("silhouette weight 0", lambda: [frame()], lambda: config(silhouette_loss=0.0), {}, "silhouette"),
])
def test_refusals_need_no_device(what, inputs, cfg, capacities, match):
    """(the checks sit in front of anything that touches a device: "cuda:0" is never opened)"""
    with pytest.raises(ValueError, match=match):
        optimization.FrameBatch(inputs(), cfg(), "cuda:0", photometric=True, **capacities)


def narrow_views(inputs, views):
    return dataclasses.replace(inputs, intrinsic_matrices=inputs.intrinsic_matrices[:views], extrinsic_matrices=inputs.extrinsic_matrices[:views],
                               soft_masks=inputs.soft_masks[:views], boxes_2d=inputs.boxes_2d[:views], visible_masks=inputs.visible_masks[:views],
                               images=inputs.images[:views])


def test_header_declares_the_symbols_and_the_binding_reads_them():
    with open(_lib.HEADER_PATH) as file:
        text = re.sub(r"/\*.*?\*/", "", file.read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"^int32_t\s+{name}\s*\(", text, flags=re.M), name
        assert name in _lib.SIGNATURES, name
    assert "#define VSRD_ABI_VERSION 12" in text and _lib.ABI_VERSION == 12
    one_frame, twin = _lib.SIGNATURES["vsrd_frame_photometric"], _lib.SIGNATURES["vsrd_frame_photometric_with_header"]
    # the twin: the one-frame call's arguments with the header in front of the stream
    assert twin[0] is ctypes.c_int32 and twin[1] == one_frame[1][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["vsrd_frame_photometric_finish_with_header"][1] == \
        _lib.SIGNATURES["vsrd_frame_photometric_finish"][1][:-1] + [ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p]
    assert _lib.SIGNATURES["vsrd_sample_rays_table_frames"][1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p,
                                                                   ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p]


def test_a_row_with_the_term_is_as_large_as_what_a_member_allocates():
    """FrameBatch._row_bytes(photometric=True) adds the sum over the term's declaration and its ray table, and a member allocates from that
    very declaration: its constructor's part, run on a host arena, leaves the row's cursor exactly there."""
    lib = _lib.load()
    cfg = dataclasses.replace(config(), surface_num_rays=48, surface_top_k=3)
    capacity_views, capacity = 5, 3
    shape = (capacity_views, H, W, capacity)
    without = optimization.FrameBatch._row_bytes(shape, cfg, headed=True)
    planned = optimization.FrameBatch._row_bytes(shape, cfg, headed=True, photometric=True)
    declared = optimization._photometric_buffers(capacity_views, capacity, H, W, cfg)
    assert [name for name, *_ in declared] == ["gray", "hard_weights", "ray_indices", "workspace", "loss", "stats", "grad_instances", "grad_mlp"]
    by_name = {name: (tuple(shape), dtype) for name, shape, dtype, _ in declared}
    assert by_name["gray"] == ((capacity_views, H, W), torch.float32) and by_name["ray_indices"] == ((48,), torch.int64)
    assert by_name["workspace"] == ((lib.vsrd_frame_photometric_workspace_bytes(capacity, 1, capacity_views, 48, 121),), torch.uint8)
    assert by_name["grad_mlp"] == ((capacity, _lib.MLP_WEIGHTS), torch.float32)
    aligned = optimization.FrameArena.aligned
    table = lib.vsrd_ray_table_bytes(H * W)
    assert planned - without == sum(aligned(optimization._buffer_bytes(s, d)) for _, s, d, _ in declared) + aligned(table)
    # weight 0: the keyword changes nothing
    off = dataclasses.replace(cfg, loss_weights={**cfg.loss_weights, "photometric_loss": 0.0})
    assert optimization.FrameBatch._row_bytes(shape, off, headed=True, photometric=True) == optimization.FrameBatch._row_bytes(shape, off, headed=True)
    # what a member's constructor allocates for the term, on a host arena
    arena = optimization.FrameArena(1, planned - without, "cpu")
    loop = object.__new__(optimization.FrameOptimizer)
    loop._row, loop.inputs, loop.config, loop.device = arena.rows[0], frame(), cfg, torch.device("cpu")
    loop.view_capacity, loop.capacity, loop.fused_glue, loop._graphs = capacity_views, capacity, True, {}
    loop._write_photometric = lambda: True                      # (the frame's contents and the table: device work)
    loop._init_photometric()
    assert set(by_name) <= set(loop._photometric) and tuple(loop._photometric["gray"].shape) == (capacity_views, H, W)
    arena.rows[0].bytes(table)                                   # (rendering.RayTable(allocate=row.bytes) in _write_photometric)
    assert arena.rows[0].cursor == planned - without == arena.stride


# ---- images in frame packs, synthetic images, the launcher's flag ------------------------------------------------------------------------
def small_pack(images):
    import make_frame_packs as tool
    return tool.make_pack(1, 3, 32, 64, 2, images=images)


def test_a_pack_round_trip_with_and_without_images(tmp_path):
    from vsrd_amd import frames, synthetic
    with_images, without = small_pack(True), small_pack(False)
    assert without.images is None and with_images.images.dtype == np.uint8 and with_images.images.shape == (3, 3, 32, 64)
    assert np.array_equal(with_images.images, synthetic.synthetic_images(1, 3, 32, 64).numpy())          # deterministic
    assert not np.array_equal(with_images.images, synthetic.synthetic_images(2, 3, 32, 64).numpy())
    assert int(with_images.images.max()) > 200 and int(with_images.images.min()) < 50                    # (texture, not a flat plane)
    for name, pack in (("with.npz", with_images), ("without.npz", without)):
        path = str(tmp_path / name)
        frames.save_pack(path, pack)
        with np.load(path) as data:
            assert ("images" in data.files) == (pack.images is not None)                                  # written only when present
        loaded = frames.load_pack(path)
        assert frames.pack_has_images(path) == (pack.images is not None)
        if pack.images is None:
            assert loaded.images is None
        else:
            assert loaded.images.dtype == np.uint8 and np.array_equal(loaded.images, pack.images)
        assert np.array_equal(loaded.inside, pack.inside) and np.array_equal(loaded.view_offsets, pack.view_offsets)
    # validated for shape and type
    for bad in (with_images.images[:2], with_images.images[:, :, :-1], with_images.images.astype(np.float32)):
        with pytest.raises(ValueError, match="images"):
            frames.validate(dataclasses.replace(with_images, images=bad))
        with pytest.raises(ValueError, match="images"):
            frames.save_pack(str(tmp_path / "bad.npz"), dataclasses.replace(with_images, images=bad))


def test_images_reach_the_loops_as_x_over_255():
    """frames.pack_images is the ONE conversion (frames.ingest and a row's reset(FramePack) both call it), and the launcher's synthetic frames
    define FrameInputs.images the same way: float32 x / 255."""
    from vsrd_amd import frames, launcher
    pack = small_pack(True)
    images = frames.pack_images(pack, "cpu")
    assert images.dtype == torch.float32 and tuple(images.shape) == (3, 3, 32, 64)
    assert torch.equal(images, torch.from_numpy(pack.images).to(torch.float32) / 255.0)
    assert float(images.max()) <= 1.0 and float(images.min()) >= 0.0
    assert frames.pack_images(small_pack(False), "cpu") is None
    for function in (frames.ingest, optimization.FrameOptimizer._ingest_pack):
        assert "pack_images(" in inspect.getsource(function), function
    assert "/ 255.0" in inspect.getsource(launcher.synthetic_frame_inputs)
    # a pack with images passes the term's host-side check, one without is refused by name of what it lacks
    cfg = dataclasses.replace(config(), surface_top_k=3)
    optimization._check_photometric(pack, cfg, pack.num_views, pack.num_instances)
    with pytest.raises(ValueError, match="images"):
        optimization._check_photometric(small_pack(False), cfg, 3, 2)
    with pytest.raises(ValueError, match="images of shape"):
        optimization._check_photometric(dataclasses.replace(pack, images=pack.images[:2]), cfg, 3, 2)


def test_the_pack_tool_writes_images_when_asked(tmp_path):
    import make_frame_packs as tool
    from vsrd_amd import frames
    assert tool.main(["--out", str(tmp_path / "a"), "--count", "2", "--views", "3", "--height", "32", "--width", "64", "--instances", "2", "--images"]) == 0
    assert tool.main(["--out", str(tmp_path / "b"), "--count", "1", "--views", "3", "--height", "32", "--width", "64", "--instances", "2"]) == 0
    assert all(frames.pack_has_images(str(tmp_path / "a" / f"frame_{k:06d}.npz")) for k in range(2))
    assert not frames.pack_has_images(str(tmp_path / "b" / "frame_000000.npz"))


def test_the_launchers_photometric_flag(tmp_path, monkeypatch):
    """Argument handling, without a device: the refusals that end a job before any rank starts, and what the flag sets in a process's work."""
    import make_frame_packs as tool
    from vsrd_amd import launcher
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    with pytest.raises(SystemExit, match="--photometric"):
        launcher.main(["--photometric", "0.1", "--selftest"])
    with pytest.raises(SystemExit, match="--photometric"):
        launcher.main(["--photometric", "-1"])
    bare, full = str(tmp_path / "bare"), str(tmp_path / "full")
    tool.write_packs(bare, 2, views=3, height=32, width=64, instances=[2])
    tool.write_packs(full, 2, views=3, height=32, width=64, instances=[2], images=True)
    with pytest.raises(SystemExit, match=r"--photometric.*frame_000000\.npz carries no images"):
        launcher.main(["--photometric", "0.1", "--frames-dir", bare])
    launcher.scan_images(launcher.scan_frames_dir(full)[0])                     # packs with images pass
    with pytest.raises(SystemExit, match="carries no images"):
        launcher.scan_images(launcher.scan_frames_dir(bare)[0])

    def work(weight):
        args = argparse.Namespace(num_steps=10, warmup_steps=5, rays=16, samples=8, fp32_mlp=False, adjoint_item_slots=0, photometric=weight)
        return launcher._RenderWork(args, {"seed": 3}, "cuda:0", None)
    on, off = work(0.25), work(0.0)
    assert on.photometric == 0.25 and optimization.photometric_weight(on.optimization_config()) == 0.25
    assert off.photometric == 0.0 and "loss_weights" not in off.config and optimization.photometric_weight(off.optimization_config()) == 0.0
    on._note_photometric(4, {"loss": 1.0, "photometric_loss": torch.tensor(0.375)})
    on._note_photometric(5, {"loss": 1.0})                                        # (a frame whose last step was box-only: no term)
    off._note_photometric(4, {"photometric_loss": torch.tensor(0.375)})
    assert on.photometric_losses == {4: 0.375} and off.photometric_losses == {}
    assert inspect.signature(launcher.synthetic_frame_inputs).parameters["images"].default is False
