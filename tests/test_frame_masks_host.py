"""The host side of vsrd_frame_masks: the binding against the header, the mask files, the IoU from counts, the launcher's flag and the
checkpoint metric -- no GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsrd_hip.h")


def test_binding_has_the_prototype_and_the_struct():
    """The prototype and the leading structures of its binding (vsrd_frame_masks_config against gcc's view of the header, member by member:
    tests/test_host_logic.py::test_struct_matches_the_header[FrameMasksConfig])."""
    from vsrd_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"^int32_t\s+vsrd_frame_masks\s*\(", header, flags=re.M)
    restype, argtypes = _lib.SIGNATURES["vsrd_frame_masks"]
    assert restype is ctypes.c_int32 and len(argtypes) == 14
    assert argtypes[:3] == [ctypes.POINTER(_lib.Field), ctypes.POINTER(_lib.RenderConfig), ctypes.POINTER(_lib.FrameMasksConfig)]
    assert [name for name, _ in _lib.FrameMasksConfig._fields_] == ["view", "num_views", "height", "width", "num_iterations", "convergence_criteria", "bounding_radius",
                                                                   "threshold", "target_stride"]


def test_the_abi_version_is_still_12():
    from vsrd_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"^#define VSRD_ABI_VERSION 12$", header, flags=re.M) and _lib.ABI_VERSION == 12
    assert "added within ABI 12; probe for the symbol" in header


def _masks(rng, n=3, height=5, width=13):
    from vsrd_amd import optimization
    bits = rng.random((n, height, width)) < 0.4
    counts = torch.tensor([[int(b.sum()), 7, min(int(b.sum()), 3)] for b in bits], dtype=torch.int32)
    return bits, dict(inside=torch.from_numpy(np.packbits(bits, axis=-1)), counts=counts, mask_iou=optimization.mask_iou(counts), threshold=0.25)


def test_mask_files_round_trip_and_frames_unpacks_them(tmp_path):
    from vsrd_amd import formats, frames
    bits, masks = _masks(np.random.default_rng(0))
    path = formats.save_frame_masks(str(tmp_path), masks, (5, 13))
    assert path == str(tmp_path / "masks" / "view_00.npz") and os.listdir(tmp_path / "masks") == ["view_00.npz"]      # (no temporary file left)
    for source in (path, str(tmp_path)):
        loaded = formats.load_frame_masks(source)
        assert loaded["shape"] == (5, 13) and loaded["threshold"] == 0.25
        assert np.array_equal(loaded["inside"], masks["inside"].numpy()) and loaded["inside"].dtype == np.uint8
        assert np.array_equal(loaded["counts"], masks["counts"].numpy()) and np.array_equal(loaded["mask_iou"], masks["mask_iou"].numpy())
        assert np.array_equal(frames.unpack_masks(loaded["inside"], loaded["shape"][1]), bits)
    with pytest.raises(ValueError):
        formats.save_frame_masks(str(tmp_path), masks, (5, 24))
    with pytest.raises(ValueError):
        frames.unpack_masks(masks["inside"].numpy(), 24)
    # the same routine unpacks a pack's own masks
    assert np.array_equal(frames.unpack_masks(np.packbits(bits, axis=-1), 13), bits)


def test_mask_iou_from_counts():
    from vsrd_amd import optimization
    counts = torch.tensor([[10, 10, 10], [8, 4, 2], [0, 0, 0], [5, 0, 0], [0, 3, 0]], dtype=torch.int32)
    iou = optimization.mask_iou(counts)
    assert iou.dtype == torch.float32
    assert torch.equal(iou, torch.tensor([1.0, 0.2, 0.0, 0.0, 0.0]))


def test_sphere_tracing_defaults_are_the_references():
    from vsrd_amd import optimization
    config = optimization.OptimizationConfig()
    assert (config.surface_num_iterations, config.surface_convergence_criteria, config.surface_bounding_radius) == (1000, 0.01, 100.0)


def test_launcher_masks_needs_out():
    env = dict(os.environ, PYTHONPATH=ROOT)
    done = subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", "1", "--masks"], capture_output=True, text=True, cwd=ROOT, env=env)
    assert done.returncode != 0 and "--masks" in done.stderr and "--out" in done.stderr
    done = subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", "1", "--masks", "--out", "x", "--selftest"],
                          capture_output=True, text=True, cwd=ROOT, env=env)
    assert done.returncode != 0 and "--selftest" in done.stderr


class _Loop:
    """What formats.checkpoint_payload reads of a loop."""
    def __init__(self):
        self.detector = torch.nn.Linear(2, 2)
        self.hyper_distance_field = torch.nn.Linear(2, 1)

    def optimizer_state_dict(self):
        return {}

    def scheduler_state_dict(self):
        return {}


def test_checkpoint_metric_is_a_float_select_model_can_compare(tmp_path):
    """tools/select_model.py compares checkpoint["metrics"][name] with < / > against a float and keeps the best (select_model.py:30-45)."""
    from vsrd_amd import formats, optimization
    value = float(optimization.mask_iou(torch.tensor([[8, 4, 2], [10, 10, 10]])).mean())
    payload = formats.checkpoint_payload(_Loop(), step=9, metrics={"mask_iou": value}, host=True)
    formats.atomic_torch_save(payload, str(tmp_path / "step_final.pt"))
    loaded = torch.load(str(tmp_path / "step_final.pt"), weights_only=False)
    metric = loaded["metrics"]["mask_iou"]
    assert type(metric) is float and metric == pytest.approx(0.6)
    best = -float("inf")
    assert metric > best and not metric < best
