"""The host side of vsrd_frame_metrics: frame packs that carry 3-D ground truth, the summary under the reference's six names, the
launcher's flag and the binding against the header -- no GPU."""
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


def _pack(instances=2, with_truth=True, with_rectification=True):
    from vsrd_amd import frames
    rng = np.random.default_rng(3)
    height, width, views = 6, 13, 2
    entries = views * instances
    polygon = np.array([[1, 1], [6, 1], [6, 4], [1, 4]], dtype=np.int32)
    boxes = rng.normal(size=(instances, 8, 3)).astype(np.float32)
    boxes[-1] = np.nan                                                  # (a slot without annotation)
    return frames.FramePack((height, width), np.tile(np.eye(3, dtype=np.float32), (views, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (views, 1, 1)),
                            np.arange(views + 1, dtype=np.int64) * instances, np.tile(np.arange(instances, dtype=np.int64), views),
                            np.arange(entries + 1, dtype=np.int64) * 4, np.tile(polygon, (entries, 1)),
                            np.zeros((entries, height, (width + 7) // 8), dtype=np.uint8),
                            boxes_3d=boxes if with_truth else None,
                            rectification_matrix=rng.normal(size=(3, 3)).astype(np.float32) if with_rectification else None)


@pytest.mark.parametrize("with_truth,with_rectification", [(True, True), (True, False), (False, False)])
def test_pack_round_trip_with_and_without_ground_truth(tmp_path, with_truth, with_rectification):
    from vsrd_amd import frames
    pack = _pack(with_truth=with_truth, with_rectification=with_rectification)
    path = str(tmp_path / "frame.npz")
    frames.save_pack(path, pack)
    with np.load(path) as data:                                        # (written only when present)
        assert ("boxes_3d" in data.files) == with_truth and ("rectification_matrix" in data.files) == with_rectification
    loaded = frames.load_pack(path)
    for field in frames._FIELDS[1:]:
        assert np.array_equal(getattr(loaded, field), getattr(pack, field)), field
    for field, present in (("boxes_3d", with_truth), ("rectification_matrix", with_rectification)):
        if present:
            assert getattr(loaded, field).dtype == np.float32 and np.array_equal(getattr(loaded, field), getattr(pack, field), equal_nan=True)
        else:
            assert getattr(loaded, field) is None


def test_a_pack_written_before_the_fields_existed_still_loads(tmp_path):
    """A file with the eight original members only -- every pack written so far -- loads with None in both fields."""
    from vsrd_amd import frames
    pack = _pack(with_truth=False, with_rectification=False)
    path = str(tmp_path / "old.npz")
    np.savez(path, **{field: np.asarray(getattr(pack, field)) for field in frames._FIELDS})
    loaded = frames.load_pack(path)
    assert loaded.boxes_3d is None and loaded.rectification_matrix is None and loaded.num_instances == 2
    assert frames.pack_counts(path) == (2, 6, 13, 2)
    positional = frames.FramePack(*[getattr(pack, field) for field in frames._FIELDS])          # (the old constructor call)
    assert positional.boxes_3d is None and positional.rectification_matrix is None


@pytest.mark.parametrize("field,shape", [("boxes_3d", (3, 8, 3)), ("boxes_3d", (2, 8, 2)), ("boxes_3d", (2, 24)), ("rectification_matrix", (4, 4)),
                                         ("rectification_matrix", (9,))])
def test_wrong_shapes_raise_and_name_the_file(tmp_path, field, shape):
    import dataclasses
    from vsrd_amd import frames
    pack = dataclasses.replace(_pack(), **{field: np.zeros(shape, dtype=np.float32)})
    path = str(tmp_path / "bad.npz")
    with pytest.raises(ValueError, match=field):
        frames.save_pack(path, pack)
    good = _pack()
    arrays = {name: np.asarray(getattr(good, name)) for name in frames._FIELDS + frames._OPTIONAL}
    arrays[field] = np.zeros(shape, dtype=np.float32)
    np.savez(path, **arrays)
    with pytest.raises(ValueError, match=r"bad\.npz.*" + field):
        frames.load_pack(path)


def test_frame_inputs_fields_are_optional_and_trailing():
    import dataclasses
    from vsrd_amd import optimization
    names = [f.name for f in dataclasses.fields(optimization.FrameInputs)]
    assert names[-2:] == ["boxes_3d", "rectification_matrix"]
    inputs = optimization.FrameInputs((2, 2), None, None, None, None, None)
    assert inputs.boxes_3d is None and inputs.rectification_matrix is None


def test_frame_metrics_are_the_six_formulas_of_the_reference():
    """scripts/main.py:908-915 on the oracle's IoUs of a few box pairs (one of them without annotation) against formats.frame_metrics of
    the summary laid out as vsrd_frame_metrics writes it."""
    from oracle import geometry
    from vsrd_amd import formats
    rng = np.random.default_rng(5)
    unit = np.array([[-1, -1, 1], [1, -1, 1], [1, -1, -1], [-1, -1, -1], [-1, 1, 1], [1, 1, 1], [1, 1, -1], [-1, 1, -1]], dtype=np.float64)

    def box(centre, size, yaw):
        c, s = np.cos(yaw), np.sin(yaw)
        world = (unit * size) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T + centre
        return np.stack([world[:, 0], world[:, 2], -world[:, 1]], axis=-1)                    # (z-up)

    ious_3d, ious_bev = [], []
    for shift in (0.1, 0.4, 0.9, 1.6, 5.0):
        size = rng.uniform(0.8, 2.0, 3)
        pair = geometry.box_3d_iou(box(np.zeros(3), size, 0.3), box(np.array([shift, 0.0, 0.2 * shift]), size * 1.05, 0.5))
        ious_3d.append(float(pair[0])); ious_bev.append(float(pair[1]))
    assert min(ious_3d) == 0.0 and max(ious_3d) > 0.5                                          # (the thresholds are exercised on both sides)
    a, b = torch.tensor(ious_3d, dtype=torch.float64), torch.tensor(ious_bev, dtype=torch.float64)
    expected = dict(iou_3d=torch.mean(a), iou_bev=torch.mean(b), accuracy_3d_25=torch.mean((a > 0.25).float()),
                    accuracy_bev_25=torch.mean((b > 0.25).float()), accuracy_3d_50=torch.mean((a > 0.50).float()),
                    accuracy_bev_50=torch.mean((b > 0.50).float()))
    summary = formats.frame_metrics_summary(ious_3d + [float("nan")], ious_bev + [float("nan")])
    assert summary[0] == 5.0 and summary[7] == 0.0 and len(summary) == 8
    named = formats.frame_metrics(summary)
    assert list(named) == ["iou_3d", "iou_bev", "accuracy_3d_25", "accuracy_bev_25", "accuracy_3d_50", "accuracy_bev_50"] == list(formats.FRAME_METRIC_NAMES)
    for name, value in expected.items():      # (the reference's accuracies are float32 means: half a float32 ulp of a share <= 1 is 3e-8)
        assert type(named[name]) is float and named[name] == pytest.approx(float(value), abs=1e-15 if name.startswith("iou") else 3e-8), name
    # the float32 tensor the kernel writes gives the same dictionary within float32
    from_tensor = formats.frame_metrics(torch.tensor(summary, dtype=torch.float32))
    assert all(type(v) is float and v == pytest.approx(named[k], abs=1e-7) for k, v in from_tensor.items()) and len(from_tensor) == 6
    # count 0: the reference logs no metrics
    assert formats.frame_metrics([0.0] * 8) == {} and formats.frame_metrics(torch.zeros(8)) == {}
    assert formats.frame_metrics_summary([float("nan")], [float("nan")]) == [0.0] * 8
    with pytest.raises(ValueError):
        formats.frame_metrics([1.0] * 7)


def test_mean_frame_metrics_of_the_jobs_line():
    from vsrd_amd import formats, launcher
    one = dict(zip(formats.FRAME_METRIC_NAMES, (0.5, 0.6, 1.0, 1.0, 0.0, 1.0)))
    two = dict(zip(formats.FRAME_METRIC_NAMES, (0.25, 0.2, 0.0, 0.0, 0.0, 0.0)))
    line = launcher.mean_frame_metrics([{"frame_metrics": {0: one}}, {"frame_metrics": {3: two}}, {"frame_metrics": {}}])
    assert line["frame_metrics_frames"] == 2 and line["frame_metrics"]["iou_3d"] == 0.375 and line["frame_metrics"]["accuracy_bev_50"] == 0.5
    assert launcher.mean_frame_metrics([{}]) == {"frame_metrics": {}, "frame_metrics_frames": 0}


def test_launcher_metrics_not_with_selftest():
    env = dict(os.environ, PYTHONPATH=ROOT)
    done = subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", "1", "--metrics", "--selftest"],
                          capture_output=True, text=True, cwd=ROOT, env=env)
    assert done.returncode != 0 and "--metrics evaluates the boxes of optimised frames" in done.stderr and "drop one of --selftest, --metrics" in done.stderr


def test_ground_truth_shapes_are_checked_before_a_loop_writes_anything():
    """optimization._check_ground_truth, which reset() calls before it overwrites the row: FrameInputs and packs alike."""
    import dataclasses
    from vsrd_amd import optimization
    inputs = optimization.FrameInputs((2, 2), None, None, None, None, None, boxes_3d=torch.zeros(3, 8, 3), rectification_matrix=torch.eye(3))
    optimization._check_ground_truth(inputs, 3)
    optimization._check_ground_truth(optimization.FrameInputs((2, 2), None, None, None, None, None), 3)
    optimization._check_ground_truth(_pack(), 2)
    with pytest.raises(ValueError, match="boxes_3d"):
        optimization._check_ground_truth(inputs, 4)
    with pytest.raises(ValueError, match="rectification_matrix"):
        optimization._check_ground_truth(dataclasses.replace(inputs, rectification_matrix=torch.eye(4)), 3)
    with pytest.raises(ValueError, match="boxes_3d"):
        optimization._check_ground_truth(dataclasses.replace(_pack(), boxes_3d=np.zeros((2, 24), dtype=np.float32)), 2)


def test_the_symbol_is_declared_inside_abi_12():
    from vsrd_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"^#define VSRD_ABI_VERSION 12$", header, flags=re.M) and _lib.ABI_VERSION == 12
    assert re.search(r"^int32_t\s+vsrd_frame_metrics\s*\(", header, flags=re.M)
    block = header[header.index("/* Frame metrics"):header.index("int32_t vsrd_frame_metrics")]
    assert "added within ABI 12; probe for the symbol" in block
    restype, argtypes = _lib.SIGNATURES["vsrd_frame_metrics"]
    assert restype is ctypes.c_int32 and len(argtypes) == 13 and argtypes[0] == ctypes.POINTER(_lib.FrameConfig)
    prototype = header[header.index("int32_t vsrd_frame_metrics"):]
    prototype = re.sub(r"/\*.*?\*/", "", prototype[:prototype.index(";")], flags=re.S)
    assert len(prototype.split(",")) == 13
