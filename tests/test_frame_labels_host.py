"""The host side of the per-frame pseudo-labels: formats.save_frame_labels (what FrameOptimizer.labels() returns, as the reference's prediction
JSONs and KITTI label lines) and the launcher's refusal of --predictions with --selftest."""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _labels(seed):
    g = torch.Generator().manual_seed(seed)
    V, n = 2, 3
    centres = torch.randn(V, n, 1, 3, generator=g) + torch.tensor([0.0, 1.0, 20.0])
    boxes_3d = centres + torch.randn(V, n, 8, 3, generator=g)
    corner = 300.0 * torch.rand(V, n, 1, 2, generator=g)
    boxes_2d = torch.cat([corner, corner + 50.0 * torch.rand(V, n, 1, 2, generator=g)], dim=-2)
    return dict(boxes_3d=boxes_3d, boxes_2d=boxes_2d, confidences=torch.rand(n, generator=g), matched_gt=torch.tensor([2, 0, 1]),
                mean_iou=torch.rand(n, n, generator=g))


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(base, name), folder) for base, _, names in os.walk(folder) for name in names)


def test_save_frame_labels_writes_the_reference_files(tmp_path):
    from vsrd_amd import formats
    folder = str(tmp_path / "frame_000003")
    expected_files = [os.path.join("labels", "view_00.txt"), os.path.join("predictions", "view_00.json"), os.path.join("predictions", "view_01.json")]
    for seed in (1, 2):                                            # the second call replaces the files of the first
        labels = _labels(seed)
        formats.save_frame_labels(folder, labels)
        assert _tree(folder) == expected_files                     # exactly these: no temporary file stays behind
        for view in range(2):
            with open(os.path.join(folder, "predictions", f"view_{view:02d}.json")) as file:
                record = json.load(file)
            assert list(record) == ["boxes_3d", "boxes_2d", "confidences"] and all(list(value) == ["car"] for value in record.values())
            assert record == formats.prediction_record(labels["boxes_3d"][view], labels["boxes_2d"][view], labels["confidences"])
        with open(os.path.join(folder, "labels", "view_00.txt")) as file:
            lines = file.readlines()
        scores = labels["confidences"].tolist()
        assert lines == [formats.kitti_label_line("car", labels["boxes_3d"][0][k], labels["boxes_2d"][0][k], scores[k]) for k in range(3)]
        assert all(line.startswith("Car ") and line.endswith(f" {scores[k]}\n") for k, line in enumerate(lines))


def test_save_frame_labels_removes_what_a_killed_writer_left(tmp_path):
    from vsrd_amd import formats
    folder = str(tmp_path / "frame_000000")
    os.makedirs(os.path.join(folder, "predictions"))
    stale = os.path.join(folder, "predictions", "view_01.json.tmp.12345")
    open(stale, "w").write("{")
    formats.save_frame_labels(folder, _labels(3), class_name="van")
    assert not os.path.exists(stale) and len(_tree(folder)) == 3
    with open(os.path.join(folder, "predictions", "view_01.json")) as file:
        assert list(json.load(file)["confidences"]) == ["van"]


def test_launcher_refuses_predictions_with_selftest(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    done = subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", "--selftest", "--predictions", "--gpus", "1", "--frames", "2", "--out", str(tmp_path / "out")],
                          cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert done.returncode != 0
    assert "--selftest" in done.stderr and "--predictions" in done.stderr
    assert not os.path.exists(str(tmp_path / "out"))
