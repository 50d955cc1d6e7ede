"""vsrd_amd.launcher --predictions: every optimised frame leaves its pseudo-labels next to its checkpoint (predictions/view_VV.json for
every view, labels/view_00.txt for the target view), written BEFORE the checkpoint that marks the frame as done -- the small mixed job of
test_launcher_mixed.py, once in a FrameBatch (one vsrd_frame_labels call per group) and once frame by frame (frame slots and loops of
their own), each in a fresh child process."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS, COUNTS, FRAMES = 3, [2, 3, 4], 6
SMALL = ["--views", str(VIEWS), "--height", "128", "--width", "128", "--rays", "128", "--samples", "40", "--num-steps", "12", "--warmup-steps", "5",
         "--adjoint-item-slots", "8"]


def _run(tmp, name, frame_batch, extra=()):
    out = os.path.join(tmp, name)
    cmd = [sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", str(FRAMES), "--instances", ",".join(map(str, COUNTS)),
           "--frame-batch", str(frame_batch), "--queue", "static", "--out", out, *SMALL, *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert done.returncode == 0, done.stderr[-4000:]
    line = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
    return out, line


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    import __graft_entry__
    __graft_entry__.build()
    tmp = str(tmp_path_factory.mktemp("predictions"))
    return {"batched": _run(tmp, "b4", 4, ["--predictions"]), "alone": _run(tmp, "b1", 1, ["--predictions"])}


def _frame_files(out, frame):
    folder = os.path.join(out, f"frame_{frame:06d}")
    return sorted(os.path.relpath(os.path.join(base, name), folder) for base, _, names in os.walk(folder) for name in names)


def _prediction(out, frame, view):
    with open(os.path.join(out, f"frame_{frame:06d}", "predictions", f"view_{view:02d}.json")) as file:
        return json.load(file)


@pytest.mark.parametrize("job", ["batched", "alone"])
def test_every_frame_has_its_checkpoint_and_its_labels(jobs, job):
    from vsrd_amd import launcher
    out, line = jobs[job]
    assert line["frames"] == FRAMES and line["predictions"] is True
    assert all(clock["labels"] > 0.0 and clock["labels_write"] > 0.0 for clock in line["phase_seconds"])
    assert len(glob.glob(os.path.join(out, "frame_*"))) == FRAMES
    expected = sorted([os.path.join("labels", "view_00.txt"), "step_11.pt", *[os.path.join("predictions", f"view_{v:02d}.json") for v in range(VIEWS)]])
    for frame in range(FRAMES):
        assert _frame_files(out, frame) == expected, frame
        n = launcher.instances_of(frame, COUNTS)
        confidences = _prediction(out, frame, 0)["confidences"]["car"]
        for view in range(VIEWS):
            record = _prediction(out, frame, view)
            assert list(record) == ["boxes_3d", "boxes_2d", "confidences"]
            assert torch.tensor(record["boxes_3d"]["car"]).shape == (n, 8, 3) and torch.tensor(record["boxes_2d"]["car"]).shape == (n, 2, 2)
            assert record["confidences"]["car"] == confidences and len(confidences) == n        # the same confidences in every view's file
        assert all(0.0 <= c <= 1.0 + 1e-6 for c in confidences)
        with open(os.path.join(out, f"frame_{frame:06d}", "labels", "view_00.txt")) as file:
            lines = file.readlines()
        assert len(lines) == n and all(text.startswith("Car ") and text.split()[-1] == str(c) for text, c in zip(lines, confidences))


def test_a_frame_has_the_same_labels_in_a_batch_and_alone(jobs):
    """(The checkpoint tensors already are identical: test_launcher_mixed.py.)"""
    for frame in range(FRAMES):
        for view in range(VIEWS):
            a, b = _prediction(jobs["batched"][0], frame, view), _prediction(jobs["alone"][0], frame, view)
            assert a["confidences"] == b["confidences"] and a["boxes_2d"] == b["boxes_2d"], (frame, view)


def test_confidences_are_the_reference_chain_on_the_written_boxes(jobs):
    """formats.multi_view_confidences (make_predictions.py:86-176, golden g12_formats) on the JSONs' own 2-D boxes and the frame's own
    ground truth reproduces the JSON's confidences within (V + 16) 2^-24 -- one float32 IoU is about ten roundings, the mean over at most V
    views adds V half-spacings -- with every prediction matched: the confidence of prediction p is the mean IoU of ITS pair."""
    from vsrd_amd import formats, launcher
    dev = torch.device("cuda:0")
    frame = 1
    n = launcher.instances_of(frame, COUNTS)
    inputs = launcher.synthetic_frame_inputs(dev, frame, VIEWS, n, height=128, width=128)
    assert bool(inputs.visible_masks.all())
    out = jobs["batched"][0]
    pd = [torch.tensor(_prediction(out, frame, view)["boxes_2d"]["car"], dtype=torch.float32) for view in range(VIEWS)]
    gt = [inputs.boxes_2d[view].cpu().float() for view in range(VIEWS)]
    confidences, pd_idx, gt_idx = formats.multi_view_confidences(pd, gt, [torch.arange(n)] * VIEWS)
    assert pd_idx.tolist() == list(range(n)) and sorted(gt_idx.tolist()) == list(range(n))
    written = torch.tensor(_prediction(out, frame, 0)["confidences"]["car"], dtype=torch.float64)
    bound = (VIEWS + 16) * 2.0 ** -24
    observed = float((written - confidences.double()).abs().max())
    print(f"confidences: |written - reference chain| = {observed:.3e} (bound {bound:.3e}); written {written.tolist()}")
    assert observed <= bound


def test_without_the_flag_nothing_changes(jobs, tmp_path):
    out, line = _run(str(tmp_path), "plain", 4)
    assert line["frames"] == FRAMES and "predictions" not in line
    assert all("labels" not in clock and "labels_write" not in clock for clock in line["phase_seconds"])
    for frame in range(FRAMES):
        assert _frame_files(out, frame) == ["step_11.pt"], frame
    a = torch.load(os.path.join(out, "frame_000001", "step_11.pt"), map_location="cpu")
    b = torch.load(os.path.join(jobs["batched"][0], "frame_000001", "step_11.pt"), map_location="cpu")
    for key, value in a["models"]["detector"].items():             # and the labels pass does not touch what is optimised
        assert torch.equal(value, b["models"]["detector"][key]), key
