"""vsrd_amd.launcher --scalar-interval / --ckpt-interval / --select: every optimised frame leaves history.json, its step_*.pt snapshots and
model.pt next to its final checkpoint, all written BEFORE that checkpoint -- a job of two frames in one FrameBatch at a tiny shape, in a
fresh child process, and a second run of it that finds both frames done."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 12
SMALL = ["--views", "2", "--instances", "2", "--height", "32", "--width", "64", "--rays", "64", "--samples", "40", "--num-steps", str(STEPS), "--warmup-steps", "6",
         "--adjoint-item-slots", "8"]
FLAGS = ["--metrics", "--scalar-interval", "3", "--ckpt-interval", "4", "--select", "iou_3d:max"]


def _run(out):
    cmd = [sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", "2", "--frame-batch", "2", "--queue", "static", "--max-restarts", "0", "--out", out,
           *SMALL, *FLAGS]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert done.returncode == 0, done.stderr[-4000:]
    return json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    import __graft_entry__
    __graft_entry__.build()
    out = str(tmp_path_factory.mktemp("log") / "out")
    return out, _run(out)


def test_every_frame_has_its_history_its_snapshots_and_its_model(job):
    out, line = job
    assert line["frames"] == 2 and line["frame_log"] == dict(scalar_interval=3, ckpt_interval=4, select="iou_3d:max")
    assert all(clock["log"] > 0.0 and clock["log_write"] > 0.0 for clock in line["phase_seconds"])
    for frame in range(2):
        folder = os.path.join(out, f"frame_{frame:06d}")
        assert sorted(os.listdir(folder)) == sorted(["history.json", "model.pt", "step_3.pt", "step_7.pt", f"step_{STEPS - 1}.pt"]), frame
        history = json.load(open(os.path.join(folder, "history.json")))
        assert len(history) == STEPS // 3 and [record["step"] for record in history] == [2, 5, 8, 11]
        assert ["losses/eikonal_loss" in record for record in history] == [False, False, True, True]
        assert all("metrics/iou_3d" in record and "learning_rates/hyper_distance_field" in record and "hyperparameters/cosine_ratio" in record for record in history)
        checkpoints = {step: torch.load(os.path.join(folder, f"step_{step}.pt"), map_location="cpu", weights_only=False) for step in (3, 7, STEPS - 1)}
        for step, checkpoint in checkpoints.items():
            assert checkpoint["step"] == step and set(checkpoint["models"]) == {"detector", "hyper_distance_field"} and "iou_3d" in checkpoint["metrics"]
        assert set(checkpoints[3]) == {"step", "models", "metrics"} and "optimizer" in checkpoints[STEPS - 1]          # (the final checkpoint is present, and complete)
        assert checkpoints[STEPS - 1]["metrics"]["iou_3d"] == history[-1]["metrics/iou_3d"]
        # model.pt: the step_*.pt whose stored iou_3d is largest, the earliest on a tie -- byte for byte
        best = max(sorted(checkpoints), key=lambda step: (checkpoints[step]["metrics"]["iou_3d"], -step))
        assert open(os.path.join(folder, "model.pt"), "rb").read() == open(os.path.join(folder, f"step_{best}.pt"), "rb").read(), (frame, best)
        assert not torch.equal(checkpoints[3]["models"]["detector"]["locations"], checkpoints[7]["models"]["detector"]["locations"])


def _stamps(out):
    return {(folder, name): os.path.getmtime(os.path.join(out, folder, name)) for folder in sorted(os.listdir(out)) if folder.startswith("frame_")
            for name in os.listdir(os.path.join(out, folder))}


def test_a_second_run_skips_both_frames(job):
    out, _ = job
    stamps = _stamps(out)
    line = _run(out)
    assert line["frames"] == 0 and line["frames_skipped_as_done"] == 2
    assert len(stamps) == 10 and _stamps(out) == stamps
