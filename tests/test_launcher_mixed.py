"""vsrd_amd.launcher --instances as a comma list: frame j gets list[j % len(list)] instances (a pure function of the frame number), a mixed
list with --frame-batch > 1 runs in FrameBatch(max_instances=max(list)) and reports the mix."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_instances_parse_and_frame_to_count():
    from vsrd_amd import launcher
    assert launcher.parse_instances("8") == [8]
    assert launcher.parse_instances("3,8,13") == [3, 8, 13]
    for bad in ("0", "65", "3,,4", "a"):
        with pytest.raises(SystemExit):
            launcher.parse_instances(bad)
    counts = [2, 3, 4]
    # a pure function of the frame number: any rank, any order, any restart gives the same count
    assert [launcher.instances_of(j, counts) for j in range(7)] == [2, 3, 4, 2, 3, 4, 2]
    assert [launcher.instances_of(j, counts) for j in reversed(range(7))] == [2, 4, 3, 2, 4, 3, 2]
    assert all(launcher.instances_of(j, [8]) == 8 for j in range(5))


SMALL = ["--views", "3", "--height", "128", "--width", "128", "--rays", "128", "--samples", "40", "--num-steps", "12", "--warmup-steps", "5",
         "--adjoint-item-slots", "8"]


def _run(tmp, frame_batch, extra=()):
    out = os.path.join(tmp, f"b{frame_batch}")
    cmd = [sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", "6", "--instances", "2,3,4", "--frame-batch", str(frame_batch),
           "--queue", "static", "--out", out, *SMALL, *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert done.returncode == 0, done.stderr[-4000:]
    line = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
    return out, line


@pytest.mark.gpu
def test_mixed_job_in_a_batch_matches_frames_alone(tmp_path):
    import __graft_entry__
    __graft_entry__.build()
    out, line = _run(str(tmp_path), 4)
    assert line["frames"] == 6 and line["instance_list"] == [2, 3, 4] and line["batch_capacity"] == 4
    assert line["frames_per_instances"] == {"2": 2, "3": 2, "4": 2} and line["frame_batch"] == 4
    files = sorted(glob.glob(os.path.join(out, "frame_*", "*.pt")))
    assert len(files) == 6
    from vsrd_amd import launcher
    for path in files:
        frame = int(os.path.basename(os.path.dirname(path)).split("_")[1])
        payload = torch.load(path, map_location="cpu")
        assert payload["models"]["detector"]["locations"].shape == (1, launcher.instances_of(frame, [2, 3, 4]), 3)
    alone_out, alone = _run(str(tmp_path), 1)
    assert alone["batch_capacity"] is None and alone["frames"] == 6
    one = os.path.relpath(files[1], out)
    a, b = torch.load(os.path.join(out, one), map_location="cpu"), torch.load(os.path.join(alone_out, one), map_location="cpu")
    for name in ("detector", "hyper_distance_field"):
        for key, value in a["models"][name].items():
            assert torch.equal(value, b["models"][name][key]), (name, key)
