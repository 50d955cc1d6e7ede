"""vsrd_amd.launcher --group-predictions: every optimised frame leaves its pseudo-labels in the frames of its GROUP next to its checkpoint
(group/predictions/<id>.json and group/labels/<id>.txt for every group frame), written BEFORE the checkpoint that marks the frame as done --
the small mixed job of test_launcher_predictions.py with --label-views 5, in a FrameBatch (one vsrd_frame_group_labels call per group of
frames), in a fresh child process."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS, COUNTS, FRAMES, LABEL_VIEWS = 3, [2, 3, 4], 6, 5
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
    tmp = str(tmp_path_factory.mktemp("group_predictions"))
    return {"group": _run(tmp, "group", 4, ["--label-views", str(LABEL_VIEWS), "--group-predictions"]), "plain": _run(tmp, "plain", 4)}


def _frame_files(out, frame):
    folder = os.path.join(out, f"frame_{frame:06d}")
    return sorted(os.path.relpath(os.path.join(base, name), folder) for base, _, names in os.walk(folder) for name in names)


def _ids(frame):
    return [frame * 10000 + view for view in range(LABEL_VIEWS)]              # (synthetic.synthetic_group)


def _prediction(out, frame, frame_id):
    with open(os.path.join(out, f"frame_{frame:06d}", "group", "predictions", f"{frame_id:010d}.json")) as file:
        return json.load(file)


def test_every_frame_has_five_jsons_and_five_txts_before_its_checkpoint(jobs):
    from vsrd_amd import launcher
    out, line = jobs["group"]
    assert line["frames"] == FRAMES and line["group_predictions"] is True and "predictions" not in line
    assert all(clock["group_labels"] > 0.0 and clock["group_labels_write"] > 0.0 and "labels" not in clock for clock in line["phase_seconds"])
    assert len(glob.glob(os.path.join(out, "frame_*"))) == FRAMES
    for frame in range(FRAMES):
        expected = sorted(["step_11.pt", *[os.path.join("group", kind, f"{i:010d}.{suffix}") for i in _ids(frame)
                                           for kind, suffix in (("predictions", "json"), ("labels", "txt"))]])
        assert _frame_files(out, frame) == expected, frame
        folder = os.path.join(out, f"frame_{frame:06d}")
        written = max(os.path.getmtime(os.path.join(folder, name)) for name in expected if name != "step_11.pt")
        assert written <= os.path.getmtime(os.path.join(folder, "step_11.pt")), frame            # the checkpoint marks the frame as done: last
        n = launcher.instances_of(frame, COUNTS)
        confidences = _prediction(out, frame, _ids(frame)[0])["confidences"]["car"]
        for frame_id in _ids(frame):
            record = _prediction(out, frame, frame_id)
            assert list(record) == ["boxes_3d", "boxes_2d", "confidences"]
            assert torch.tensor(record["boxes_3d"]["car"]).shape == (n, 8, 3) and torch.tensor(record["boxes_2d"]["car"]).shape == (n, 2, 2)
            assert record["confidences"]["car"] == confidences and len(confidences) == n       # the same confidences in every group frame's file
            with open(os.path.join(folder, "group", "labels", f"{frame_id:010d}.txt")) as file:
                lines = file.readlines()
            assert len(lines) == n and all(text.startswith("Car ") and text.split()[-1] == str(c) for text, c in zip(lines, confidences))
        assert all(0.0 <= c <= 1.0 + 1e-6 for c in confidences)


def test_confidences_are_the_reference_chain_on_the_written_boxes(jobs):
    """formats.multi_view_confidences (make_predictions.py:86-176) on the JSONs' own 2-D boxes and the frame's own label boxes reproduces the
    JSONs' confidences within (L + 16) 2^-24 -- the bound of test_launcher_predictions.py with the group's L views: one float32 IoU is about
    ten roundings, the mean over at most L views adds L half-spacings.  A view contributes the slots it sees (gt_to_target = -1 elsewhere)."""
    from vsrd_amd import formats, launcher
    dev = torch.device("cuda:0")
    frame = 1
    n = launcher.instances_of(frame, COUNTS)
    inputs = launcher.synthetic_frame_inputs(dev, frame, VIEWS, n, height=128, width=128, label_views=LABEL_VIEWS)
    assert inputs.label_frame_ids.tolist() == _ids(frame)
    visible = inputs.label_visible.cpu().bool()
    assert bool(visible.any(dim=0).all())                           # every slot is seen by some group frame: the chain divides by no zero
    out = jobs["group"][0]
    pd = [torch.tensor(_prediction(out, frame, frame_id)["boxes_2d"]["car"], dtype=torch.float32) for frame_id in _ids(frame)]
    gt = [inputs.label_boxes_2d[view].cpu().float().unflatten(-1, (2, 2)) for view in range(LABEL_VIEWS)]
    table = [torch.where(visible[view], torch.arange(n), torch.full((n,), -1)) for view in range(LABEL_VIEWS)]
    confidences, pd_idx, gt_idx = formats.multi_view_confidences(pd, gt, table)
    assert pd_idx.tolist() == list(range(n)) and sorted(gt_idx.tolist()) == list(range(n))
    written = torch.tensor(_prediction(out, frame, _ids(frame)[0])["confidences"]["car"], dtype=torch.float64)
    bound = (LABEL_VIEWS + 16) * 2.0 ** -24
    observed = float((written - confidences.double()).abs().max())
    print(f"confidences: |written - reference chain| = {observed:.3e} (bound {bound:.3e}); written {written.tolist()}")
    assert observed <= bound


def test_without_the_flag_nothing_changes(jobs):
    out, line = jobs["plain"]
    assert line["frames"] == FRAMES and "group_predictions" not in line
    assert all("group_labels" not in clock and "group_labels_write" not in clock for clock in line["phase_seconds"])
    for frame in range(FRAMES):
        assert _frame_files(out, frame) == ["step_11.pt"], frame
    a = torch.load(os.path.join(out, "frame_000001", "step_11.pt"), map_location="cpu")
    b = torch.load(os.path.join(jobs["group"][0], "frame_000001", "step_11.pt"), map_location="cpu")
    for key, value in a["models"]["detector"].items():             # and the group's labels do not touch what is optimised
        assert torch.equal(value, b["models"]["detector"][key]), key
