"""vsrd_amd.launcher --views as a comma list and --frames-dir over packs of different view counts: frame j gets list[j % len(list)] views
(a pure function of the frame number, independent of the --instances list's cycle), a mixed list with --frame-batch > 1 runs in
FrameBatch(max_views=max(list)), a directory may mix view counts (not image sizes), and the line reports the mix.  With them the layout of
the grown vsrd_frame_header (ABI 12)."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _environment():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_views_parse_and_frame_to_views():
    from vsrd_amd import launcher
    assert launcher.parse_views("17") == [17]
    assert launcher.parse_views("9,13,17") == [9, 13, 17]
    for bad in ("0", "33", "3,,4", "a", ""):
        with pytest.raises(SystemExit):
            launcher.parse_views(bad)
    views, counts = [2, 3], [2, 3, 4]
    # a pure function of the frame number, and each list cycles with its own length: six frames meet all six (views, instances) pairs
    assert [launcher.views_of(j, views) for j in range(7)] == [2, 3, 2, 3, 2, 3, 2]
    assert [launcher.views_of(j, views) for j in reversed(range(7))] == [2, 3, 2, 3, 2, 3, 2]
    pairs = [(launcher.views_of(j, views), launcher.instances_of(j, counts)) for j in range(6)]
    assert pairs == [(2, 2), (3, 3), (2, 4), (3, 2), (2, 3), (3, 4)] and len(set(pairs)) == 6
    assert all(launcher.views_of(j, [17]) == 17 for j in range(5))


def test_abi_version_is_12():
    from vsrd_amd import _lib
    header = open(os.path.join(ROOT, "include", "vsrd_hip.h")).read()
    assert _lib.ABI_VERSION == 12 and "#define VSRD_ABI_VERSION 12" in header


def test_frame_header_layout_matches_the_c_struct():
    """The grown vsrd_frame_header as literals (against gcc's view of the header, member by member: tests/test_host_logic.py::
    test_struct_matches_the_header[FrameHeader]; the flag against its #define: test_constants_match_the_header)."""
    from vsrd_amd import _lib
    names = [name for name, _ in _lib.FrameHeader._fields_]
    assert names == ["num_instances", "loss_scale", "num_views", "reserved", "num_pixels"]
    assert ctypes.sizeof(_lib.FrameHeader) == 24
    header = open(os.path.join(ROOT, "include", "vsrd_hip.h")).read()
    assert _lib.FRAME_HEADER_HAS_VIEWS == 0x10000 and "#define VSRD_FRAME_HEADER_HAS_VIEWS 0x10000 " in header
    assert (_lib.FrameHeader.num_instances.offset, _lib.FrameHeader.loss_scale.offset) == (0, 4)          # the ABI-9 header is its first 8 bytes


@pytest.fixture(scope="module")
def mixed_dir(tmp_path_factory):
    """Six small packs with 1, 2, 3, 1, 2, 3 views and 2, 3, 2, 3, 2, 3 instances at 32 x 48."""
    import make_frame_packs
    folder = str(tmp_path_factory.mktemp("packs_of_mixed_views"))
    paths = make_frame_packs.write_packs(folder, 6, views=[1, 2, 3], height=32, width=48, instances=[2, 3])
    return folder, paths


def test_make_frame_packs_cycles_a_list_of_views(mixed_dir, tmp_path):
    import make_frame_packs
    from vsrd_amd import frames
    _, paths = mixed_dir
    assert [frames.pack_counts(path) for path in paths] == [(1, 32, 48, 2), (2, 32, 48, 3), (3, 32, 48, 2), (1, 32, 48, 3), (2, 32, 48, 2), (3, 32, 48, 3)]
    # an integer as before, and the command line's list
    assert [frames.pack_counts(path)[0] for path in make_frame_packs.write_packs(str(tmp_path / "uniform"), 2, views=2, height=32, width=48, instances=[2])] == [2, 2]
    assert make_frame_packs.main(["--out", str(tmp_path / "cli"), "--count", "3", "--views", "2,1", "--height", "32", "--width", "48", "--instances", "2"]) == 0
    assert [frames.pack_counts(path)[0] for path in sorted(glob.glob(str(tmp_path / "cli" / "*.npz")))] == [2, 1, 2]


def test_scan_frames_dir_takes_packs_of_different_view_counts(mixed_dir, tmp_path):
    import make_frame_packs
    import shutil
    from vsrd_amd import launcher
    folder, paths = mixed_dir
    files, shapes = launcher.scan_frames_dir(folder)
    assert files == sorted(paths)
    assert shapes == [(1, 32, 48, 2), (2, 32, 48, 3), (3, 32, 48, 2), (1, 32, 48, 3), (2, 32, 48, 2), (3, 32, 48, 3)]
    # another image size is still refused, and the message names the file
    odd = tmp_path / "odd"
    shutil.copytree(folder, odd)
    pack = make_frame_packs.make_pack(9, 2, 32, 56, 2)
    from vsrd_amd import frames
    frames.save_pack(str(odd / "frame_000009.npz"), pack)
    with pytest.raises(SystemExit) as refusal:
        launcher.scan_frames_dir(str(odd))
    assert "frame_000009.npz" in str(refusal.value) and "image size" in str(refusal.value)


def test_selftest_over_a_directory_of_mixed_views(mixed_dir, tmp_path):
    folder, paths = mixed_dir
    out = subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", "--selftest", "--gpus", "2", "--frames-dir", folder, "--selftest-seconds", "0.05",
                          "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, env=_environment(), cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")][-1]
    assert line["frames"] == 6 and line["frames_per_views"] == {"1": 2, "2": 2, "3": 2} and line["frames_per_instances"] == {"2": 3, "3": 3}
    completed = [int(row.split()[0]) for row in open(tmp_path / "out" / "completed.log").read().splitlines()]
    assert sorted(completed) == list(range(len(paths)))               # every file exactly once


# ---- on the GPU: a job of mixed views in a batch and frame by frame ---------------------------------------------------------------------------

VIEWS, COUNTS, FRAMES = [2, 3], [2, 3, 4], 6
SMALL = ["--height", "128", "--width", "128", "--rays", "128", "--samples", "40", "--num-steps", "12", "--warmup-steps", "5", "--adjoint-item-slots", "8"]


def _run(tmp, frame_batch):
    out = os.path.join(tmp, f"b{frame_batch}")
    cmd = [sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", str(FRAMES), "--views", ",".join(map(str, VIEWS)),
           "--instances", ",".join(map(str, COUNTS)), "--frame-batch", str(frame_batch), "--queue", "static", "--out", out, "--predictions", *SMALL]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=_environment())
    assert done.returncode == 0, done.stderr[-4000:]
    return out, json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_job_of_mixed_views_in_a_batch_matches_frames_alone(tmp_path):
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import launcher
    out, line = _run(str(tmp_path), 3)
    assert line["frames"] == FRAMES and line["frame_batch"] == 3
    assert line["view_list"] == VIEWS and line["batch_view_capacity"] == 3 and line["frames_per_views"] == {"2": 3, "3": 3}
    assert line["instance_list"] == COUNTS and line["batch_capacity"] == 4 and line["frames_per_instances"] == {"2": 2, "3": 2, "4": 2}
    assert "2,3 views" in line["metric"] and line["frames_outside_slots"] == []
    alone_out, alone = _run(str(tmp_path), 1)
    assert alone["frames"] == FRAMES and alone["batch_view_capacity"] is None and alone["frames_per_views"] == {"2": 3, "3": 3}
    for frame in range(FRAMES):
        views, n = launcher.views_of(frame, VIEWS), launcher.instances_of(frame, COUNTS)
        one = os.path.join(f"frame_{frame:06d}", "step_11.pt")
        a, b = torch.load(os.path.join(out, one), map_location="cpu"), torch.load(os.path.join(alone_out, one), map_location="cpu")
        assert a["models"]["detector"]["locations"].shape == (1, n, 3)
        for name in ("detector", "hyper_distance_field"):
            for key, value in a["models"][name].items():
                assert torch.equal(value, b["models"][name][key]), (frame, name, key)
        # --predictions: one file per view of the frame's OWN views, the same in both runs
        for folder in (out, alone_out):
            written = sorted(os.path.basename(p) for p in glob.glob(os.path.join(folder, f"frame_{frame:06d}", "predictions", "*.json")))
            assert written == [f"view_{v:02d}.json" for v in range(views)], (frame, written)
        for view in range(views):
            records = [json.load(open(os.path.join(folder, f"frame_{frame:06d}", "predictions", f"view_{view:02d}.json"))) for folder in (out, alone_out)]
            assert records[0] == records[1], (frame, view)
            assert torch.tensor(records[0]["boxes_3d"]["car"]).shape == (n, 8, 3)
