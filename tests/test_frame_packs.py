"""Frame packs (vsrd_amd/frames.py), host side: the file format, its validation, the re-indexing tables, and the launcher's --frames-dir on
the GPU-free selftest path.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _pack(height=20, width=27):
    """V = 3, N = 3: view 1 lacks instance 22, view 2 lists (33, 11, 77, 22) -- another order and an id the target does not have."""
    from vsrd_amd import frames
    rng = np.random.default_rng(4)
    ids = [11, 22, 33, 11, 33, 33, 11, 77, 22]
    counts = [4, 1, 2, 5, 3, 7, 2, 4, 6]
    vertices = np.stack([rng.integers(0, width, sum(counts)), rng.integers(0, height, sum(counts))], -1).astype(np.int32)
    inside = np.packbits(rng.random((len(ids), height, width)) < 0.3, axis=-1)
    intrinsics = rng.random((3, 3, 3)).astype(np.float32)
    extrinsics = rng.random((3, 4, 4)).astype(np.float32)
    return frames.FramePack((height, width), intrinsics, extrinsics, np.array([0, 3, 5, 9]), np.array(ids), np.concatenate([[0], np.cumsum(counts)]),
                            vertices, inside)


def test_save_then_load_is_bit_identical(tmp_path):
    from vsrd_amd import frames
    pack = _pack()
    path = str(tmp_path / "frame.npz")
    frames.save_pack(path, pack)
    assert os.listdir(tmp_path) == ["frame.npz"]                       # (nothing staged is left behind)
    loaded = frames.load_pack(path)
    assert tuple(loaded.image_size) == (20, 27) and loaded.num_views == 3 and loaded.num_instances == 3
    for field, dtype in (("intrinsic_matrices", np.float32), ("extrinsic_matrices", np.float32), ("view_offsets", np.int64), ("instance_ids", np.int64),
                         ("polygon_offsets", np.int64), ("polygon_vertices", np.int32), ("inside", np.uint8)):
        got, want = getattr(loaded, field), np.asarray(getattr(pack, field))
        assert got.dtype == dtype and got.shape == want.shape and got.tobytes() == want.astype(dtype).tobytes(), field
    assert loaded.inside.shape == (9, 20, 4)
    assert frames.pack_counts(path) == (3, 20, 27, 3)


def test_collate_tables_restate_the_reference_reindexing():
    """scripts/main.py:204-255: per source view, the index of each target instance id among the view's ids, -1 where it is absent."""
    from vsrd_amd import frames
    pack = _pack()
    offsets, ids = pack.view_offsets, pack.instance_ids
    target = list(ids[offsets[0]:offsets[1]])
    expected = []
    for view in range(3):
        own = list(ids[offsets[view]:offsets[view + 1]])
        expected.append([offsets[view] + own.index(instance) if instance in own else -1 for instance in target])
    table = frames.collate_tables(pack)
    assert table.dtype == np.int32 and table.tolist() == expected == [[0, 1, 2], [3, -1, 4], [6, 8, 5]]


def _arrays(pack):
    from vsrd_amd import frames
    return {field: np.asarray(getattr(pack, field)) for field in frames._FIELDS}


@pytest.mark.parametrize("case", ["truncated_offsets", "duplicate_id", "empty_polygon", "object_array", "too_many_views", "not_an_archive"])
def test_malformed_files_raise_and_name_the_file(tmp_path, case):
    from vsrd_amd import frames
    arrays = _arrays(_pack())
    path = str(tmp_path / f"{case}.npz")
    if case == "truncated_offsets":
        arrays["polygon_offsets"] = arrays["polygon_offsets"][:-1]
    elif case == "duplicate_id":
        arrays["instance_ids"] = arrays["instance_ids"].copy()
        arrays["instance_ids"][8] = 33                                  # view 2 then lists 33 twice
    elif case == "empty_polygon":
        arrays["polygon_offsets"] = arrays["polygon_offsets"].copy()
        arrays["polygon_offsets"][2] = arrays["polygon_offsets"][1]     # P = 0 for entry 1
    elif case == "object_array":
        arrays["instance_ids"] = np.array([{"id": k} for k in range(9)], dtype=object)
    elif case == "too_many_views":
        arrays["view_offsets"] = np.concatenate([arrays["view_offsets"], np.full(40, 9)])
    if case == "not_an_archive":
        open(path, "wb").write(b"no zip here")
    else:
        with open(path, "wb") as handle:
            np.savez(handle, **arrays)
    with pytest.raises(ValueError) as error:
        frames.load_pack(path)
    assert path in str(error.value)
    if case == "object_array":                                          # (refused, never unpickled)
        assert "pickle" in str(error.value)


def test_save_refuses_a_malformed_pack(tmp_path):
    from vsrd_amd import frames
    pack = _pack()
    pack.polygon_offsets = pack.polygon_offsets[:-1]
    with pytest.raises(ValueError):
        frames.save_pack(str(tmp_path / "bad.npz"), pack)
    assert os.listdir(tmp_path) == []


def test_make_frame_packs_drop_and_shuffle(tmp_path):
    """tools/make_frame_packs.py: --drop takes a target instance out of a source view, --shuffle reorders the source views' entries; the table
    still finds every remaining instance, and every entry has a polygon and at least one set bit."""
    import make_frame_packs
    from vsrd_amd import frames
    paths = make_frame_packs.write_packs(str(tmp_path), 2, views=3, height=32, width=48, instances=[4, 3], drop=[(1, 0), (2, 1)], shuffle=True)
    assert [os.path.basename(p) for p in paths] == ["frame_000000.npz", "frame_000001.npz"]
    assert [frames.pack_counts(p) for p in paths] == [(3, 32, 48, 4), (3, 32, 48, 3)]
    pack = frames.load_pack(paths[0])
    table = frames.collate_tables(pack)
    assert table[0].tolist() == [0, 1, 2, 3] and table[1, 0] == -1 and table[2, 1] == -1
    assert (table >= 0).sum() == 10 == len(pack.instance_ids)
    for view in range(3):
        for slot in range(4):
            if table[view, slot] >= 0:
                assert pack.instance_ids[table[view, slot]] == pack.instance_ids[slot]
    assert bool(np.unpackbits(pack.inside, axis=-1)[:, :, :48].any(axis=(1, 2)).all())
    assert bool((pack.polygon_vertices >= 0).all()) and bool((pack.polygon_vertices[:, 0] < 48).all()) and bool((pack.polygon_vertices[:, 1] < 32).all())


def _launch(arguments):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", *arguments], cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)


def test_launcher_selftest_over_a_directory_of_packs(tmp_path):
    import make_frame_packs
    packs = str(tmp_path / "packs")
    make_frame_packs.write_packs(packs, 6, views=3, height=32, width=48, instances=[2, 3, 4])
    out = str(tmp_path / "out")
    done = _launch(["--selftest", "--gpus", "2", "--frames-dir", packs, "--out", out, "--selftest-seconds", "0.01"])
    assert done.returncode == 0, done.stderr[-4000:]
    line = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
    assert line["frames"] == 6 and line["ranks"] == 2 and line["frames_dir"] == packs
    assert line["frames_per_instances"] == {"2": 2, "3": 2, "4": 2}
    taken = sorted(int(l.split()[0]) for l in open(os.path.join(out, "completed.log")))
    assert taken == [0, 1, 2, 3, 4, 5]                                  # every file exactly once
    # --frames K: the first K files
    done = _launch(["--selftest", "--gpus", "2", "--frames-dir", packs, "--frames", "4", "--out", str(tmp_path / "out4"), "--selftest-seconds", "0.01"])
    assert done.returncode == 0, done.stderr[-4000:]
    line = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
    assert line["frames"] == 4 and line["frames_per_instances"] == {"2": 2, "3": 1, "4": 1}
    # the packs carry their own shapes
    for flag in (["--views", "3"], ["--instances", "2"], ["--height", "32"], ["--width", "48"]):
        refused = _launch(["--selftest", "--gpus", "2", "--frames-dir", packs, *flag])
        assert refused.returncode != 0 and flag[0] in refused.stderr
    # one file of another image size: the job does not start, the odd file is named
    odd = make_frame_packs.make_pack(9, 3, 32, 40, 2)
    from vsrd_amd import frames
    frames.save_pack(os.path.join(packs, "frame_000003b.npz"), odd)
    refused = _launch(["--selftest", "--gpus", "2", "--frames-dir", packs, "--out", str(tmp_path / "out_odd")])
    assert refused.returncode != 0 and "frame_000003b.npz" in refused.stderr
    assert not os.path.exists(str(tmp_path / "out_odd"))
