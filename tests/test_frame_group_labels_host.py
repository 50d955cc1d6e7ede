"""The host side of a frame's GROUP (the frames that get the target's labels: vsrd_frame_group_labels): the label_* members of a frame pack
(round trip, validation, the cheap reader of L, the synthetic exporter), formats.save_frame_group_labels, and what the launcher refuses
before any rank starts."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GROUP = ("label_frame_ids", "label_intrinsic_matrices", "label_extrinsic_matrices", "label_boxes_2d", "label_visible")
SMALL = dict(views=3, height=32, width=64)


def _pack(label_views=0, frame=1, instances=3):
    import make_frame_packs as tool
    return tool.make_pack(frame, SMALL["views"], SMALL["height"], SMALL["width"], instances, label_views=label_views)


def _members(path):
    with np.load(path) as data:
        return {name: data[name] for name in data.files}


# ---- the pack members --------------------------------------------------------------------------------------------------------------------
def test_pack_round_trip_with_and_without_a_group(tmp_path):
    from vsrd_amd import frames
    plain, grouped = _pack(), _pack(label_views=5)
    assert plain.num_label_views == 0 and all(getattr(plain, field) is None for field in GROUP)
    assert grouped.num_label_views == 5
    assert grouped.label_frame_ids.shape == (5,) and grouped.label_intrinsic_matrices.shape == (5, 3, 3) and grouped.label_extrinsic_matrices.shape == (5, 4, 4)
    assert grouped.label_boxes_2d.shape == (5, 3, 4) and grouped.label_visible.shape == (5, 3)
    for name, pack in (("plain", plain), ("grouped", grouped)):
        path = str(tmp_path / f"{name}.npz")
        frames.save_pack(path, pack)
        loaded = frames.load_pack(path)
        assert frames.pack_label_views(path) == pack.num_label_views == loaded.num_label_views
        assert frames.pack_counts(path) == (SMALL["views"], SMALL["height"], SMALL["width"], 3)          # (unchanged: four numbers)
        for field in GROUP:
            a, b = getattr(pack, field), getattr(loaded, field)
            assert (a is None and b is None) or (b.dtype == a.dtype and np.array_equal(a, b)), (name, field)
        assert set(_members(path)) >= {"image_size", "inside"} and (set(GROUP) <= set(_members(path))) == (name == "grouped")
    loaded = frames.load_pack(str(tmp_path / "grouped.npz"))
    assert loaded.label_frame_ids.dtype == np.int64 and loaded.label_visible.dtype == np.uint8 and loaded.label_boxes_2d.dtype == np.float32


def test_the_synthetic_group_holds_the_target_and_no_source_position():
    pack = _pack(label_views=6)
    assert np.array_equal(pack.label_extrinsic_matrices[0], np.eye(4, dtype=np.float32))                  # the target, first
    sources = {float(z) for z in pack.extrinsic_matrices[1:, 2, 3]}
    assert not sources & {float(z) for z in pack.label_extrinsic_matrices[1:, 2, 3]}
    assert len(set(pack.label_frame_ids.tolist())) == 6
    # boxes: (xmin, ymin, xmax, ymax) inside the image, with area where visible and zero where not; the target sees every instance
    boxes, visible = pack.label_boxes_2d, pack.label_visible.astype(bool)
    assert bool(visible[0].all())
    assert bool((boxes[~visible] == 0).all())
    area = (boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1])
    assert bool((area[visible] > 0).all()) and boxes.min() >= 0 and boxes[..., 0::2].max() <= SMALL["width"] and boxes[..., 1::2].max() <= SMALL["height"]


def _without(pack, *fields):
    import dataclasses
    return dataclasses.replace(pack, **{field: None for field in fields})


def test_malformed_groups_are_rejected_by_name(tmp_path):
    import dataclasses
    from vsrd_amd import frames
    good = _pack(label_views=4)
    frames.validate(good, "good")
    cases = {
        "only some members": (_without(good, "label_visible"), "needs all of"),
        "one member alone": (_without(good, *GROUP[1:]), "needs all of"),
        "ids twice": (dataclasses.replace(good, label_frame_ids=np.array([7, 8, 7, 9], dtype=np.int64)), "twice"),
        "no views": (dataclasses.replace(good, label_frame_ids=np.zeros(0, dtype=np.int64), label_intrinsic_matrices=np.zeros((0, 3, 3), np.float32),
                                         label_extrinsic_matrices=np.zeros((0, 4, 4), np.float32), label_boxes_2d=np.zeros((0, 3, 4), np.float32),
                                         label_visible=np.zeros((0, 3), np.uint8)), f"1..{frames.MAX_LABEL_VIEWS}"),
        "too many views": (dataclasses.replace(good, label_frame_ids=np.arange(frames.MAX_LABEL_VIEWS + 1, dtype=np.int64)), f"1..{frames.MAX_LABEL_VIEWS}"),
        "intrinsics": (dataclasses.replace(good, label_intrinsic_matrices=good.label_intrinsic_matrices[:3]), "label_intrinsic_matrices of shape"),
        "extrinsics": (dataclasses.replace(good, label_extrinsic_matrices=good.label_extrinsic_matrices[:, :3]), "label_extrinsic_matrices of shape"),
        "boxes": (dataclasses.replace(good, label_boxes_2d=good.label_boxes_2d[:, :2]), "label_boxes_2d of shape"),
        "visible": (dataclasses.replace(good, label_visible=good.label_visible.T.copy()), "label_visible of shape"),
        "ids' shape": (dataclasses.replace(good, label_frame_ids=good.label_frame_ids[:, None]), "label_frame_ids of shape"),
    }
    for label, (pack, why) in cases.items():
        with pytest.raises(ValueError, match="case file") as error:
            frames.validate(pack, "case file")
        assert why in str(error.value), (label, str(error.value))
        with pytest.raises(ValueError):
            frames.save_pack(str(tmp_path / "bad.npz"), pack)
    assert frames.MAX_LABEL_VIEWS == 4096
    # a file with only some of the members is malformed when it is loaded, and named
    path = str(tmp_path / "partial.npz")
    frames.save_pack(path, good)
    members = _members(path)
    del members["label_boxes_2d"]
    np.savez(path, **members)
    with pytest.raises(ValueError, match="partial.npz"):
        frames.load_pack(path)


# (tools/make_frame_packs.write_packs(tmp, 2, views=3, height=32, width=64, instances=(2, 3))[1] as the tool wrote it before it knew of groups:
#  sha256 over every member's name, dtype, shape and bytes, in file order -- an .npz itself carries the time it was written)
PARENT_MEMBERS = ["image_size", "intrinsic_matrices", "extrinsic_matrices", "view_offsets", "instance_ids", "polygon_offsets", "polygon_vertices", "inside",
                  "boxes_3d"]
PARENT_DIGEST = "b034880e5e80e1ee3ab0d1c73e6b6fe72e7ab0bb63f8630c7af40d2c7e9a2730"


def test_packs_without_the_flag_are_what_they_were(tmp_path):
    import make_frame_packs as tool
    path = tool.write_packs(str(tmp_path / "plain"), 2, views=3, height=32, width=64, instances=(2, 3))[1]
    digest = hashlib.sha256()
    with np.load(path) as data:
        assert list(data.files) == PARENT_MEMBERS
        for name in data.files:
            array = data[name]
            for part in (name.encode(), str(array.dtype).encode(), str(array.shape).encode(), np.ascontiguousarray(array).tobytes()):
                digest.update(part)
    assert digest.hexdigest() == PARENT_DIGEST
    assert tool.main(["--out", str(tmp_path / "flag"), "--count", "2", "--views", "3", "--height", "32", "--width", "64", "--instances", "2,3", "--label-views", "4"]) == 0
    grouped = _members(str(tmp_path / "flag" / "frame_000001.npz"))
    assert list(grouped) == PARENT_MEMBERS + list(GROUP) and all(np.array_equal(grouped[name], _members(path)[name]) for name in PARENT_MEMBERS)


def test_frame_inputs_carry_the_group_as_optional_fields():
    from vsrd_amd import optimization
    empty = torch.zeros(0)
    inputs = optimization.FrameInputs((4, 4), empty, empty, empty, empty, empty)
    assert all(getattr(inputs, field) is None for field in GROUP) and optimization.label_view_count(inputs) == 0
    inputs.label_frame_ids = torch.arange(7)
    assert optimization.label_view_count(inputs) == 7 and optimization.label_view_count(_pack(label_views=2)) == 2


# ---- the files ---------------------------------------------------------------------------------------------------------------------------
def _labels(seed, ids):
    g = torch.Generator().manual_seed(seed)
    L, n = len(ids), 3
    centres = torch.randn(L, n, 1, 3, generator=g) + torch.tensor([0.0, 1.0, 20.0])
    corner = 300.0 * torch.rand(L, n, 1, 2, generator=g)
    return dict(boxes_3d=centres + torch.randn(L, n, 8, 3, generator=g), boxes_2d=torch.cat([corner, corner + 50.0 * torch.rand(L, n, 1, 2, generator=g)], dim=-2),
                confidences=torch.rand(n, generator=g), matched_gt=torch.tensor([2, 0, 1]), mean_iou=torch.rand(n, n, generator=g),
                frame_ids=torch.tensor(ids, dtype=torch.int64))


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(base, name), folder) for base, _, names in os.walk(folder) for name in names)


def test_save_frame_group_labels_writes_one_json_and_one_txt_per_group_frame(tmp_path):
    from vsrd_amd import formats
    folder, ids = str(tmp_path / "frame_000003"), [4711, 12, 3000000000]
    expected = sorted([os.path.join("group", kind, f"{i:010d}.{suffix}") for i in ids for kind, suffix in (("predictions", "json"), ("labels", "txt"))])
    for seed in (1, 2):                                            # the second call replaces the files of the first
        labels = _labels(seed, ids)
        formats.save_frame_group_labels(folder, labels)
        assert _tree(folder) == expected                           # exactly these: no temporary file stays behind
        scores = labels["confidences"].tolist()
        for view, frame_id in enumerate(ids):
            with open(os.path.join(folder, "group", "predictions", f"{frame_id:010d}.json")) as file:
                record = json.load(file)
            assert list(record) == ["boxes_3d", "boxes_2d", "confidences"] and all(list(value) == ["car"] for value in record.values())
            assert record == formats.prediction_record(labels["boxes_3d"][view], labels["boxes_2d"][view], labels["confidences"])
            assert record["confidences"]["car"] == scores          # the same confidences in every file
            with open(os.path.join(folder, "group", "labels", f"{frame_id:010d}.txt")) as file:
                lines = file.readlines()
            assert lines == [formats.kitti_label_line("car", labels["boxes_3d"][view][k], labels["boxes_2d"][view][k], scores[k]) for k in range(3)]
    with pytest.raises(ValueError):
        formats.save_frame_group_labels(folder, _labels(1, [5, 5, 6]))


# ---- the launcher's refusals (before any rank starts: no GPU) -------------------------------------------------------------------------
def _launcher(*arguments):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", *arguments], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)


def test_launcher_refuses_group_predictions_without_out_or_without_a_group(tmp_path):
    import make_frame_packs as tool
    done = _launcher("--group-predictions", "--label-views", "5", "--frames", "2")
    assert done.returncode != 0 and "--group-predictions" in done.stderr and "--out" in done.stderr
    out = str(tmp_path / "out")
    done = _launcher("--group-predictions", "--frames", "2", "--out", out)                 # synthetic frames without --label-views
    assert done.returncode != 0 and "--label-views" in done.stderr
    done = _launcher("--group-predictions", "--selftest", "--label-views", "5", "--frames", "2", "--out", out)
    assert done.returncode != 0 and "--selftest" in done.stderr
    packs = str(tmp_path / "packs")
    tool.write_packs(packs, 1, label_views=3, **SMALL, instances=(2,))                     # frame_000000 has a group ...
    os.rename(tool.write_packs(str(tmp_path / "other"), 2, **SMALL, instances=(2,))[1], os.path.join(packs, "frame_000001.npz"))      # ... frame_000001 has none
    done = _launcher("--group-predictions", "--frames-dir", packs, "--out", out)
    assert done.returncode != 0 and "frame_000001.npz" in done.stderr and "group" in done.stderr and "frame_000000.npz" not in done.stderr
    assert not os.path.exists(out)
