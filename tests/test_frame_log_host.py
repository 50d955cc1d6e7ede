"""The host side of the frame log (vsrd_frame_log): the binding against the header, history.json, the step snapshots' files, the selection
rule, the configuration's refusals and the launcher's flags -- no GPU."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsrd_hip.h")

LOSSES = ("iou_projection_loss", "l1_projection_loss", "silhouette_loss", "eikonal_loss", "loss")
RATES = ("learning_rates/detector/locations", "learning_rates/detector/dimensions", "learning_rates/detector/orientations",
         "learning_rates/detector/embeddings", "learning_rates/hyper_distance_field")
HYPERPARAMETERS = ("hyperparameters/sdf_union_temperature", "hyperparameters/sdf_std_deviation", "hyperparameters/cosine_ratio")
METRICS = ("iou_3d", "iou_bev", "accuracy_3d_25", "accuracy_bev_25", "accuracy_3d_50", "accuracy_bev_50")


def _members(struct):
    header = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
    declarations = [line for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if line.strip()]
    return [re.search(r"(\w+)\s*$", declaration).group(1) for declaration in declarations]


def test_binding_matches_the_header(tmp_path):
    """The prototype, the constants, and both structures against gcc's view of the header: names in order, sizeof, every offset and size."""
    from vsrd_amd import _lib
    header = open(HEADER).read()
    assert re.search(r"^#define VSRD_ABI_VERSION 12$", header, flags=re.M) and _lib.ABI_VERSION == 12
    assert _lib.SIGNATURES["vsrd_frame_log"] == (ctypes.c_int32, [ctypes.POINTER(_lib.FrameLogConfig), ctypes.c_void_p])
    assert _lib.FRAME_LOG_COLUMNS == int(re.search(r"^#define VSRD_LOG_SCALARS (\d+)$", header, flags=re.M).group(1)) == 1 + 5 + 5 + 3 + 8
    assert _lib.FRAME_LOG_SEGMENTS == int(re.search(r"^#define VSRD_LOG_MAX_SEGMENTS (\d+)$", header, flags=re.M).group(1)) == 32
    structs = {"vsrd_frame_log_config": _lib.FrameLogConfig, "vsrd_log_segment": _lib.LogSegment}
    lines = []
    for struct in structs:
        lines.append(f'printf("{struct} %zu 0\\n", sizeof({struct}));')
        lines += [f'printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct}*)0)->{name}));' for name in _members(struct)]
    source = tmp_path / "layout.c"
    source.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vsrd_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(tmp_path / "layout")], check=True)
    rows = [line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()]
    compiled = {key: (int(first), int(second)) for key, first, second in rows}
    for struct, binding in structs.items():
        names = [name for name, _ in binding._fields_]
        assert names == _members(struct)
        assert ctypes.sizeof(binding) == compiled[struct][0]
        for name in names:
            member = getattr(binding, name)
            assert (member.offset, member.size) == compiled[f"{struct}.{name}"], (struct, name)


def _history(steps, warmup, metrics):
    """A history as FrameOptimizer.history() returns it, from numbers that are exact in float32."""
    rows = len(steps)
    table = {name: torch.tensor([0.5 + k + 0.25 * j for j in range(rows)]) for k, name in enumerate(LOSSES)}
    table["eikonal_loss"] = torch.where(torch.tensor(steps) >= warmup, table["eikonal_loss"], torch.full((rows,), float("nan")))
    return dict(steps=torch.tensor(steps, dtype=torch.int32), learning_rates=torch.tensor([[2.0 ** -(5 + g + j) for g in range(5)] for j in range(rows)]),
                hyperparameters=torch.tensor([[1.0 - 0.125 * j, 0.5 - 0.0625 * j, 0.25 * j] for j in range(rows)]), metrics=torch.tensor(metrics), **table)


def test_save_frame_history_uses_the_references_names(tmp_path):
    from vsrd_amd import formats
    nan, inf = float("nan"), float("inf")
    summaries = [[nan] * 8,                                             # no metrics were logged
                 [0.0] * 8,                                             # metrics on, no pair with ground truth
                 [2.0, 0.5, 0.75, 1.0, 1.0, 0.5, inf, 0.0],             # one value is not finite: left out
                 [3.0, 0.5, 0.75, 1.0, 1.0, 0.5, 0.25, 0.0]]
    history = _history([2, 5, 8, 11], warmup=6, metrics=summaries)
    path = formats.save_frame_history(str(tmp_path), history)
    assert path == str(tmp_path / "history.json") and os.listdir(tmp_path) == ["history.json"]           # (no temporary file left)
    records = json.load(open(path))
    assert [r["step"] for r in records] == [2, 5, 8, 11] and all(isinstance(r["step"], int) for r in records)
    always = {"step", *(f"losses/{name}" for name in LOSSES if name != "eikonal_loss"), *RATES, *HYPERPARAMETERS}
    assert set(records[0]) == always                                                           # box-only: no eikonal key; NaN summary: no metrics
    assert set(records[1]) == always
    assert set(records[2]) == always | {"losses/eikonal_loss"} | {f"metrics/{name}" for name in METRICS if name != "accuracy_bev_50"}
    assert set(records[3]) == always | {"losses/eikonal_loss"} | {f"metrics/{name}" for name in METRICS}
    for j, record in enumerate(records):
        assert record["losses/loss"] == 4.5 + 0.25 * j and record["losses/iou_projection_loss"] == 0.5 + 0.25 * j
        assert [record[name] for name in RATES] == [2.0 ** -(5 + g + j) for g in range(5)]
        assert [record[name] for name in HYPERPARAMETERS] == [1.0 - 0.125 * j, 0.5 - 0.0625 * j, 0.25 * j]
    assert records[3]["losses/eikonal_loss"] == 3.5 + 0.75 and records[3]["metrics/iou_bev"] == 0.75 and records[3]["metrics/accuracy_bev_50"] == 0.25
    assert all(math.isfinite(value) for record in records for value in record.values())
    assert formats.frame_history_records(history) == records


def _folder(tmp_path, name, checkpoints):
    """A frame's folder of hand-made checkpoints: {file name: (step, metrics)}; every file's bytes differ (its step is in it)."""
    folder = tmp_path / name
    folder.mkdir()
    for file_name, (step, metrics) in checkpoints.items():
        torch.save(dict(step=step, models={"detector": {"locations": torch.full((1, 2, 3), float(step))}}, metrics=metrics), folder / file_name)
    return str(folder)


def _is_copy_of(folder, name):
    return open(os.path.join(folder, "model.pt"), "rb").read() == open(os.path.join(folder, name), "rb").read()


def test_select_model_carries_the_references_rule(tmp_path):
    from vsrd_amd import formats
    files = {"step_3.pt": (3, dict(iou_3d=0.25, mask_iou=0.75)), "step_7.pt": (7, dict(iou_3d=0.75, mask_iou=0.25)),
             "step_11.pt": (11, dict(iou_3d=0.5, mask_iou=0.875)), "step_15.pt": (15, dict(mask_iou=1.0))}
    folder = _folder(tmp_path, "plain", files)
    # maximum and minimum of one metric; the file without it never competes
    winner, values = formats.select_model(folder, ["iou_3d"], maximum=True)
    assert winner == os.path.join(folder, "step_7.pt") and values == dict(iou_3d=0.75) and _is_copy_of(folder, "step_7.pt")
    winner, _ = formats.select_model(folder, "iou_3d")
    assert winner == os.path.join(folder, "step_3.pt") and _is_copy_of(folder, "step_3.pt")
    assert sorted(os.listdir(folder)) == sorted([*files, "model.pt"])                           # (no temporary file left)
    # the mean of two metrics: 0.5, 0.5, 0.6875 -- and the tie of the first two goes to the earliest step when the smallest is asked for
    winner, values = formats.select_model(folder, ["iou_3d", "mask_iou"], maximum=True)
    assert winner == os.path.join(folder, "step_11.pt") and values == dict(iou_3d=0.5, mask_iou=0.875) and _is_copy_of(folder, "step_11.pt")
    assert formats.select_model(folder, ["iou_3d", "mask_iou"])[0] == os.path.join(folder, "step_3.pt")
    # a constraint that removes the best file; a file lacking the constrained metric does not meet it
    assert formats.select_model(folder, ["iou_3d"], maximum=True, constraints=["mask_iou>=0.5"])[0] == os.path.join(folder, "step_11.pt")
    assert formats.select_model(folder, ["mask_iou"], maximum=True, constraints=["iou_3d>0"])[0] == os.path.join(folder, "step_11.pt")
    assert formats.select_model(folder, ["mask_iou"], maximum=True)[0] == os.path.join(folder, "step_15.pt")
    assert formats.select_model(folder, ["iou_3d"], maximum=True, constraints=["iou_3d<0.75", "mask_iou!=0.875"])[0] == os.path.join(folder, "step_3.pt")
    # a step range (range(*step_range), as the reference's epoch_range)
    assert formats.select_model(folder, ["iou_3d"], maximum=True, step_range=(8, 16))[0] == os.path.join(folder, "step_11.pt")
    assert formats.select_model(folder, ["iou_3d"], maximum=True, step_range=(4,))[0] == os.path.join(folder, "step_3.pt")
    # an existing model.pt is ignored as a candidate, even when it would win ...
    torch.save(dict(step=99, models={}, metrics=dict(iou_3d=10.0)), os.path.join(folder, "model.pt"))
    assert formats.select_model(folder, ["iou_3d"], maximum=True)[0] == os.path.join(folder, "step_7.pt") and _is_copy_of(folder, "step_7.pt")
    # ... and left alone when nothing competes
    before = open(os.path.join(folder, "model.pt"), "rb").read()
    assert formats.select_model(folder, ["unknown"], maximum=True) == (None, {}) and open(os.path.join(folder, "model.pt"), "rb").read() == before
    assert formats.select_model(folder, ["iou_3d"], constraints=["iou_3d>5"]) == (None, {})
    with pytest.raises(ValueError):
        formats.select_model(folder, ["iou_3d"], constraints=["iou_3d~1"])
    with pytest.raises(ValueError):
        formats.select_model(folder, [])


def test_select_model_keeps_the_earliest_step_on_a_tie(tmp_path):
    """Ascending STEP order, whatever the names sort like (step_11 < step_3 as strings) and whichever way the comparison goes."""
    from vsrd_amd import formats
    folder = _folder(tmp_path, "tie", {"step_11.pt": (11, dict(iou_3d=0.5)), "step_3.pt": (3, dict(iou_3d=0.5)), "step_7.pt": (7, dict(iou_3d=0.25))})
    assert formats.select_model(folder, ["iou_3d"], maximum=True)[0] == os.path.join(folder, "step_3.pt") and _is_copy_of(folder, "step_3.pt")
    assert formats.select_model(folder, ["iou_3d"])[0] == os.path.join(folder, "step_7.pt")
    folder = _folder(tmp_path, "all", {"step_11.pt": (11, dict(iou_3d=0.5)), "step_3.pt": (3, dict(iou_3d=0.5)), "step_7.pt": (7, dict(iou_3d=0.5))})
    assert formats.select_model(folder, ["iou_3d"])[0] == os.path.join(folder, "step_3.pt")


def test_save_frame_snapshots_writes_one_file_per_step(tmp_path):
    from vsrd_amd import formats
    summary = torch.tensor([2.0, 0.5, 0.75, 1.0, 1.0, 0.5, 0.25, 0.0])
    snapshots = [dict(step=torch.tensor(step, dtype=torch.int32), models={"detector": {"locations": torch.full((1, 2, 3), float(step))}, "hyper_distance_field": {}},
                      metrics=dict(summary=summary, mask_iou=torch.tensor([0.25, 0.75]))) for step in (3, 7, 11)]
    paths = formats.save_frame_snapshots(str(tmp_path), snapshots, skip_steps=(11,))
    assert paths == [str(tmp_path / "step_3.pt"), str(tmp_path / "step_7.pt")] and sorted(os.listdir(tmp_path)) == ["step_3.pt", "step_7.pt"]
    loaded = torch.load(paths[1], map_location="cpu", weights_only=False)
    assert set(loaded) == {"step", "models", "metrics"} and loaded["step"] == 7 and isinstance(loaded["step"], int)
    assert torch.equal(loaded["models"]["detector"]["locations"], torch.full((1, 2, 3), 7.0))
    assert loaded["metrics"] == dict(zip(METRICS, [0.5, 0.75, 1.0, 1.0, 0.5, 0.25]), mask_iou=0.5)
    assert all(isinstance(value, float) for value in loaded["metrics"].values())
    assert formats.select_model(str(tmp_path), ["mask_iou"], maximum=True)[0] == paths[0]            # (a tie: the earliest step)
    # payloads pass through snapshot_payloads unchanged, so save_frame_snapshots takes either
    payloads = formats.snapshot_payloads(snapshots)
    again = formats.snapshot_payloads(payloads)
    assert [(p["step"], p["metrics"]) for p in again] == [(p["step"], p["metrics"]) for p in payloads] and again[1]["metrics"] == loaded["metrics"]
    assert formats.save_frame_snapshots(str(tmp_path / "again"), payloads, skip_steps=(3, 7)) == [str(tmp_path / "again" / "step_11.pt")]
    # without metrics or masks a snapshot's metrics are empty, and a summary without a pair names nothing
    bare = formats.snapshot_payloads([dict(step=torch.tensor(3), models={"detector": {}}, metrics={}),
                                      dict(step=torch.tensor(7), models={"detector": {}}, metrics=dict(summary=torch.zeros(8)))])
    assert [payload["metrics"] for payload in bare] == [{}, {}]


def test_config_refuses_negative_intervals_and_loops_without_the_fused_glue():
    """Before anything touches a device: the intervals are at least 0, and the log belongs to the fused-glue graph loop."""
    from vsrd_amd import optimization
    assert optimization.OptimizationConfig().scalar_interval == 0 and optimization.OptimizationConfig().checkpoint_interval == 0
    for name in ("scalar_interval", "checkpoint_interval"):
        with pytest.raises(ValueError, match=name):
            optimization.OptimizationConfig(**{name: -1})
    inputs = optimization.FrameInputs((4, 6), torch.eye(3).expand(2, 3, 3), torch.eye(4).expand(2, 4, 4), torch.rand(2, 4, 6, 2), torch.zeros(2, 2, 2, 2),
                                      torch.ones(2, 2, dtype=torch.bool))
    for intervals in (dict(scalar_interval=3), dict(checkpoint_interval=4)):
        config = optimization.OptimizationConfig(num_steps=12, num_rays=8, num_samples=16, **intervals)
        for loop in (dict(graph=False), dict(graph=True, fused_glue=False), dict(graph=False, fused_glue=False)):
            with pytest.raises(ValueError, match="fused-glue graph loop"):
                optimization.FrameOptimizer(inputs, config, "cpu", **loop)


@pytest.mark.parametrize("flags", [["--scalar-interval", "3"], ["--ckpt-interval", "4"], ["--select", "iou_3d:max"]])
def test_launcher_refuses_the_flags_without_out_or_with_selftest(flags, tmp_path):
    command = [sys.executable, "-m", "vsrd_amd.launcher", "--gpus", "1", "--frames", "1", "--max-restarts", "0", *flags]
    environment = {key: value for key, value in os.environ.items() if key not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    for extra, needle in (([], "needs --out"), (["--out", str(tmp_path / "out"), "--selftest"], "--selftest")):
        result = subprocess.run(command + extra, cwd=ROOT, env=environment, capture_output=True, text=True, timeout=120)
        assert result.returncode != 0 and flags[0] in result.stderr and needle in result.stderr, result.stderr
    assert not os.path.exists(tmp_path / "out")


def test_launcher_parses_select_and_refuses_nonsense():
    from vsrd_amd import launcher
    assert launcher.parse_select("") is None and launcher.parse_select("iou_3d") == (["iou_3d"], False)
    assert launcher.parse_select("iou_3d,mask_iou:max") == (["iou_3d", "mask_iou"], True) and launcher.parse_select("mask_iou:min") == (["mask_iou"], False)
    for text in ("iou_3d:most", ":max", "iou 3d", "a,,b"):
        with pytest.raises(ValueError):
            launcher.parse_select(text)
    for flags in (["--select", "iou_3d:most"], ["--scalar-interval", "-1"]):
        with pytest.raises(SystemExit):
            launcher.main(["--out", "somewhere", *flags])
