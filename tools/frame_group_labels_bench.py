#!/usr/bin/env python3
"""Pseudo-labels of B = 16 frames in the views of their groups, at (N = 8 boxes, L = 100 label views) and (N = 64, L = 1024): (a) the
host path the library offered before vsrd_frame_group_labels -- decode and project on the device, copy the 2-D boxes to the host,
formats.multi_view_confidences frame by frame -- against (b) ONE vsrd_frame_group_labels call for all frames (device time between two
events, and wall time including the copy of the confidences to the host).  Median of five timed repetitions with the fastest and the
slowest, after two warm-up repetitions (one for the host path).  The comparison that matters is (a) against (b).
    python tools/frame_group_labels_bench.py [--out profiles/r07/frame_group_labels.txt]"""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, HEIGHT, WIDTH = 16, 376, 1408
SHAPES = ((8, 100), (64, 1024))            # (N, L)


def median_of(run, repetitions=5, warmup=2):
    for _ in range(warmup):
        run()
    times = [run() for _ in range(repetitions)]
    return statistics.median(times), min(times), max(times)


def measure(N, L):
    from vsrd_amd import _lib, formats, models, operations, optimization, synthetic
    lib, dev = _lib.load(), torch.device("cuda:0")
    f32, u8 = torch.float32, torch.uint8
    buffers = (("loc", (N, 3), f32), ("dim", (N, 3), f32), ("ori", (N, 2), f32), ("E", (L, 16), f32), ("K", (L, 9), f32), ("gt", (L, N, 4), f32),
               ("visible", (L, N), u8), ("corners", (L, N, 8, 3), f32), ("boxes", (L, N, 4), f32), ("mean", (N, N), f32), ("matched", (N,), torch.int64),
               ("confidences", (N,), f32))
    size = lambda shape, dtype: (math.prod(shape) * torch.empty((), dtype=dtype).element_size() + 255) // 256 * 256
    arena = optimization.FrameArena(B, sum(size(shape, dtype) for _, shape, dtype in buffers), dev)
    rows = [{name: row.new(shape, dtype, fill=0) for name, shape, dtype in buffers} for row in arena.rows]
    detector = models.BoxParameters3D(1, N).to(dev)
    groups = []
    for f in range(B):
        _, _, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(f, 1, HEIGHT, WIDTH, N)
        with torch.no_grad():
            detector.locations.copy_(raw_loc); detector.dimensions.copy_(raw_dim); detector.orientations.copy_(raw_ori)
            truth = detector()["boxes_3d"][0].cpu()
        group = synthetic.synthetic_group(f, HEIGHT, WIDTH, L, truth)
        groups.append(group)
        noise = 0.05 * torch.randn(N, 3, generator=torch.Generator().manual_seed(f))          # (the labelled boxes are near the truth, not on it)
        rows[f]["loc"].copy_(raw_loc[0] + noise); rows[f]["dim"].copy_(raw_dim[0]); rows[f]["ori"].copy_(raw_ori[0])
        rows[f]["E"].copy_(group["label_extrinsic_matrices"].reshape(L, 16)); rows[f]["K"].copy_(group["label_intrinsic_matrices"].reshape(L, 9))
        rows[f]["gt"].copy_(group["label_boxes_2d"]); rows[f]["visible"].copy_(group["label_visible"])
    frame = _lib.make_frame_config(N, 1, (HEIGHT, WIDTH), 1.0e-6, detector.location_range, detector.dimension_range, frames=(B, arena.stride))
    pointer = lambda name: ctypes.c_void_p(rows[0][name].data_ptr())

    def launch():
        _lib.check(lib.vsrd_frame_group_labels(frame, pointer("loc"), pointer("dim"), pointer("ori"), L, None, pointer("E"), pointer("K"), pointer("gt"),
                                               pointer("visible"), pointer("corners"), pointer("boxes"), pointer("mean"), pointer("matched"),
                                               pointer("confidences"), None, _lib.stream()))

    def device_time():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        launch()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def wall_time():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        launch()
        confidences = torch.stack([rows[f]["confidences"] for f in range(B)]).cpu()
        assert confidences.shape == (B, N)
        return 1000.0 * (time.perf_counter() - t0)
    tables = [[torch.where(g["label_visible"][l].bool(), torch.arange(N), torch.full((N,), -1)) for l in range(L)] for g in groups]
    truths = [list(g["label_boxes_2d"].unflatten(-1, (2, 2))) for g in groups]
    cameras = [(g["label_extrinsic_matrices"].to(dev), g["label_intrinsic_matrices"].to(dev)) for g in groups]

    def host_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(B):
            with torch.no_grad():
                detector.locations.copy_(rows[f]["loc"][None]); detector.dimensions.copy_(rows[f]["dim"][None])
                detector.orientations.copy_(rows[f]["ori"][None])
                boxes, _ = operations.project_boxes_multi_view(detector()["boxes_3d"][0], *cameras[f], (HEIGHT, WIDTH))
            confidences, _, _ = formats.multi_view_confidences(list(boxes.cpu()), truths[f], tables[f])
            assert confidences.shape == (N,)
        return 1000.0 * (time.perf_counter() - t0)
    a, b, c = median_of(host_path, warmup=1), median_of(device_time), median_of(wall_time)
    return [f"B = {B} frames, N = {N} boxes, L = {L} label views; ms for all frames",
            f"(a) host path: decode + project, copy the boxes out, formats.multi_view_confidences   {a[0]:10.3f} [{a[1]:.3f} .. {a[2]:.3f}]  (wall)",
            f"(b) one vsrd_frame_group_labels call (three kernels)                                 {b[0]:10.3f} [{b[1]:.3f} .. {b[2]:.3f}]  (device, events)",
            f"(b) ... with the copy of the {B} frames' confidences to the host                        {c[0]:10.3f} [{c[1]:.3f} .. {c[2]:.3f}]  (wall)"]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="")
    args = parser.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    lines = ["# tools/frame_group_labels_bench.py: median of five [fastest .. slowest]"]
    for N, L in SHAPES:
        lines += measure(N, L)
        print("\n".join(lines[-4:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
