#!/usr/bin/env python3
"""Pseudo-labels of B = 16 frames in the views of their groups, at (N = 8 boxes, L = 100 label views) and (N = 64, L = 1024): (a) the
host path the library offered before vsrd_frame_group_labels -- decode and project on the device, copy the 2-D boxes to the host,
formats.multi_view_confidences frame by frame -- against (b) ONE vsrd_frame_group_labels call for all frames (device time between two
events, and wall time including the copy of the confidences to the host).  Median of five timed repetitions with the fastest and the
slowest, after two warm-up repetitions (one for the host path).  The comparison that matters is (a) against (b).
    python tools/frame_group_labels_bench.py [--out profiles/r07/frame_group_labels.txt]"""
import argparse
import ctypes
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
    from vsrd_amd import _lib, formats, models, operations, synthetic
    lib, dev = _lib.load(), torch.device("cuda:0")
    fields = (("loc", N * 12), ("dim", N * 12), ("ori", N * 8), ("E", L * 64), ("K", L * 36), ("gt", L * N * 16), ("visible", L * N),
              ("corners", L * N * 96), ("boxes", L * N * 16), ("mean", N * N * 4), ("matched", N * 8), ("confidences", N * 4))
    offsets, at = {}, 0
    for name, nbytes in fields:
        offsets[name] = (at, nbytes)
        at = (at + nbytes + 255) // 256 * 256
    stride = at
    arena = torch.zeros(B, stride, dtype=torch.uint8, device=dev)

    def view(f, name, shape, dtype=torch.float32):
        offset, nbytes = offsets[name]
        return arena[f, offset:offset + nbytes].view(dtype).view(shape)
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
        view(f, "loc", (N, 3)).copy_(raw_loc[0] + noise); view(f, "dim", (N, 3)).copy_(raw_dim[0]); view(f, "ori", (N, 2)).copy_(raw_ori[0])
        view(f, "E", (L, 16)).copy_(group["label_extrinsic_matrices"].reshape(L, 16)); view(f, "K", (L, 9)).copy_(group["label_intrinsic_matrices"].reshape(L, 9))
        view(f, "gt", (L, N, 4)).copy_(group["label_boxes_2d"]); view(f, "visible", (L, N), torch.uint8).copy_(group["label_visible"])
    frame = _lib.FrameConfig()
    frame.num_boxes, frame.num_views = N, 1
    frame.height, frame.width, frame.epsilon = float(HEIGHT), float(WIDTH), 1.0e-6
    for j in range(3):
        frame.location_lo[j], frame.location_hi[j] = float(detector.location_range[0, j]), float(detector.location_range[1, j])
        frame.dimension_lo[j], frame.dimension_hi[j] = float(detector.dimension_range[0, j]), float(detector.dimension_range[1, j])
    frame.num_frames, frame.frame_stride = B, stride
    pointer = lambda name: ctypes.c_void_p(arena.data_ptr() + offsets[name][0])

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
        confidences = torch.stack([view(f, "confidences", (N,)) for f in range(B)]).cpu()
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
                detector.locations.copy_(view(f, "loc", (N, 3))[None]); detector.dimensions.copy_(view(f, "dim", (N, 3))[None])
                detector.orientations.copy_(view(f, "ori", (N, 2))[None])
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
