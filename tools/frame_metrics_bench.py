#!/usr/bin/env python3
"""3-D / BEV IoU metrics of B = 16 frames of N = 8 boxes: (a) the host path the library offered before vsrd_frame_metrics -- decode on the
device, copy the boxes to the host, operations.box_3d_iou pair by pair, the six means -- against (b) ONE vsrd_frame_metrics launch for
all frames (device time, and wall time including a synchronisation).  Median of five timed repetitions with the fastest and the slowest,
after two warm-up repetitions.  The launch is one latency-bound wave per frame: what it buys is that nothing waits for the host, not
throughput.
    python tools/frame_metrics_bench.py [--out profiles/r07/frame_metrics.txt]"""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N = 16, 8


def median_of(run, repetitions=5, warmup=2):
    for _ in range(warmup):
        run()
    times = [run() for _ in range(repetitions)]
    return statistics.median(times), min(times), max(times)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="")
    args = parser.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import _lib, formats, models, operations, optimization, synthetic
    lib, dev = _lib.load(), torch.device("cuda:0")
    buffers = (("loc", (N, 3)), ("dim", (N, 3)), ("ori", (N, 2)), ("gt", (N, 8, 3)), ("rect", (3, 3)), ("corners", (N, 8, 3)), ("ious", (N, 2)), ("summary", (8,)))
    arena = optimization.FrameArena(B, sum((4 * math.prod(shape) + 255) // 256 * 256 for _, shape in buffers), dev)
    rows = [{name: row.new(shape, fill=0) for name, shape in buffers} for row in arena.rows]
    detector = models.BoxParameters3D(1, N).to(dev)
    tilt = math.radians(2.0)
    rect = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(tilt), -math.sin(tilt)], [0.0, math.sin(tilt), math.cos(tilt)]])
    for f in range(B):
        _, _, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(f, 1, 376, 1408, N)
        rows[f]["loc"].copy_(raw_loc[0]); rows[f]["dim"].copy_(raw_dim[0]); rows[f]["ori"].copy_(raw_ori[0])
        with torch.no_grad():
            detector.locations.copy_(raw_loc); detector.dimensions.copy_(raw_dim); detector.orientations.copy_(raw_ori)
            truth = detector()["boxes_3d"][0]
        rows[f]["gt"].copy_(truth + 0.3 * torch.randn(N, 1, 3, generator=torch.Generator().manual_seed(f)).to(dev))
        rows[f]["rect"].copy_(rect)
    frame = _lib.make_frame_config(N, 1, (0.0, 0.0), 0.0, detector.location_range, detector.dimension_range, frames=(B, arena.stride))
    pointer = lambda name: ctypes.c_void_p(rows[0][name].data_ptr())

    def launch():
        _lib.check(lib.vsrd_frame_metrics(frame, pointer("loc"), pointer("dim"), pointer("ori"), pointer("gt"), pointer("rect"), None, None, pointer("corners"),
                                          pointer("ious"), pointer("summary"), None, _lib.stream()))

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
        summaries = torch.stack([rows[f]["summary"] for f in range(B)]).cpu()
        named = [formats.frame_metrics(s) for s in summaries]
        assert len(named) == B
        return 1000.0 * (time.perf_counter() - t0)
    rotation = operations.rotation_matrix_x(torch.tensor(-np.pi / 2.0))

    def host_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        named = []
        for f in range(B):
            with torch.no_grad():
                detector.locations.copy_(rows[f]["loc"][None]); detector.dimensions.copy_(rows[f]["dim"][None])
                detector.orientations.copy_(rows[f]["ori"][None])
                boxes = (detector()["boxes_3d"][0] @ rect.to(dev).T).cpu()
            truth = (rows[f]["gt"] @ rect.to(dev).T).cpu()
            pairs = [operations.box_3d_iou(boxes[k] @ rotation.T, truth[k] @ rotation.T) for k in range(N)]
            named.append(formats.frame_metrics(formats.frame_metrics_summary([p[0] for p in pairs], [p[1] for p in pairs])))
        return 1000.0 * (time.perf_counter() - t0)
    a, b, c = median_of(host_path), median_of(device_time), median_of(wall_time)
    lines = [f"# tools/frame_metrics_bench.py: B = {B} frames, N = {N} boxes, median of five [fastest .. slowest], ms for all frames",
             f"(a) host path: decode, copy to the host, operations.box_3d_iou per pair   {a[0]:9.3f} [{a[1]:.3f} .. {a[2]:.3f}]  (wall)",
             f"(b) one vsrd_frame_metrics launch                                         {b[0]:9.3f} [{b[1]:.3f} .. {b[2]:.3f}]  (device, events)",
             f"(b) ... with the copy of the {B} summaries to the host and their dicts       {c[0]:9.3f} [{c[1]:.3f} .. {c[2]:.3f}]  (wall)",
             "one latency-bound wave per frame: the gain is that the loop does not wait for the host, not throughput"]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
