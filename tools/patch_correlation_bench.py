#!/usr/bin/env python3
"""What the device-side patch-correlation loss (vsrd_patch_correlation_forward / _backward, csrc/patch_correlation.h) buys at the
reference's own shape -- 17 views, 100 rays, 11 x 11 patches, 376 x 1408 images -- against the same computation composed from torch
operators on the device: tests/patch_correlation_reference.py in float32, the restatement of scripts/main.py:783-851 with V grid_sample
calls' worth of sampling, the homography chains and a Python loop with cov / sqrt / topk per converged ray.  One call = forward + backward
to positions and normals.  The arithmetic is tiny; what differs is the launch count, so both the device time (events around the call) and
the wall time (with a synchronisation behind it) are reported: the median of five with the fastest and the slowest, after one warm-up
call each, the two run in turns in one process.  The native call runs on pre-converted gray planes (losses.grayscale_images, once per
frame); the conversion itself is timed separately.
    python tools/patch_correlation_bench.py [--out profiles/r07/patch_correlation.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="")
    parser.add_argument("--views", type=int, default=17)
    parser.add_argument("--rays", type=int, default=100)
    parser.add_argument("--height", type=int, default=376)
    parser.add_argument("--width", type=int, default=1408)
    parser.add_argument("--patch", type=int, default=11)
    parser.add_argument("--top-k", type=int, default=4)
    parser.add_argument("--repetitions", type=int, default=5)
    args = parser.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import patch_correlation_reference as pcr
    from vsrd_amd import losses
    dev = torch.device("cuda:0")
    patch_size = (args.patch, args.patch)
    s = pcr.scene(0, args.views, args.rays, args.height, args.width, smooth=True, patch_size=patch_size)
    images, K, E = s["images"].to(dev), s["K"].to(dev), s["E"].to(dev)
    pixels, converged = s["pixels"].to(dev), s["converged"].to(dev)
    indices = pixels[:, 1] * args.width + pixels[:, 0]
    gray = losses.grayscale_images(images)

    def native():
        p, n = s["positions"].to(dev).requires_grad_(True), s["normals"].to(dev).requires_grad_(True)
        loss = losses.patch_correlation_loss(gray, K, E, indices, p, n, converged, patch_size, args.top_k)
        return (loss.detach(), *torch.autograd.grad(loss, [p, n]))

    def composed():
        p, n = s["positions"].to(dev).requires_grad_(True), s["normals"].to(dev).requires_grad_(True)
        loss = pcr.reference(images, K, E, pixels, p, n, converged, patch_size, args.top_k, dtype=torch.float32, record=False)["loss"]
        return (loss.detach(), *torch.autograd.grad(loss, [p, n]))

    def timed(call):
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        out = call()
        end.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, start.elapsed_time(end) * 1e-3, out

    calls = {"native": native, "composed": composed, "grayscale": lambda: losses.grayscale_images(images)}
    times = {name: [] for name in calls}
    results = {}
    for repetition in range(args.repetitions + 1):
        for name, call in calls.items():
            wall, device, results[name] = timed(call)
            if repetition:                          # (the first turn of each warms it up)
                times[name].append((wall, device))

    def summary(values):
        return f"{1e3 * statistics.median(values):9.3f} [{1e3 * min(values):.3f} .. {1e3 * max(values):.3f}] ms"
    gap = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    lines = [f"# tools/patch_correlation_bench.py: {args.views} views, {args.rays} rays (all converged), {args.patch} x {args.patch} patches, top-{args.top_k}, "
             f"{args.height} x {args.width} images; one call = forward + backward to positions and normals",
             f"# median of {args.repetitions} [fastest .. slowest], the calls run in turns in one process; wall = host time with a synchronisation behind the call"]
    for name, label in (("native", "vsrd_patch_correlation_*, gray planes given"), ("composed", "torch operators, float32 (grid_sample, cov, topk per ray)"),
                        ("grayscale", "vsrd_grayscale_images, once per frame")):
        lines.append(f"{label:58s} wall {summary([w for w, _ in times[name]])}   device {summary([d for _, d in times[name]])}")
    lines.append(f"wall, composed / native: {statistics.median([w for w, _ in times['composed']]) / statistics.median([w for w, _ in times['native']]):.1f} x "
                 f"(launch count, not throughput: the arithmetic is {args.rays} x {args.views} x {args.patch * args.patch} samples)")
    lines.append(f"native against composed: |loss difference| {abs(results['native'][0].item() - results['composed'][0].item()):.2e}, "
                 f"grad positions {gap(results['native'][1], results['composed'][1]):.2e}, grad normals {gap(results['native'][2], results['composed'][2]):.2e} of the largest entry")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
