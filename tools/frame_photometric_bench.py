#!/usr/bin/env python3
"""What the photometric term costs in the frame loop (vsrd_amd.optimization.FrameOptimizer), at the reference's shape: 1 target + 16 source
views of 376x1408, N = 8, 1000 rays x 100 samples per step plus 100 photometric rays, residual phase.

Three loops on the same frame, all warmed before anything is timed, the graph loops measured alternately:
  * graph mode (captured fused glue), term off  -- the step of tools/native_mode_bench.py --graph --residual;
  * graph mode, term on                          -- vsrd_frame_photometric inside the captured step;
  * eager mode, term on                          -- the term composed from torch operators and autograd (the parity reference).
Every figure is ms per step over a window that ends in a device synchronisation: the median of five windows with the fastest and slowest.

  python tools/frame_photometric_bench.py [--steps 200] [--output profiles/r07/frame_photometric.txt]

--frame-batch B (several: --frame-batch 4 16): the term in a FrameBatch (FrameBatch(..., photometric=True): one
vsrd_frame_photometric_with_header call per step for the B frames) -- for every B a batch of B copies of the frame with the term off and one
with it on, beside ONE FrameOptimizer with the term on, the loops alternating; ms per FRAME-step (a window's time over steps x B).
  python tools/frame_photometric_bench.py --frame-batch 4 16 [--output profiles/r07/frame_photometric_batch.txt]

--parent-root DIR (with --frame-batch): DIR is a built checkout of the parent commit.  For every B the term-off batch step is then also
measured in child processes of their own -- this tree, the parent's, this tree, the parent's -- each a run of this file with
--term-off-batch B (and --root DIR for the parent's: the package, the header and the library are then DIR's), so that "a batch without
the term costs what it did" rests on numbers taken in the same call.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = ROOT
if "--root" in sys.argv:            # (a child of --parent-root: everything is imported from that tree)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)


def smooth_images(generator, V, H, W):
    """Six sinusoids of period 24-64 px per view and channel, in 0..1: texture a correlation can hold on to."""
    import math
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    images = torch.zeros(V, 3, H, W)
    for _ in range(6):
        period = torch.empty(V, 3, 1, 1).uniform_(24.0, 64.0, generator=generator)
        angle = torch.empty(V, 3, 1, 1).uniform_(0.0, 2.0 * math.pi, generator=generator)
        phase = torch.empty(V, 3, 1, 1).uniform_(0.0, 2.0 * math.pi, generator=generator)
        images += torch.sin(2.0 * math.pi * (x * torch.cos(angle) + y * torch.sin(angle)) / period + phase)
    return (images / 12.0 + 0.5).clamp(0.0, 1.0)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=200, help="steps per timed window of the graph loops")
    parser.add_argument("--eager-steps", type=int, default=20, help="steps per timed window of the eager loop")
    parser.add_argument("--instances", type=int, default=8)
    parser.add_argument("--views", type=int, default=17)
    parser.add_argument("--rays", type=int, default=1000)
    parser.add_argument("--surface-rays", type=int, default=100)
    parser.add_argument("--weight", type=float, default=0.1, help="loss_weights['photometric_loss'] of the loops with the term")
    parser.add_argument("--steps-per-graph", type=int, default=4)
    parser.add_argument("--frame-batch", type=int, nargs="*", default=[], help="measure the term in batches of these sizes instead of the three loops")
    parser.add_argument("--parent-root", default="", help="a built checkout of the parent commit: its term-off batch step beside this tree's")
    parser.add_argument("--term-off-batch", type=int, default=0, help=argparse.SUPPRESS)      # (the child processes of --parent-root)
    parser.add_argument("--root", default="", help=argparse.SUPPRESS)
    parser.add_argument("--output", default=None)
    args = parser.parse_args()
    if args.output is None:
        args.output = os.path.join(ROOT, "profiles", "r07", "frame_photometric_batch.txt" if args.frame_batch else "frame_photometric.txt")
    if not args.root:
        import __graft_entry__
        __graft_entry__.build()
    import bench
    from vsrd_amd import fields, losses, models, operations, optimization, rendering
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    V, H, W, N = args.views, 376, 1408, args.instances
    K, E, raw_loc, raw_dim, raw_ori = bench.synthetic_frame(0, V, H, W, N)
    det = models.BoxParameters3D(1, N).to(dev)
    with torch.no_grad():
        det.locations.copy_(raw_loc); det.dimensions.copy_(raw_dim); det.orientations.copy_(raw_ori)
        out = det()
        cam, dirs = rendering.ray_casting((H, W), K.to(dev), E.to(dev))
        block = fields.FieldBlock(fields.pack_instances(out["locations"][0], out["orientations"][0], out["dimensions"][0]), 0.1, None, None)
        origins = cam[:, None, None, :].expand(V, H, W, 3).reshape(-1, 3).contiguous()
        soft = rendering.render_hierarchical(block, origins, dirs.reshape(-1, 3), (0.0, 100.0), 64, 0.1, 1.0, seed=1,
                                             skip_exact_misses=True)["labels"].clamp(0, 1).reshape(V, H, W, N).contiguous()
        gt_boxes, _ = operations.project_boxes_multi_view(out["boxes_3d"][0], E.to(dev), K.to(dev), (H, W))
    images = smooth_images(torch.Generator().manual_seed(0), V, H, W).to(dev)
    inputs = optimization.FrameInputs((H, W), K.to(dev), E.to(dev), soft, gt_boxes, torch.ones(V, N, dtype=torch.bool, device=dev), images=images)

    def loop_of(weight, graph):
        cfg = optimization.OptimizationConfig(seed=0, num_rays=args.rays, surface_num_rays=args.surface_rays,
                                              loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": weight})
        loop = optimization.FrameOptimizer(inputs, cfg, dev, graph=graph)
        with torch.no_grad():
            loop.detector.locations.copy_(raw_loc); loop.detector.dimensions.copy_(raw_dim); loop.detector.orientations.copy_(raw_ori)
        loop.step_index = cfg.warmup_steps                # the residual phase, at its first step's schedule
        if graph:
            loop.step_tensor.fill_(loop.step_index)
        return loop

    def config_of(weight):
        return optimization.OptimizationConfig(seed=0, num_rays=args.rays, surface_num_rays=args.surface_rays,
                                               loss_weights={**losses.LOSS_WEIGHTS, "photometric_loss": weight})

    def batch_of(size, weight):
        batch = optimization.FrameBatch([inputs] * size, config_of(weight), dev, photometric=True)
        for member in batch.frames:
            with torch.no_grad():
                member.detector.locations.copy_(raw_loc); member.detector.dimensions.copy_(raw_dim); member.detector.orientations.copy_(raw_ori)
            member.step_index = batch.config.warmup_steps   # the residual phase, at its first step's schedule
            member.step_tensor.fill_(member.step_index)
        return batch

    if args.term_off_batch:             # a child process: one term-off batch (no keyword: the parent's FrameBatch has none), one line
        batch = optimization.FrameBatch([inputs] * args.term_off_batch, config_of(0.0), dev)
        for member in batch.frames:
            with torch.no_grad():
                member.detector.locations.copy_(raw_loc); member.detector.dimensions.copy_(raw_dim); member.detector.orientations.copy_(raw_ori)
            member.step_index = batch.config.warmup_steps
            member.step_tensor.fill_(member.step_index)
        batch.run(8 + args.steps_per_graph, args.steps_per_graph)
        values = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch.run(args.steps, args.steps_per_graph)
            torch.cuda.synchronize()
            values.append((time.perf_counter() - t0) / (args.steps * args.term_off_batch) * 1e3)
        ordered = sorted(values)
        print(f"TERM-OFF {ordered[2]:.3f}  [{ordered[0]:.3f} .. {ordered[-1]:.3f}]")
        batch.close()
        return

    if args.frame_batch:
        lines = [f"the photometric term in frame batches, residual phase: V={V}, {H}x{W}, N={N}, {args.rays} rays x 100 samples + {args.surface_rays} photometric "
                 f"rays, weight {args.weight}; ms per frame-step, median of five windows [fastest .. slowest], the loops alternating; "
                 f"{torch.cuda.get_device_name(0)}"]
        for size in args.frame_batch:
            loops = {f"FrameBatch of {size}, term off": (batch_of(size, 0.0), size), f"FrameBatch of {size}, term on": (batch_of(size, args.weight), size),
                     "one FrameOptimizer, term on": (loop_of(args.weight, True), 1)}
            for loop, _ in loops.values():
                loop.run(8 + args.steps_per_graph, args.steps_per_graph)
            torch.cuda.synchronize()
            windows = {name: [] for name in loops}
            for _ in range(5):
                for name, (loop, frames_of_loop) in loops.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loop.run(args.steps, args.steps_per_graph)
                    torch.cuda.synchronize()
                    windows[name].append((time.perf_counter() - t0) / (args.steps * frames_of_loop) * 1e3)
            for name, values in windows.items():
                ordered = sorted(values)
                lines.append(f"  {name:34s} {ordered[2]:8.3f}  [{ordered[0]:.3f} .. {ordered[-1]:.3f}]  ({args.steps} steps per window)")
            off, on = sorted(windows[f"FrameBatch of {size}, term off"])[2], sorted(windows[f"FrameBatch of {size}, term on"])[2]
            alone = sorted(windows["one FrameOptimizer, term on"])[2]
            lines.append(f"  B = {size}: the term adds {on - off:.3f} ms per frame-step to a {off:.3f} ms frame-step; one frame alone steps in {alone:.3f} ms with it")
            for loop, _ in loops.values():
                loop.close()
            del loops
            torch.cuda.empty_cache()
            if args.parent_root:
                import subprocess
                for turn in range(2):
                    for name, extra in (("this tree", []), ("the parent commit", ["--root", os.path.abspath(args.parent_root)])):
                        child = subprocess.run([sys.executable, os.path.join(HERE, "tools", "frame_photometric_bench.py"), "--term-off-batch", str(size),
                                                "--steps", str(args.steps), "--steps-per-graph", str(args.steps_per_graph), "--instances", str(N),
                                                "--views", str(V), "--rays", str(args.rays), *extra], capture_output=True, text=True, timeout=600)
                        found = [line for line in child.stdout.splitlines() if line.startswith("TERM-OFF ")]
                        if child.returncode != 0 or not found:
                            raise SystemExit(f"the term-off child of {name} failed:\n{child.stderr[-2000:]}")
                        lines.append(f"  FrameBatch of {size}, term off, a process of its own, {name:18s} turn {turn + 1}: {found[-1][len('TERM-OFF '):]}")
        text = "\n".join(lines)
        print(text)
        os.makedirs(os.path.dirname(args.output), exist_ok=True)
        with open(args.output, "w") as file:
            file.write(text + "\n")
        return

    loops = {"graph, term off": loop_of(0.0, True), "graph, term on": loop_of(args.weight, True), "eager, term on (torch operators)": loop_of(args.weight, False)}
    steps = {name: args.eager_steps if name.startswith("eager") else args.steps for name in loops}
    for name, loop in loops.items():                     # warm: the eager steps of graph mode, the captures, a window's worth of replays
        loop.run(8 + args.steps_per_graph if name.startswith("graph") else 3, args.steps_per_graph)
    torch.cuda.synchronize()
    windows = {name: [] for name in loops}
    last = {}
    for _ in range(5):
        for name, loop in loops.items():                 # alternating: the three share whatever else the machine does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = loop.run(steps[name], args.steps_per_graph)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / steps[name] * 1e3)
    lines = [f"frame loop with the photometric term, residual phase: V={V}, {H}x{W}, N={N}, {args.rays} rays x 100 samples + {args.surface_rays} photometric rays, "
             f"weight {args.weight}; ms per step, median of five windows [fastest .. slowest]; {torch.cuda.get_device_name(0)}"]
    for name, values in windows.items():
        ordered = sorted(values)
        converged = ""
        if "photometric_loss" in last[name]:
            converged = f"  photometric loss {float(last[name]['photometric_loss']):.4f}"
        lines.append(f"  {name:34s} {ordered[2]:8.3f}  [{ordered[0]:.3f} .. {ordered[-1]:.3f}]  ({steps[name]} steps per window){converged}")
    off, on = sorted(windows["graph, term off"])[2], sorted(windows["graph, term on"])[2]
    lines.append(f"  the term adds {on - off:.3f} ms to a {off:.3f} ms step in graph mode")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as file:
        file.write(text + "\n")
    for loop in loops.values():
        loop.close()


if __name__ == "__main__":
    main()
