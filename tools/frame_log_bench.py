#!/usr/bin/env python3
"""What the device-side log (vsrd_frame_log, csrc/frame_log.h) costs a batch of frames: ONE FrameBatch of B = 16 frames through all 3000
steps of the reference's schedule (1000 box-only, 2000 residual) at the reference's intervals -- scalars every 50 steps, a snapshot every
500 -- against the same batch without the log.  Same process, same box, the two batches built and captured up front and run in turns
(off, on, off, on, ...): one warm-up run each, then the median of five timed runs with the fastest and the slowest.  A run is timed from
after the rows' resets to a device synchronisation behind the last replay.  Reported: frame-steps per second, and the `log` phase -- the
host time of the log's launches between the replays.  The two batches' final parameters are compared bit for bit (the log changes nothing).
    python tools/frame_log_bench.py [--out profiles/r07/frame_log.txt] [--frames 16] [--views 17] [--instances 8] [--distinct 4]"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="")
    parser.add_argument("--frames", type=int, default=16)
    parser.add_argument("--views", type=int, default=17)
    parser.add_argument("--instances", type=int, default=8)
    parser.add_argument("--height", type=int, default=376)
    parser.add_argument("--width", type=int, default=1408)
    parser.add_argument("--num-steps", type=int, default=3000)
    parser.add_argument("--warmup-steps", type=int, default=1000)
    parser.add_argument("--scalar-interval", type=int, default=50)
    parser.add_argument("--ckpt-interval", type=int, default=500)
    parser.add_argument("--distinct", type=int, default=4, help="distinct synthetic frames, served to the rows in turn")
    parser.add_argument("--repetitions", type=int, default=5)
    args = parser.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import launcher, optimization
    dev = torch.device("cuda:0")
    B = args.frames
    distinct = [launcher.synthetic_frame_inputs(dev, f, args.views, args.instances, args.height, args.width) for f in range(min(args.distinct, B))]
    frames = [distinct[f % len(distinct)] for f in range(B)]
    plain = optimization.OptimizationConfig(num_steps=args.num_steps, warmup_steps=args.warmup_steps, seed=0)
    configs = {"off": plain, "on": dataclasses.replace(plain, scalar_interval=args.scalar_interval, checkpoint_interval=args.ckpt_interval)}
    batches = {}
    for name, config in configs.items():
        batches[name] = optimization.FrameBatch(frames, config, dev, init_seeds=list(range(B)))
        batches[name].capture_all()
    torch.cuda.synchronize()

    def run(name):
        batch = batches[name]
        for f in range(B):
            assert batch.reset(f, frames[f], init_seed=f)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.run(args.num_steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, batch.frames[0].log_seconds

    times = {name: [] for name in batches}
    for repetition in range(args.repetitions + 1):
        for name in ("off", "on"):
            seconds, log_seconds = run(name)
            if repetition:                          # (the first turn of each warms it up)
                times[name].append((seconds, log_seconds))
    identical = all(torch.equal(p.data, q.data) for a, b in zip(batches["off"].frames, batches["on"].frames)
                    for module in ("detector", "hyper_distance_field") for p, q in zip(getattr(a, module).parameters(), getattr(b, module).parameters()))
    history = batches["on"].history()[0]
    snapshots = batches["on"].snapshots()[0]
    counters = [m._log["counters"].tolist() for m in batches["on"].frames]
    work = B * args.num_steps

    def summary(values):
        return f"{statistics.median(values):10.4f} [{min(values):.4f} .. {max(values):.4f}]"
    off, on = [t for t, _ in times["off"]], [t for t, _ in times["on"]]
    lines = [f"# tools/frame_log_bench.py: one FrameBatch of {B} frames ({args.views} views, {args.height} x {args.width}, {args.instances} instances, 1000 rays, 100 samples), "
             f"{args.num_steps} steps ({args.warmup_steps} box-only), scalars every {args.scalar_interval}, a snapshot every {args.ckpt_interval} steps",
             f"# median of {args.repetitions} [fastest .. slowest], the two batches run in turns in one process",
             f"without the log: seconds per batch   {summary(off)}   frame-steps/s {summary([work / t for t in off])}",
             f"with the log:    seconds per batch   {summary(on)}   frame-steps/s {summary([work / t for t in on])}",
             f"with the log:    `log` phase (host time of the log launches between the replays), seconds per batch {summary([l for _, l in times['on']])}",
             f"difference of the medians: {statistics.median(on) - statistics.median(off):+.4f} s = {100.0 * (statistics.median(on) / statistics.median(off) - 1.0):+.2f} %; "
             f"spread of the runs without the log: {max(off) - min(off):.4f} s",
             f"rows logged per frame {int(history['steps'].numel())}, snapshots per frame {len(snapshots)}, counters of every frame (rows, dropped, slots, dropped) "
             f"{'all ' + str(counters[0]) if all(c == counters[0] for c in counters) else counters}",
             f"snapshot slot: {batches['on'].frames[0]._log['slot_floats']} floats = {4 * batches['on'].frames[0]._log['slot_floats'] / 2 ** 20:.2f} MiB",
             f"final parameters of the two batches bit-identical: {identical}"]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")
    for batch in batches.values():
        batch.close()


if __name__ == "__main__":
    main()
