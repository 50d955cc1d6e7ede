#!/usr/bin/env python3
"""Dense predicted masks of B frames at 376 x 1408, N = 8: (a) the composition the library offered before vsrd_frame_masks, per frame --
vsrd_render_hierarchical_forward on every pixel + vsrd_sphere_trace + torch multiply, threshold and packbits -- against (b) ONE
vsrd_frame_masks launch for all B frames.  Box-only and residual fields, B = 1 and B = 16, median of five timed repetitions with the fastest
and the slowest, after two warm-up repetitions; device time by events around the whole repetition.  Also prints the share of pixels whose
trace converged (the pixels (b) renders at all).
    python tools/frame_masks_bench.py [--out profiles/r07/frame_masks.txt] [--height 376 --width 1408]"""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, S, T, STD, RATIO = 8, 100, 0.1, 0.1, 1.0
TRACE = (1000, 0.01, 100.0)


def pointer(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def packbits(mask):
    """numpy.packbits along the last axis with torch ops (most significant bit first, zero padding)."""
    pad = (-mask.shape[-1]) % 8
    mask = torch.nn.functional.pad(mask, (0, pad)).unflatten(-1, (-1, 8)).to(torch.uint8)
    weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=mask.device)
    return (mask * weights).sum(-1, dtype=torch.uint8)


def timed(run, repetitions=5, warmup=2):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(repetitions):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times), min(times), max(times)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="")
    parser.add_argument("--height", type=int, default=376)
    parser.add_argument("--width", type=int, default=1408)
    args = parser.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from vsrd_amd import _lib, fields, models, optimization, rendering, synthetic
    lib, dev = _lib.load(), torch.device("cuda:0")
    H, W = args.height, args.width
    R, row_bytes = H * W, (W + 7) // 8
    lines = [f"# tools/frame_masks_bench.py: {H} x {W}, N = {N}, S = {S}, trace {TRACE}, median of five [fastest .. slowest], ms per call for all B frames"]
    for residual in (False, True):
        for B in (1, 16):
            f32 = torch.float32
            buffers = (("instances", (N, 16), f32), ("cam", (1, 3), f32), ("dirs", (R, 3), f32), ("mlp", (N, _lib.MLP_WEIGHTS), f32), ("inside", (N, H, row_bytes), torch.uint8))
            size = lambda shape, dtype: (math.prod(shape) * torch.empty((), dtype=dtype).element_size() + 255) // 256 * 256
            arena = optimization.FrameArena(B, sum(size(shape, dtype) for _, shape, dtype in buffers), dev)
            rows = [{name: row.new(shape, dtype, fill=0) for name, shape, dtype in buffers} for row in arena.rows]
            stride = arena.stride
            for f in range(B):
                K, E, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(f, 1, H, W, N)
                det = models.BoxParameters3D(1, N)
                with torch.no_grad():
                    det.locations.copy_(raw_loc); det.dimensions.copy_(raw_dim); det.orientations.copy_(raw_ori)
                    out = det()
                cam, dirs = rendering.ray_casting((H, W), K.to(dev), E.to(dev))
                rows[f]["instances"].copy_(fields.pack_instances(out["locations"][0], out["orientations"][0], out["dimensions"][0]))
                rows[f]["cam"].copy_(cam)
                rows[f]["dirs"].copy_(dirs.reshape(-1, 3))
                if residual:
                    rows[f]["mlp"].copy_(0.05 * torch.randn(N, _lib.MLP_WEIGHTS, generator=torch.Generator().manual_seed(f)))
            labels = torch.empty(R, N, device=dev)
            positions, converged = torch.empty(R, 3, device=dev), torch.empty(R, dtype=torch.uint8, device=dev)

            def field_of(f):
                return _lib.Field(N, T, rows[f]["instances"].data_ptr(), rows[f]["mlp"].data_ptr() if residual else None)

            def composition():
                for f in range(B):
                    field, cam, dirs = field_of(f), rows[f]["cam"], rows[f]["dirs"]
                    config = _lib.make_config(R, S, (0.0, 100.0), STD, RATIO, 1.0e-6, 0, seed=1)
                    _lib.check(lib.vsrd_render_hierarchical_forward(field, config, pointer(cam), pointer(dirs), None, None, pointer(labels), None, None, None, None, None, None, _lib.stream()))
                    _lib.check(lib.vsrd_sphere_trace(field, pointer(cam), 0, pointer(dirs), None, R, TRACE[0], TRACE[1], TRACE[2], 0, 0, pointer(positions), pointer(converged), _lib.stream()))
                    mask = (labels * converged[:, None].to(torch.float32)) > 0.5
                    rows[f]["inside"].copy_(packbits(mask.view(H, W, N).permute(2, 0, 1)))

            def fused():
                config = _lib.make_config(0, S, (0.0, 100.0), STD, RATIO, 1.0e-6, 3, seed=1, frames=(B, stride) if B > 1 else None)
                masks = _lib.FrameMasksConfig(0, 1, H, W, TRACE[0], TRACE[1], TRACE[2], 0.5, N)
                _lib.check(lib.vsrd_frame_masks(field_of(0), config, masks, pointer(rows[0]["cam"]), pointer(rows[0]["dirs"]),
                                                None, None, None, None, pointer(rows[0]["inside"]), None, None, None, _lib.stream()))
            a, b = timed(composition), timed(fused)
            share = float(converged.float().mean())
            lines.append(f"{'residual' if residual else 'box-only'} B = {B:2d}: (a) composition {a[0]:9.3f} [{a[1]:.3f} .. {a[2]:.3f}]   (b) vsrd_frame_masks {b[0]:9.3f} [{b[1]:.3f} .. {b[2]:.3f}]"
                         f"   pixels rendered by (b) in the last frame: {100.0 * share:.1f} %")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
