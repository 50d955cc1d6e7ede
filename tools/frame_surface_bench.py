#!/usr/bin/env python3
"""Dense surface renders of B frames at 376 x 1408, N = 8: (a) the composition of the public entry points, per frame -- sphere_tracing on
every pixel, evaluate_field (gradient and labels), F.normalize, the arg-max label, the range, shadow_rendering (a second trace on every
pixel), phong_shading, the blend over a photograph, quantisation and two packbits -- against (b) ONE vsrd_frame_surface launch for all B
frames, same outputs.  The soft union on both sides (the composition takes the instance from its labels).  Box-only and residual fields,
B = 1 and B = 16, median of five timed repetitions with the fastest and the slowest, after two warm-up repetitions; device time by events
around the whole repetition.  Also prints the share of pixels whose trace converged (the pixels that reach steps 2-4 of (b)).
    python tools/frame_surface_bench.py [--out profiles/r07/frame_surface.txt] [--height 376 --width 1408]"""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T = 8, 0.1
TRACE = (1000, 0.01, 100.0)
ALPHA = 0.6


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
    from vsrd_amd.rendering import renderers
    lib, dev = _lib.load(), torch.device("cuda:0")
    H, W = args.height, args.width
    R, row_bytes = H * W, (W + 7) // 8
    lines = [f"# tools/frame_surface_bench.py: {H} x {W}, N = {N}, soft union T = {T}, trace {TRACE}, median of five [fastest .. slowest], ms per call for all B frames"]
    one = lambda values: torch.tensor(values, device=dev)
    shading = dict(light_ambient=(1.0, 1.0, 1.0), light_diffuse=(1.0, 1.0, 1.0), light_specular=(1.0, 1.0, 1.0), material_ambient=(0.1, 0.1, 0.1),
                   material_specular=(0.3, 0.3, 0.3), material_emission=(0.0, 0.0, 0.0), shininess=32.0)
    for residual in (False, True):
        for B in (1, 16):
            f32, u8 = torch.float32, torch.uint8
            buffers = (("instances", (N, 16), f32), ("cam", (1, 3), f32), ("dirs", (R, 3), f32), ("mlp", (N, _lib.MLP_WEIGHTS), f32), ("light", (3,), f32),
                       ("palette", (N, 3), f32), ("background", (R, 3), u8), ("converged_bits", (H, row_bytes), u8), ("shadow_bits", (H, row_bytes), u8),
                       ("instance", (R,), u8), ("range", (R,), f32), ("colors", (R, 3), u8))
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
                rows[f]["light"].copy_(torch.tensor(renderers.SURFACE_LIGHT))
                rows[f]["palette"].copy_(renderers.surface_palette(N))
                rows[f]["background"].copy_(synthetic.synthetic_images(f, 1, H, W)[0].permute(1, 2, 0).reshape(R, 3))
                if residual:
                    rows[f]["mlp"].copy_(renderers._centre_mlp_torch(0.05 * torch.randn(N, _lib.MLP_WEIGHTS, generator=torch.Generator().manual_seed(f))))
            last = {}

            def composition():
                for f in range(B):
                    row = rows[f]
                    block = fields.FieldBlock(row["instances"], T, row["mlp"] if residual else None, None, False)
                    directions, light = row["dirs"], row["light"].expand(R, 3)
                    positions, converged = rendering.sphere_tracing(block, row["cam"][0], directions, TRACE[0], TRACE[1], bounding_radius=TRACE[2], initialization=False)
                    _, labels, gradients = rendering.evaluate_field(block, positions, with_gradients=True, with_labels=True)
                    normals = torch.nn.functional.normalize(gradients, dim=-1)
                    owner = labels.argmax(dim=-1)
                    distance = (positions - row["cam"][0]).norm(dim=-1)
                    shadow = renderers.shadow_rendering(block, positions, normals, light, TRACE[0], TRACE[1], converged, bounding_radius=TRACE[2])
                    lit, dark = (rendering.phong_shading(directions, normals, light, one(shading["light_ambient"]), scale * one(shading["light_diffuse"]),
                                                         scale * one(shading["light_specular"]), one(shading["material_ambient"]), row["palette"][owner],
                                                         one(shading["material_specular"]), one(shading["material_emission"]), shading["shininess"]) for scale in (1.0, 0.0))
                    colour = torch.where(shadow, dark, lit)
                    back = row["background"].to(f32) / 255.0
                    image = torch.where(converged, ALPHA * colour + (1.0 - ALPHA) * back, back)
                    row["colors"].copy_((255.0 * image + 0.5).to(u8))
                    row["instance"].copy_(torch.where(converged[:, 0], owner, torch.full_like(owner, 255)).to(u8))
                    row["range"].copy_(distance * converged[:, 0])
                    row["converged_bits"].copy_(packbits(converged.view(H, W)))
                    row["shadow_bits"].copy_(packbits(shadow.view(H, W)))
                    last["converged"] = converged

            def fused():
                field = _lib.Field(N, T, rows[0]["instances"].data_ptr(), rows[0]["mlp"].data_ptr() if residual else None)
                config = _lib.make_config(0, 2, (0.0, 1.0), 1.0, 1.0, 1.0e-6, 3, frames=(B, stride) if B > 1 else None)
                surface = renderers.surface_config(0, 1, H, W, *TRACE, TRACE[1], hard=False, shadows=True, background=True, alpha=ALPHA, **shading)
                row = rows[0]
                _lib.check(lib.vsrd_frame_surface(field, config, surface, pointer(row["cam"]), pointer(row["dirs"]), pointer(row["light"]), pointer(row["palette"]),
                                                  pointer(row["background"]), pointer(row["converged_bits"]), pointer(row["shadow_bits"]), pointer(row["instance"]),
                                                  pointer(row["range"]), pointer(row["colors"]), None, None, None, _lib.stream()))
            a, b = timed(composition), timed(fused)
            share = float(last["converged"].float().mean())
            lines.append(f"{'residual' if residual else 'box-only'} B = {B:2d}: (a) composition {a[0]:9.3f} [{a[1]:.3f} .. {a[2]:.3f}]   (b) vsrd_frame_surface {b[0]:9.3f} [{b[1]:.3f} .. {b[2]:.3f}]"
                         f"   pixels that reached steps 2-4 in the last frame: {100.0 * share:.1f} %")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
