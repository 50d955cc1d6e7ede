#!/usr/bin/env python3
"""What the device-side second-order adjoint of a field call (vsrd_field_eval_adjoint, csrc/aux_kernels.h) buys at the photometric
branch's shape -- 100 points, 8 instances, hard union -- against the same quantity composed from torch operators on the device: the
route of rendering/generic.py for fields the kernels do not know, the field written in torch (oracle/fields.py on the device), the normal
by torch.autograd.grad(..., create_graph=True) as vsrd/rendering/renderers.py:100-109 takes it.  One call = surface_normal, a sum against
fixed weights, backward to locations, dimensions, rotations (and the MLP weights) and positions.  The arithmetic is tiny; what differs is
the launch count, so both the device time (events around the call) and the wall time (with a synchronisation behind it) are reported:
the median of five with the fastest and the slowest, after one warm-up call each, the two run in turns in one process.
    python tools/field_normals_bench.py [--out profiles/r07/field_normals.txt]"""
import argparse
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
    parser.add_argument("--points", type=int, default=100)
    parser.add_argument("--instances", type=int, default=8)
    parser.add_argument("--repetitions", type=int, default=5)
    args = parser.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from oracle import fields as ofields
    from vsrd_amd import fields, rendering
    dev = torch.device("cuda:0")
    P, N = args.points, args.instances
    g = torch.Generator().manual_seed(0)
    locations = torch.stack([torch.empty(N).uniform_(-6, 6, generator=g), torch.empty(N).uniform_(0.2, 1.2, generator=g),
                             torch.empty(N).uniform_(8, 30, generator=g)], -1)
    dimensions = torch.stack([torch.empty(N).uniform_(0.75, 1.0, generator=g), torch.empty(N).uniform_(0.75, 1.0, generator=g),
                              torch.empty(N).uniform_(1.5, 2.5, generator=g)], -1)
    yaws = torch.empty(N).uniform_(-3.1, 3.1, generator=g)
    rotations = torch.stack([torch.stack([torch.cos(yaws), torch.zeros(N), torch.sin(yaws)], -1), torch.tensor([0.0, 1.0, 0.0]).expand(N, 3),
                             torch.stack([-torch.sin(yaws), torch.zeros(N), torch.cos(yaws)], -1)], -2)
    mlp_weights = torch.randn(N, 1617, generator=g) * 0.1
    # points a little outside the boxes' faces and edges, where the normal depends on every parameter
    points = locations[torch.arange(P) % N] + torch.randn(P, 3, generator=g) * (dimensions[torch.arange(P) % N] + 0.3)
    weights = torch.randn(P, 3, generator=g).to(dev)

    def leaves(residual):
        tensors = [locations, dimensions, rotations] + ([mlp_weights] if residual else [])
        return [t.clone().to(dev).requires_grad_(True) for t in tensors], points.clone().to(dev).requires_grad_(True)

    def native(residual):
        params, pts = leaves(residual)
        loc, dim, rot = params[:3]

        def member(i):
            box = rendering.sdfs.box(dim[i])
            if residual:
                box = fields.residual_composition(box, fields.ResidualField(params[3][i]))
            return rendering.sdfs.translation(rendering.sdfs.rotation(fields.instance_field(box, i, N), rot[i]), loc[i])
        normals = rendering.surface_normal(fields.hard_union([member(i) for i in range(N)]), pts)
        return torch.autograd.grad((normals * weights).sum(), params + [pts])

    def composed(residual):
        params, pts = leaves(residual)
        union = ofields.InstanceUnion(params[0], params[2], params[1], 1.0, params[3] if residual else None)
        # the oracle writes the member gradient out analytically; the reference's route differentiates the distance instead
        distances, _ = union.instance_terms(pts)
        sdf = distances.min(dim=0).values
        gradient, = torch.autograd.grad(sdf.sum(), pts, create_graph=True)
        normals = torch.nn.functional.normalize(gradient, dim=-1)
        return torch.autograd.grad((normals * weights).sum(), params + [pts])

    def timed(call, residual):
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        out = call(residual)
        end.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, start.elapsed_time(end) * 1e-3, out

    calls = [(name, call, residual) for residual in (False, True) for name, call in (("native", native), ("composed", composed))]
    times = {(name, residual): [] for name, _, residual in calls}
    results = {}
    for repetition in range(args.repetitions + 1):
        for name, call, residual in calls:
            wall, device, results[(name, residual)] = timed(call, residual)
            if repetition:                          # (the first turn of each warms it up)
                times[(name, residual)].append((wall, device))

    def summary(values):
        return f"{1e3 * statistics.median(values):9.3f} [{1e3 * min(values):.3f} .. {1e3 * max(values):.3f}] ms"
    gap = lambda a, b: ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    lines = [f"# tools/field_normals_bench.py: {P} points, {N} instances, hard union; one call = surface_normal + a weighted sum + backward to the boxes, "
             f"the MLP weights (residual) and the positions",
             f"# median of {args.repetitions} [fastest .. slowest], the calls run in turns in one process; wall = host time with a synchronisation behind the call"]
    for residual in (False, True):
        kind = "residual" if residual else "box-only"
        for name, label in (("native", "vsrd_field_eval + vsrd_field_eval_adjoint"), ("composed", "torch operators, float32, autograd.grad(create_graph=True)")):
            t = times[(name, residual)]
            lines.append(f"{kind:9s} {label:58s} wall {summary([w for w, _ in t])}   device {summary([d for _, d in t])}")
        ratio = statistics.median([w for w, _ in times[("composed", residual)]]) / statistics.median([w for w, _ in times[("native", residual)]])
        worst = max(gap(a, b) for a, b in zip(results[("native", residual)], results[("composed", residual)]))
        lines.append(f"{kind:9s} wall, composed / native: {ratio:.1f} x (launch count, not throughput); native against composed: {worst:.2e} of the largest "
                     f"entry, the worst tensor")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as file:
            file.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
