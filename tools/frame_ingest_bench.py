#!/usr/bin/env python3
"""One row's INPUT PHASE at the reference's size (17 views of 376 x 1408, N = 8), two ways, host-to-device copies included:

  (a) materialised: the path without frame packs -- transforms.soft_masks over the V x N polygons (vsrd_polygon_soft_masks, [B,H,W]), the
      torch re-index / permute / stack to a FrameInputs [V,H,W,N], boxes from the masks, then FrameBatch.reset (strided copy into the
      row, amax).  It starts from the entries' [B,H,W] bool masks in host memory (what a dataset without packs would hold: 72 MB
      per frame, copied to the device inside the timing); unpacking them from the pack's bits is NOT timed;
  (b) in place: FrameBatch.reset from the pack (vsrd_frame_ingest writes the row).

Both include what reset() does after its inputs block (fresh parameters, Adam state, sampling table).  Rows of capacity 8 and 13, once
with the synthetic packs' own polygons (a handful of vertices: the pixel pass is bound by its stores) and once with every polygon
subdivided to about --vertices vertices (real contours have hundreds: the side loop is what is timed).
Each figure: the median of --repeats runs after one warm-up, with the fastest and slowest run, so the spread is on record next to it.

    python tools/frame_ingest_bench.py [--repeats 5] [--out profiles/r07/frame_ingest.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)


def host_masks(pack):
    """(table, chosen entries, their [B,H,W] bool masks in host memory): prepared outside every timing."""
    from vsrd_amd import frames
    table = frames.collate_tables(pack)
    chosen = [int(e) for e in table.reshape(-1) if e >= 0]
    return table, chosen, torch.from_numpy(np.unpackbits(pack.inside[chosen], axis=-1)[:, :, :pack.image_size[1]].astype(bool))


def materialise(pack, device, unpacked):
    """(a)'s first half: a FrameInputs from the pack's polygons and the host masks with the per-polygon kernel and torch."""
    from vsrd_amd import frames, optimization, transforms
    H, W = pack.image_size
    V, N = pack.num_views, pack.num_instances
    table, chosen, masks_on_host = unpacked
    polygons = [torch.from_numpy(pack.polygon_vertices[pack.polygon_offsets[e]:pack.polygon_offsets[e + 1]]).to(device) for e in chosen]
    inside = masks_on_host.to(device)                                                                                # [B,H,W] bool
    soft = transforms.soft_masks(polygons, inside, frames.TEMPERATURE)                                               # [B,H,W]
    index = torch.full((V * N,), len(chosen), dtype=torch.int64)
    index[torch.from_numpy(table.reshape(-1) >= 0)] = torch.arange(len(chosen))
    index = index.to(device)
    padded = torch.cat([soft, soft.new_zeros(1, H, W)])                                                              # (the zero padding index -1 selects)
    masks = padded[index].view(V, N, H, W).permute(0, 2, 3, 1).contiguous()                                          # [V,H,W,N]
    rows, columns = inside.any(dim=2), inside.any(dim=1)                                                             # [B,H], [B,W]
    first = lambda t: t.to(torch.uint8).argmax(dim=1)
    last = lambda t: t.shape[1] - 1 - t.flip(1).to(torch.uint8).argmax(dim=1)
    boxes = torch.stack([first(columns), first(rows), last(columns), last(rows)], -1).to(torch.float32)
    seen = rows.any(dim=1)
    boxes = torch.cat([boxes * seen[:, None], boxes.new_zeros(1, 4)])[index].view(V, N, 2, 2)
    visible = torch.cat([seen, seen.new_zeros(1)])[index].view(V, N)
    intrinsics, extrinsics = frames.camera_matrices(pack, device)
    return optimization.FrameInputs((H, W), intrinsics, extrinsics, masks * visible[:, None, None, :], boxes, visible)


def timed(action, repeats):
    action()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        action()
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples), min(samples), max(samples)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--views", type=int, default=17)
    parser.add_argument("--height", type=int, default=376)
    parser.add_argument("--width", type=int, default=1408)
    parser.add_argument("--instances", type=int, default=8)
    parser.add_argument("--capacities", default="8,13")
    parser.add_argument("--vertices", type=int, default=200, help="vertices per polygon of the second pass")
    parser.add_argument("--out", default="")
    args = parser.parse_args(argv)
    import __graft_entry__
    __graft_entry__.build()
    import make_frame_packs
    from vsrd_amd import frames, optimization
    device = torch.device("cuda:0")
    lines = [f"# tools/frame_ingest_bench.py: one row's input phase, {args.views} x {args.height} x {args.width}, N = {args.instances}, synthetic packs, "
             f"median of {args.repeats} after one warm-up [fastest .. slowest], seconds, host-to-device copies included",
             "# (a) starts from [B,H,W] bool masks in host memory (their unpacking is not timed) and copies them to the device; (b) starts from the pack"]
    for vertices in (0, args.vertices):
        packs = [make_frame_packs.make_pack(frame, args.views, args.height, args.width, args.instances, vertices=vertices) for frame in (0, 1)]
        unpacked = [host_masks(pack) for pack in packs]
        counts = np.diff(packs[0].polygon_offsets)
        lines.append(f"# polygons of {int(counts.min())}..{int(counts.max())} vertices (mean {counts.mean():.0f})")
        founder = frames.ingest(packs[0], device)
        check = materialise(packs[0], device, unpacked[0])
        agree = float((check.soft_masks - founder.soft_masks).abs().max())
        same = torch.equal(check.boxes_2d, founder.boxes_2d) and torch.equal(check.visible_masks, founder.visible_masks)
        lines.append(f"# the two paths agree: max |soft (a) - soft (b)| = {agree:.2e}, boxes and visibility equal: {same}")
        for capacity in (int(c) for c in args.capacities.split(",")):
            batch = optimization.FrameBatch([founder], optimization.OptimizationConfig(), device, max_instances=capacity)
            turn = [0]

            def reset_a():
                turn[0] += 1
                assert batch.reset(0, materialise(packs[turn[0] % 2], device, unpacked[turn[0] % 2]), init_seed=turn[0])

            def reset_b():
                turn[0] += 1
                assert batch.reset(0, packs[turn[0] % 2], init_seed=turn[0])

            def only_materialise():
                turn[0] += 1
                materialise(packs[turn[0] % 2], device, unpacked[turn[0] % 2])

            def only_ingest():
                turn[0] += 1
                member = batch.frames[0]
                frames.ingest_into(packs[turn[0] % 2], device, capacity, soft_masks=member.flat_masks, sampling_weights=member.sampling_weights,
                                   gt_boxes=member._glue["gt_boxes"], visible=member._glue["visible"])

            for label, action in (("(a) materialise + FrameBatch.reset(FrameInputs)", reset_a), ("(b) FrameBatch.reset(FramePack)", reset_b),
                                  ("    (a)'s materialise alone", only_materialise), ("    (b)'s vsrd_frame_ingest alone (copies + both kernels)", only_ingest)):
                median, fastest, slowest = timed(action, args.repeats)
                lines.append(f"capacity {capacity:2d}  {label:58s} {median:8.4f}  [{fastest:.4f} .. {slowest:.4f}]")
            batch.close()
            del batch
            torch.cuda.empty_cache()
    resources = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout.splitlines()
    lines.append("# kernel resources (tools/kernel_resources.py)")
    lines += [line for line in resources if line.startswith("kernel") or "frame_ingest" in line]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            handle.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
