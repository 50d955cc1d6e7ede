#!/usr/bin/env python3
"""Write K synthetic frame packs (vsrd_amd/frames.py) for `python -m vsrd_amd.launcher --frames-dir DIR`.  Host only, no GPU.

    python tools/make_frame_packs.py --out DIR --count 16 [--views 17 --height 376 --width 1408 --instances 8 | --instances 2,3,4]
                                     [--drop 1:0,2:1] [--shuffle] [--vertices 200] [--label-views 40]

Frame j is synthetic.synthetic_frame(seed = j) with instances[j % len(instances)] boxes.  Per view, an instance's polygon is the
integer-rounded convex hull of its true box's eight projected corners (clamped to the image), and its inside bits come from an
even-odd test at the pixel centres, plus the hull's own vertices, so that no entry is empty.

THIS IS NOT cv.fillPoly: OpenCV's LINE_8 fill also covers the boundary pixels, and cv.findContours would return the contour of the
filled mask, not a hull.  The packs written here exercise the ingest path and the launcher; real packs come from a dataset-side
exporter that runs the reference's own OpenCV steps (SoftRasterizer.make_polygon / make_binary_mask; INTEGRATION.md has the
recipe), which is out of scope of this repository.

--drop VIEW:SLOT[,...] removes the target's instance SLOT from source view VIEW (invisible there); --shuffle lists the entries of
every source view in a seeded random order: both exercise the visibility and the re-indexing of frames.collate_tables.

--label-views L gives every pack a GROUP (the label_* members of a pack: the frames that get the target's labels, `launcher
--group-predictions`): synthetic.synthetic_group, L cameras on the frame's trajectory between the sources' positions, the target among
them, with the true boxes' clipped 2-D boxes.  Without the flag the packs have no group."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def convex_hull(points):
    """Andrew's monotone chain over integer points [K,2] -> hull vertices [P,2] (P >= 1; collinear points dropped)."""
    unique = sorted({(int(x), int(y)) for x, y in points})
    if len(unique) <= 2:
        return np.asarray(unique, dtype=np.int32)

    def half(sequence):
        chain = []
        for p in sequence:
            while len(chain) >= 2 and (chain[-1][0] - chain[-2][0]) * (p[1] - chain[-2][1]) - (chain[-1][1] - chain[-2][1]) * (p[0] - chain[-2][0]) <= 0:
                chain.pop()
            chain.append(p)
        return chain[:-1]

    return np.asarray(half(unique) + half(reversed(unique)), dtype=np.int32)


def densify(polygon, vertices):
    """About `vertices` vertices on the same outline: every side gets its share of integer-rounded points between its ends (what
    cv.CHAIN_APPROX_NONE contours look like: hundreds of vertices, many of them collinear)."""
    if len(polygon) < 2 or vertices <= len(polygon):
        return polygon
    sides = np.roll(polygon, -1, axis=0) - polygon
    lengths = np.hypot(sides[:, 0], sides[:, 1])
    points = []
    for start, side, length in zip(polygon, sides, lengths):
        steps = max(1, int(round(vertices * length / max(lengths.sum(), 1.0))))
        points += [np.round(start + side * (k / steps)).astype(np.int32) for k in range(steps)]
    return np.asarray(points, dtype=np.int32)


def even_odd_mask(polygon, height, width):
    """[H,W] bool: pixel centres an odd number of polygon sides lie to the right of, plus the polygon's vertices themselves."""
    mask = np.zeros((height, width), dtype=bool)
    x0, y0 = polygon.min(0)
    x1, y1 = polygon.max(0)
    if len(polygon) >= 3:
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        crossings = np.zeros(ys.shape, dtype=np.int64)
        for (ax, ay), (bx, by) in zip(polygon, np.roll(polygon, -1, axis=0)):
            if ay == by:
                continue
            spans = (ay <= ys) != (by <= ys)
            at = ax + (ys - ay) * (float(bx) - float(ax)) / (float(by) - float(ay))
            crossings += spans & (xs < at)
        mask[y0:y1 + 1, x0:x1 + 1] = crossings % 2 == 1
    mask[polygon[:, 1], polygon[:, 0]] = True
    return mask


def make_pack(frame, views, height, width, instances, drop=(), shuffle=False, vertices=0, label_views=0, images=False):
    """The FramePack of synthetic frame number `frame`; `images`: with the views' colour images (synthetic.synthetic_images)."""
    from vsrd_amd import frames, models, synthetic
    K, E, raw_loc, raw_dim, raw_ori = synthetic.synthetic_frame(int(frame), views, height, width, instances)
    detector = models.BoxParameters3D(1, instances)
    with torch.no_grad():
        detector.locations.copy_(raw_loc); detector.dimensions.copy_(raw_dim); detector.orientations.copy_(raw_ori)
        corners = detector()["boxes_3d"][0].to(torch.float64)                                       # [N,8,3], the target camera's frame
    K, E = K.to(torch.float64), E.to(torch.float64)
    rng = np.random.default_rng(1000 + int(frame))
    dropped = {(int(v), int(n)) for v, n in drop}
    view_offsets, ids, polygons, masks = [0], [], [], []
    for view in range(views):
        camera = corners @ E[view, :3, :3].T + E[view, :3, 3]                                         # [N,8,3]
        order = list(range(instances))
        if shuffle and view > 0:
            order = [int(j) for j in rng.permutation(instances)]
        for n in order:
            if view > 0 and (view, n) in dropped:
                continue
            if float(camera[n, :, 2].min()) < 0.1:                                                     # (a box that reaches behind the camera: not in this view)
                if view == 0:
                    raise ValueError(f"synthetic frame {frame}: instance {n} reaches behind the target camera")
                continue
            image = camera[n] @ K[view].T
            points = torch.round(image[:, :2] / image[:, 2:3]).numpy().astype(np.int64)
            points[:, 0] = points[:, 0].clip(0, width - 1)
            points[:, 1] = points[:, 1].clip(0, height - 1)
            hull = convex_hull(points)
            ids.append(100 + 7 * n)                                                                    # (ids are labels, not indices)
            polygons.append(densify(hull, vertices))          # (the same outline: the inside bits stay the hull's)
            masks.append(np.packbits(even_odd_mask(hull, height, width), axis=-1))
        view_offsets.append(len(ids))
    polygon_offsets = np.concatenate([[0], np.cumsum([len(p) for p in polygons])])
    group = {key: value.numpy() for key, value in synthetic.synthetic_group(frame, height, width, label_views, corners).items()} if label_views else {}
    return frames.FramePack((height, width), K.numpy().astype(np.float32), E.numpy().astype(np.float32), np.asarray(view_offsets, dtype=np.int64),
                            np.asarray(ids, dtype=np.int64), polygon_offsets.astype(np.int64), np.concatenate(polygons).astype(np.int32), np.stack(masks),
                            boxes_3d=corners.numpy().astype(np.float32),      # (the true boxes in the target's instance order: ground truth for --metrics)
                            images=synthetic.synthetic_images(frame, views, height, width).numpy() if images else None, **group)


def write_packs(out, count, views=17, height=376, width=1408, instances=(8,), drop=(), shuffle=False, vertices=0, label_views=0, images=False):
    """Packs frame_000000.npz .. of frames 0..count-1 in `out`; returns their paths.  `views`: one count, or a list cycled over the frames
    like `instances` (frame j gets views[j % len(views)], each list with its own length)."""
    from vsrd_amd import frames
    os.makedirs(out, exist_ok=True)
    paths = []
    views = [int(views)] if isinstance(views, int) else [int(v) for v in views]
    for frame in range(int(count)):
        pack = make_pack(frame, views[frame % len(views)], height, width, int(instances[frame % len(instances)]), drop, shuffle, vertices, label_views, images)
        paths.append(os.path.join(out, f"frame_{frame:06d}.npz"))
        frames.save_pack(paths[-1], pack)
    return paths


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--out", required=True)
    parser.add_argument("--count", type=int, default=16)
    parser.add_argument("--views", default="17", help="one count or a comma list (frame j gets list[j %% len(list)])")
    parser.add_argument("--height", type=int, default=376)
    parser.add_argument("--width", type=int, default=1408)
    parser.add_argument("--instances", default="8", help="one count or a comma list (frame j gets list[j %% len(list)])")
    parser.add_argument("--drop", default="", help="VIEW:SLOT[,VIEW:SLOT...]: the target's instance SLOT is missing from source view VIEW")
    parser.add_argument("--vertices", type=int, default=0, help="subdivide every polygon to about this many vertices (real contours have hundreds)")
    parser.add_argument("--shuffle", action="store_true", help="source views list their entries in a seeded random order")
    parser.add_argument("--label-views", type=int, default=0, help="give every pack a group of this many label views (default: none)")
    parser.add_argument("--images", action="store_true",
                        help="give every pack the views' colour images ([V,3,H,W] uint8: the launcher's --photometric needs them; 27 MB per pack at 17 x 376 x 1408)")
    args = parser.parse_args(argv)
    drop = [tuple(int(x) for x in item.split(":")) for item in args.drop.split(",") if item]
    paths = write_packs(args.out, args.count, [int(x) for x in args.views.split(",")], args.height, args.width, [int(x) for x in args.instances.split(",")], drop, args.shuffle, args.vertices, args.label_views, args.images)
    print(f"{len(paths)} packs in {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
