// vsrd_frame_metrics: a frame's evaluation against its 3-D ground truth -- what the reference logs every `scalar_intervals` steps
// (scripts/main.py:870-924): for every matched (prediction, ground truth) pair rectify both boxes, turn them z-up, vsrd.operations.box_3d_iou
// (vsrd/operations/kitti360_operations.py:82-108) and from the IoUs iou_3d, iou_bev and the accuracies at 0.25 and 0.5.  One WAVE per frame,
// lane k handles pair k = (p = pd_indices[k], g = gt_indices[k]):
//
//   1. decode          decode_box + unit_corner (frame_step.h) on the frame's n boxes, lane b box b -> world corners (LDS, exported)
//   2. rectify, z-up   both boxes, float32: c' = Rect c as (R0 c0 + R1 c1) + R2 c2 with every product and sum rounded on its own (no FMA: the
//                      numbers can be reproduced on the host operation by operation), then (x, y, z) -> (x, z, -y)
//   3. box3dIou        in double on those float32 numbers, quirks kept as oracle/geometry.py::box_3d_iou has them: footprint = corners 3, 2, 1, 0;
//                      Sutherland-Hodgman with the strict `inside` test; crossings divide by determinant + 0.01; the intersection area is the
//                      area of the convex hull of the clipped polygon, capped by the smaller footprint; volumes from three edge lengths; heights
//                      from corners 0 and 4
//   4. summary         lane 0, pairs in ascending k, double: count, mean iou_3d, mean iou_bev, the shares of pairs with IoU > 0.25 / > 0.5
//
// Stated deviations.  (i) The reference turns the boxes z-up by multiplying with rotation_matrix_x(-pi/2) in float32, whose cosine is -4.37e-8
// and not 0; here the turn is the exact map.  The difference, together with the float32 rounding of the decode and the rectification, is
// what tests/test_hip_frame_metrics.py's end-to-end test measures.  (ii) A clipped polygon with fewer than three distinct points or a hull
// of zero area has area 0 (vsrd_amd/operations/kitti360_operations.py does the same); the reference's qhull raises there.
//
// The predicates and the crossing formula are evaluated as NumPy evaluates them: every product is rounded before it is added or subtracted
// (`rounded`), operands in the oracle's order.  `inside` compares two separately rounded products; contracted into an FMA one of them
// becomes exact, a vertex ON a clip line falls on the other side, and a box compared with itself comes out with an empty polygon, IoU 0.
// The library is built with -ffp-contract=fast, so the rounding is enforced per product and not by a pragma.
//
// A clip replaces every maximal run of dropped vertices by two crossings, P' <= P + floor(P / 2): 4 -> 6 -> 9 -> 13 -> 19.  Because of the
// + 0.01 the crossings do not lie on the clip line, so 8 is not a bound.  Every lane has two polygons of kMetricVertices = 20 in LDS (the
// second one holds the hull's chains afterwards): no per-lane array with a dynamic index lives in private memory.
//
// Instances n_f .. N - 1 of a row laid out for a capacity N (a header, wave.h: mixed batches) are never read and never written.
#pragma once
#include "frame_step.h"

namespace vsrd {

constexpr int kMetricVertices = 20;

struct MetricBuffers {
    const float* raw_locations;      // [N,3]
    const float* raw_dimensions;     // [N,3]
    const float* raw_orientations;   // [N,2]
    const float* gt_boxes_3d;        // [N,8,3]
    const float* rectification;      // [3,3] or null
    const long long* pd_indices;     // [N] or null (then gt_indices is null too): pair k = (k, k)
    const long long* gt_indices;     // [N]
    float* corners;                  // out [N,8,3] or null
    float* ious;                     // out [N,2]
    float* summary;                  // out [8]
};

__device__ __forceinline__ void shift_frame(MetricBuffers& b, long long shift) {
    b.raw_locations = of_frame(b.raw_locations, shift); b.raw_dimensions = of_frame(b.raw_dimensions, shift); b.raw_orientations = of_frame(b.raw_orientations, shift);
    b.gt_boxes_3d = of_frame(b.gt_boxes_3d, shift); b.rectification = of_frame(b.rectification, shift);
    b.pd_indices = of_frame(b.pd_indices, shift); b.gt_indices = of_frame(b.gt_indices, shift);
    b.corners = of_frame(b.corners, shift); b.ious = of_frame(b.ious, shift); b.summary = of_frame(b.summary, shift);
}

// The value as a register holds it: what is computed from it cannot be contracted with what computed it.
__device__ __forceinline__ double rounded(double v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float rounded(float v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ double product(double a, double b) { return rounded(a * b); }

struct Point2 { double x, y; };

// One lane's polygon: vertex v of lane l at [v * kWave + l] (16-byte entries, the lanes side by side).
struct LanePolygon {
    double2* base;
    __device__ __forceinline__ Point2 get(int v) const { const double2 p = base[v * kWave]; return {p.x, p.y}; }
    __device__ __forceinline__ void set(int v, Point2 p) const { if (v < kMetricVertices) base[v * kWave] = make_double2(p.x, p.y); }
};

// kitti360_operations.py:11-12 (oracle/geometry.py::clip_polygon.inside)
__device__ __forceinline__ bool metric_inside(Point2 p, Point2 previous, Point2 edge) {
    return product(edge.x, p.y - previous.y) > product(edge.y, p.x - previous.x);
}

// kitti360_operations.py:14-31 (oracle/geometry.py::clip_polygon.crossing)
__device__ __forceinline__ Point2 metric_crossing(Point2 s, Point2 e, Point2 previous, Point2 current) {
    const Point2 dc = {previous.x - current.x, previous.y - current.y}, dp = {s.x - e.x, s.y - e.y};
    const double n1 = rounded(product(previous.x, current.y) - product(previous.y, current.x));
    const double n2 = rounded(product(s.x, e.y) - product(s.y, e.x));
    const double n3 = 1.0 / (rounded(product(dc.x, dp.y) - product(dc.y, dp.x)) + 0.01);
    return {product(rounded(product(n1, dp.x) - product(n2, dc.x)), n3), product(rounded(product(n1, dp.y) - product(n2, dc.y)), n3)};
}

// 0.5 |dot(x, roll(y, 1)) - dot(y, roll(x, 1))| of a quadrilateral (oracle/geometry.py::box_3d_iou.shoelace)
__device__ __forceinline__ double quad_area(const Point2 (&f)[4]) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a += product(f[i].x, f[(i + 3) & 3].y);
        b += product(f[i].y, f[(i + 3) & 3].x);
    }
    return 0.5 * fabs(a - b);
}

__device__ __forceinline__ double cross_of(Point2 o, Point2 a, Point2 b) {
    return product(a.x - o.x, b.y - o.y) - product(a.y - o.y, b.x - o.x);
}

// Area of the convex hull of the `count` points of `points` (scipy's ConvexHull(...).volume in the reference): the points sorted by (x, y)
// in place, duplicates dropped, then the two monotone chains, each built in `chain` and summed as it stands (shoelace over its edges).
__device__ __forceinline__ double hull_area(const LanePolygon points, const LanePolygon chain, int count) {
    for (int i = 1; i < count; ++i) {                                   // insertion sort
        const Point2 p = points.get(i);
        int j = i;
        for (; j > 0; --j) {
            const Point2 q = points.get(j - 1);
            if (q.x < p.x || (q.x == p.x && q.y <= p.y)) break;
            points.set(j, q);
        }
        points.set(j, p);
    }
    int distinct = count > 0 ? 1 : 0;
    for (int i = 1; i < count; ++i) {
        const Point2 p = points.get(i), q = points.get(distinct - 1);
        if (p.x != q.x || p.y != q.y) points.set(distinct++, p);
    }
    if (distinct < 3) return 0.0;
    double twice = 0.0;
    for (int pass = 0; pass < 2; ++pass) {                              // lower chain left to right, upper chain right to left
        int k = 0;
        for (int step = 0; step < distinct; ++step) {
            const Point2 p = points.get(pass == 0 ? step : distinct - 1 - step);
            while (k >= 2 && cross_of(chain.get(k - 2), chain.get(k - 1), p) <= 0.0) --k;
            chain.set(k++, p);
        }
        for (int i = 1; i < k; ++i) {
            const Point2 a = chain.get(i - 1), b = chain.get(i);
            twice += product(a.x, b.y) - product(a.y, b.x);
        }
    }
    return 0.5 * fabs(twice);
}

__global__ __launch_bounds__(kWave) void frame_metrics_kernel(FrameStepArgs a, MetricBuffers b) {
    if (a.frame_stride != 0) {             // a batch of frames (wave.h): one wave per frame
        const long long shift = frame_shift(a.frame_stride, blockIdx.x);
        shift_frame(b, shift);
        a.header = of_frame(a.header, shift);
    }
    __shared__ double2 polygons[2 * kMetricVertices * kWave];
    __shared__ float corners[kFrameMaxBoxes * 24];
    __shared__ double pair_iou[kWave * 2];
    __shared__ int pair_valid[kWave];
    const int lane = static_cast<int>(threadIdx.x);
    const int NS = a.num_boxes;
    const int n = a.header ? frame_count(a.header, NS) : NS;
    // ---- 1. decode -> world corners (box_parameters.py:78-90), lane b box b ---------------------------------------------------------------
    if (lane < n) {
        const DecodedBox d = decode_box(a, b.raw_locations + 3 * lane, b.raw_dimensions + 3 * lane, b.raw_orientations + 2 * lane);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float u[3];
            unit_corner(k, u);
            const float lx = u[0] * d.dim[0], ly = u[1] * d.dim[1], lz = u[2] * d.dim[2];
            const float x = d.c * lx + d.s * lz + d.loc[0], y = ly + d.loc[1], z = -d.s * lx + d.c * lz + d.loc[2];
            corners[lane * 24 + 3 * k + 0] = x; corners[lane * 24 + 3 * k + 1] = y; corners[lane * 24 + 3 * k + 2] = z;
            if (b.corners) {
                float* o = b.corners + lane * 24 + 3 * k;
                o[0] = x; o[1] = y; o[2] = z;
            }
        }
    }
    pair_valid[lane] = 0;
    __syncthreads();
    // ---- 2./3. pair `lane` ------------------------------------------------------------------------------------------------------------------
    long long p = lane, g = lane;
    if (lane < n && b.pd_indices) { p = b.pd_indices[lane]; g = b.gt_indices[lane]; }
    if (lane < n && p >= 0 && p < n && g >= 0 && g < n) {
        float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        if (b.rectification) {
#pragma unroll
            for (int j = 0; j < 9; ++j) R[j] = b.rectification[j];
        }
        // of each box: corners 0, 1, 2, 3 and 4, rectified and z-up (all the metric reads), as doubles
        double pd[5][3], gt[5][3];
        bool annotated = true;
        const float* pc = corners + static_cast<int>(p) * 24;
        const float* gc = b.gt_boxes_3d + g * 24;
        for (int j = 0; j < 24; ++j) annotated = annotated && fabsf(gc[j]) <= 3.4028234e38f;      // (false for NaN and infinities)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                const float* c = (which == 0 ? pc : gc) + 3 * k;
                const float c0 = c[0], c1 = c[1], c2 = c[2];
                float r[3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    r[j] = rounded(rounded(rounded(R[3 * j] * c0) + rounded(R[3 * j + 1] * c1)) + rounded(R[3 * j + 2] * c2));
                double (&o)[3] = which == 0 ? pd[k] : gt[k];
                o[0] = static_cast<double>(r[0]); o[1] = static_cast<double>(r[2]); o[2] = static_cast<double>(-r[1]);
            }
        }
        if (annotated) {
            const LanePolygon first = {polygons + lane}, second = {polygons + kMetricVertices * kWave + lane};
            Point2 f1[4], f2[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f1[i] = {pd[3 - i][0], pd[3 - i][1]};
                f2[i] = {gt[3 - i][0], gt[3 - i][1]};
            }
            const double area1 = quad_area(f1), area2 = quad_area(f2);
            // Sutherland-Hodgman: the prediction's footprint clipped by every edge of the ground truth's
            LanePolygon source = first, output = second;
#pragma unroll
            for (int i = 0; i < 4; ++i) source.set(i, f1[i]);
            int count = 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (count > 0) {
                    const Point2 previous = f2[(j + 3) & 3], current = f2[j];
                    const Point2 edge = {current.x - previous.x, current.y - previous.y};
                    int out = 0;
                    Point2 s = source.get(count - 1);
                    bool s_in = metric_inside(s, previous, edge);
                    for (int i = 0; i < count; ++i) {
                        const Point2 e = source.get(i);
                        const bool e_in = metric_inside(e, previous, edge);
                        if (e_in != s_in) output.set(out++, metric_crossing(s, e, previous, current));
                        if (e_in) output.set(out++, e);
                        s = e; s_in = e_in;
                    }
                    count = out < kMetricVertices ? out : kMetricVertices;
                    const LanePolygon t = source; source = output; output = t;
                }
            }
            double inter_area = count > 0 ? hull_area(source, output, count) : 0.0;
            inter_area = fmin(fmin(area1, area2), inter_area);
            const double iou_bev = inter_area / (area1 + area2 - inter_area);
            const double height = fmax(0.0, fmin(pd[0][2], gt[0][2]) - fmax(pd[4][2], gt[4][2]));
            const double inter_volume = inter_area * height;
            double volumes[2];
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                const double (&c)[5][3] = which == 0 ? pd : gt;
                double lengths[3];
                const int ends[3][2] = {{0, 1}, {1, 2}, {0, 4}};
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const double dx = c[ends[e][0]][0] - c[ends[e][1]][0], dy = c[ends[e][0]][1] - c[ends[e][1]][1], dz = c[ends[e][0]][2] - c[ends[e][1]][2];
                    lengths[e] = sqrt(product(dx, dx) + product(dy, dy) + product(dz, dz));
                }
                volumes[which] = lengths[0] * lengths[1] * lengths[2];
            }
            const double iou_3d = inter_volume / (volumes[0] + volumes[1] - inter_volume);
            pair_iou[2 * lane] = iou_3d; pair_iou[2 * lane + 1] = iou_bev;
            pair_valid[lane] = 1;
            b.ious[2 * p] = static_cast<float>(iou_3d); b.ious[2 * p + 1] = static_cast<float>(iou_bev);
        } else {
            const float nan = __builtin_nanf("");
            b.ious[2 * p] = nan; b.ious[2 * p + 1] = nan;
        }
    }
    __syncthreads();
    // ---- 4. summary: the pairs with an annotation, ascending, in double (main.py:908-915) ---------------------------------------------------
    if (lane == 0) {
        double count = 0.0, sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < n; ++k) {
            if (pair_valid[k] == 0) continue;
            const double i3 = pair_iou[2 * k], ib = pair_iou[2 * k + 1];
            count += 1.0;
            sums[0] += i3; sums[1] += ib;
            sums[2] += i3 > 0.25 ? 1.0 : 0.0; sums[3] += ib > 0.25 ? 1.0 : 0.0;
            sums[4] += i3 > 0.5 ? 1.0 : 0.0; sums[5] += ib > 0.5 ? 1.0 : 0.0;
        }
        b.summary[0] = static_cast<float>(count);
#pragma unroll
        for (int j = 0; j < 6; ++j) b.summary[1 + j] = count > 0.0 ? static_cast<float>(sums[j] / count) : 0.0f;
        b.summary[7] = 0.0f;
    }
}

}  // namespace vsrd
