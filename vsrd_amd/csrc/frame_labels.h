// vsrd_frame_labels: a frame's pseudo-labels from its arena row at the end of the optimisation -- what the reference produces in a second
// pass over the checkpoints (tools/kitti_360/make_predictions.py:61-192): decode the boxes, transform and project them into every view the
// row was optimised on (NOT the target's group of make_predictions.py:50-60: frame_group_labels.h labels that), torchvision.ops.box_iou
// against each view's ground-truth boxes, the mean over the views in which an instance exists,
// scipy.optimize.linear_sum_assignment(maximize=True), confidence = the matched mean IoU.  One workgroup of kFrameThreads per frame:
//
//   1. decode          decode_box + unit_corner (frame_step.h) on the frame's n boxes -> world corners (LDS)
//   2. project         every (view, box) pair, strided over the workgroup: camera corners = E_v corner / w (main.py:343-344), then
//                      project_box_3d with clip_lines_to_front over the 12 edges and clip_boxes_to_image (clip_edge / project_point of
//                      projection.h, the functions the prologue projects with) -> camera_corners, boxes_2d; the boxes stay in LDS
//   3. mean IoU        every (prediction p, ground-truth slot g): the views in ASCENDING order (the reference's accumulation order), where
//                      visible[v,g] add box_iou(boxes_2d[v,p], gt_boxes[v,g]) (vsrd_amd/formats.py::box_iou: no epsilon; a NaN, 0/0,
//                      counts as 0: the reference's nan_to_num) and count the view; mean_iou[p,g] = sum / count
//   4. assign          one wave: the n x n assignment on cost -mean_iou (scipy's maximize=True is that negation, which is exact) by the
//                      solver of matching.h, which reproduces scipy's result including ties; confidences[p] = mean_iou[p, matched_gt[p]]
//
// The ground-truth tables are in the target's instance order already (vsrd_frame_ingest / FrameInputs apply the source-to-target table of
// make_predictions.py:142-162), and the extrinsics are relative to the rectified target (make_predictions.py:74-109 is folded in).
//
// A stated deviation: a ground-truth slot that is visible in NO view (count = 0) gets mean_iou exactly 0.0 in its whole column.  The
// reference divides 0 by 0 there and hands scipy a NaN, which raises.  It happens when vsrd_frame_ingest finds a target entry without a
// set bit and takes it out of the table.
//
// Instances n_f .. N - 1 of a row laid out for a capacity N (a header, wave.h: mixed batches) are never read and never written, in any
// output -- the rows and columns of mean_iou beyond n_f included.  Likewise the views v_f .. V - 1 of a row laid out for a view capacity V
// (ABI 12): phases 2 and 3 cover the frame's own v_f views, the mean is over those among them that see the slot.
#pragma once
#include "frame_step.h"

namespace vsrd {

constexpr int kLabelMaxPairs = kFrameMaxViews * kFrameMaxBoxes;

struct LabelBuffers {
    const float* raw_locations;      // [N,3]
    const float* raw_dimensions;     // [N,3]
    const float* raw_orientations;   // [N,2]
    const float* extrinsics;         // [V,16]
    const float* intrinsics;         // [V,9]
    const float* gt_boxes;           // [V,N,4]
    const unsigned char* visible;    // [V,N] (by ground-truth instance)
    float* camera_corners;           // out [V,N,8,3] or null
    float* boxes_2d;                 // out [V,N,4] or null
    float* mean_iou;                 // out [N,N] or null
    long long* matched_gt;           // out [N] or null
    float* confidences;              // out [N] or null
};

__device__ __forceinline__ void shift_frame(LabelBuffers& b, long long shift) {
    b.raw_locations = of_frame(b.raw_locations, shift); b.raw_dimensions = of_frame(b.raw_dimensions, shift); b.raw_orientations = of_frame(b.raw_orientations, shift);
    b.extrinsics = of_frame(b.extrinsics, shift); b.intrinsics = of_frame(b.intrinsics, shift); b.gt_boxes = of_frame(b.gt_boxes, shift);
    b.visible = of_frame(b.visible, shift); b.camera_corners = of_frame(b.camera_corners, shift); b.boxes_2d = of_frame(b.boxes_2d, shift);
    b.mean_iou = of_frame(b.mean_iou, shift); b.matched_gt = of_frame(b.matched_gt, shift); b.confidences = of_frame(b.confidences, shift);
}

// project_box_3d + clip_boxes_to_image of one box from its eight camera-frame corners (geometric_operations.py:343-389, main.py:359-362):
// the forward half of the prologue's projection phase, without the record of which edge end gave each extreme.
__device__ __forceinline__ void clipped_box_2d(const float (&cam)[8][3], const float* K, float eps, float height, float width, float (&out)[4]) {
    const int edges[kBoxEdges][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};   // main.py:26-30
    float lo_u = 0.0f, lo_v = 0.0f, hi_u = 0.0f, hi_v = 0.0f;
    bool any = false;
#pragma unroll                                                   // (static corner indices: cam[] stays in registers)
    for (int e = 0; e < kBoxEdges; ++e) {
        const ClippedEdge c = clip_edge(cam[edges[e][0]], cam[edges[e][1]], eps);
        if (!c.front) continue;
        const EdgePoint pf = project_point(K, c.fx, c.fy, c.fz, eps, nullptr, nullptr);
        const EdgePoint pn = project_point(K, c.nx, c.ny, c.nz, eps, nullptr, nullptr);
        if (!any) {
            lo_u = hi_u = pf.u; lo_v = hi_v = pf.v;
            any = true;
        } else {
            lo_u = pf.u < lo_u ? pf.u : lo_u; lo_v = pf.v < lo_v ? pf.v : lo_v;
            hi_u = pf.u > hi_u ? pf.u : hi_u; hi_v = pf.v > hi_v ? pf.v : hi_v;
        }
        lo_u = pn.u < lo_u ? pn.u : lo_u; lo_v = pn.v < lo_v ? pn.v : lo_v;
        hi_u = pn.u > hi_u ? pn.u : hi_u; hi_v = pn.v > hi_v ? pn.v : hi_v;
    }
    out[0] = lo_u; out[1] = lo_v; out[2] = hi_u; out[3] = hi_v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                             // clip_boxes_to_image
        const float limit = (k & 1) ? height : width;
        if (out[k] < 0.0f) out[k] = 0.0f;
        if (out[k] > limit) out[k] = limit;
    }
}

// A decoded box's eight world corners (box_parameters.py:78-90) -> out [8,3]; shared with frame_group_labels.h like project_pair.
__device__ __forceinline__ void world_corners(const DecodedBox& d, float* out) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float u[3];
        unit_corner(k, u);
        const float lx = u[0] * d.dim[0], ly = u[1] * d.dim[1], lz = u[2] * d.dim[2];
        // (c lx + s lz and -s lx + c lz with the fused multiply-add SPELLED OUT: under -ffp-contract=fast the compiler picks which product of
        //  such a sum it fuses by the code around it, and the two kernels that share this function must round alike -- this is the form
        //  frame_labels_kernel has always been compiled to: the product with s rounded, the one with c fused)
        out[3 * k + 0] = __builtin_fmaf(d.c, lx, d.s * lz) + d.loc[0];
        out[3 * k + 1] = ly + d.loc[1];
        out[3 * k + 2] = __builtin_fmaf(d.c, lz, -d.s * lx) + d.loc[2];
    }
}

// One (view, box) pair, the body both vsrd_frame_labels and vsrd_frame_group_labels (frame_group_labels.h) run: camera corners = E corner / w
// (main.py:343-344) from the view's 25 floats `view` = (E [16], K [9]) and the box's eight world corners, written to `camera_out` ([8,3]) unless
// it is null, then the clipped 2-D box.
__device__ __forceinline__ void project_pair(const float* view, const float* corners, float eps, float height, float width, float* camera_out, float (&box)[4]) {
    const float* E = view;
    float cam[8][3];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float* c = corners + 3 * k;
        const float w = E[12] * c[0] + E[13] * c[1] + E[14] * c[2] + E[15];
#pragma unroll
        for (int j = 0; j < 3; ++j) cam[k][j] = (E[4 * j] * c[0] + E[4 * j + 1] * c[1] + E[4 * j + 2] * c[2] + E[4 * j + 3]) / w;
        if (camera_out) {
            float* o = camera_out + 3 * k;
            o[0] = cam[k][0]; o[1] = cam[k][1]; o[2] = cam[k][2];
        }
    }
    clipped_box_2d(cam, E + 16, eps, height, width, box);
}

// torchvision.ops.box_iou of one pair (vsrd_amd/formats.py::box_iou), NaN -> 0 (make_predictions.py: nan_to_num).  An infinite value
// (only a malformed ground-truth box, xmax < xmin, can produce one; the reference's scipy call raises on it) counts as 0 as well, so that
// the assignment's costs are always finite.
__device__ __forceinline__ float box_iou_or_zero(const float* a, const float* b) {
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]), area_b = (b[2] - b[0]) * (b[3] - b[1]);
    const float w = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.0f), h = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.0f);
    const float inter = w * h;
    const float iou = inter / (area_a + area_b - inter);
    return fabsf(iou) <= 3.0e38f ? iou : 0.0f;
}

__global__ __launch_bounds__(kFrameThreads) void frame_labels_kernel(FrameStepArgs a, LabelBuffers b) {
    if (a.frame_stride != 0) {             // a batch of frames (wave.h): one workgroup per frame
        const long long shift = frame_shift(a.frame_stride, blockIdx.x);
        shift_frame(b, shift);
        a.header = of_frame(a.header, shift);
    }
    __shared__ float corners[kFrameMaxBoxes * 24];
    __shared__ float view_matrices[kFrameMaxViews * 25];
    __shared__ float boxes[kLabelMaxPairs * 4];                         // [V,n,4]: phase 3 reads them here, no second projection
    __shared__ float negative_mean[kFrameMaxBoxes * kFrameMaxBoxes];    // [n,n]: the assignment's cost
    const int tid = static_cast<int>(threadIdx.x);
    // n: the boxes this frame has; NS: the stride of every instance axis (the capacity of a mixed batch, else n)
    // V: the views this frame has (wave.h: frame_views; rows v_f .. of camera_corners and boxes_2d are left alone)
    const int NS = a.num_boxes, V = frame_views(a.header, a.num_views);
    const int n = a.header ? frame_count(a.header, NS) : NS;
    for (int idx = tid; idx < V * 25; idx += kFrameThreads) {
        const int v = idx / 25, r = idx - 25 * v;
        view_matrices[idx] = r < 16 ? b.extrinsics[v * 16 + r] : b.intrinsics[v * 9 + (r - 16)];
    }
    // ---- 1. decode -> world corners (box_parameters.py:78-90) ------------------------------------------------------------------
    if (tid < n) {
        world_corners(decode_box(a, b.raw_locations + 3 * tid, b.raw_dimensions + 3 * tid, b.raw_orientations + 2 * tid), corners + tid * 24);
    }
    __syncthreads();
    // ---- 2. every (view, box) pair: camera corners, clipped 2-D box ------------------------------------------------------------------
    for (int idx = tid; idx < V * n; idx += kFrameThreads) {
        const int v = idx / n, p = idx - v * n;
        const size_t pair = static_cast<size_t>(v) * NS + p;
        float box[4];
        project_pair(view_matrices + v * 25, corners + p * 24, a.epsilon, a.height, a.width, b.camera_corners ? b.camera_corners + pair * 24 : nullptr, box);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            boxes[idx * 4 + k] = box[k];
            if (b.boxes_2d) b.boxes_2d[pair * 4 + k] = box[k];
        }
    }
    __syncthreads();
    // ---- 3. mean IoU of every (prediction, ground-truth slot) over the views that see the slot ----------------------------------------
    for (int idx = tid; idx < n * n; idx += kFrameThreads) {
        const int p = idx / n, g = idx - p * n;
        float sum = 0.0f, count = 0.0f;
        for (int v = 0; v < V; ++v) {
            if (b.visible[v * NS + g] == 0) continue;
            sum += box_iou_or_zero(boxes + (v * n + p) * 4, b.gt_boxes + (static_cast<size_t>(v) * NS + g) * 4);
            count += 1.0f;
        }
        const float mean = count > 0.0f ? sum / count : 0.0f;
        negative_mean[idx] = -mean;
        if (b.mean_iou) b.mean_iou[p * NS + g] = mean;
    }
    __syncthreads();
    // ---- 4. the assignment that maximises the matched mean IoU (matching.h) ------------------------------------------------------------
    if (tid < kWave) {                                     // wave 0 (all 64 lanes take part in the wave-cooperative solver)
        const int col4row = lsap_rows_le_cols(negative_mean, n, n);
        if (tid < n) {
            if (b.matched_gt) b.matched_gt[tid] = col4row;
            if (b.confidences) b.confidences[tid] = -negative_mean[tid * n + col4row];
        }
    }
}

}  // namespace vsrd
