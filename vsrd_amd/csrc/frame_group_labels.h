// vsrd_frame_group_labels: a frame's pseudo-labels in the views of its GROUP -- what tools/kitti_360/make_predictions.py:50-192 writes.  The
// group of a target frame is every frame of grouped_image_filenames.txt whose filtered instance-id set equals the target's
// (tools/kitti_360/sample_annotations.py:133,164-170): the frames a detector is later trained on.  It is NOT the set of views the frame was
// optimised on (the target plus the medians of at most 16 chunks of its source list, vsrd/datasets/kitti_360_dataset.py:192-197, of which a
// source needs only half the target's instances): sources outside the group would get labels, group frames outside the <= 32 views none,
// and the confidences would be means over the wrong views.  A group can hold thousands of frames, so the label views are tables of their
// own ([L,16] extrinsics, [L,9] intrinsics, [L,N,4] boxes, [L,N] visibility, L <= VSRD_MAX_LABEL_VIEWS) and the work is spread over the
// device in three kernels, ordered by the stream:
//
//   1. project   grid (ceil(L / 4), frames), four waves: a wave per label view (its 25 floats are wave-uniform), a lane per box.  Every
//                workgroup decodes the frame's n boxes into LDS (decode_box + world_corners: 64 lanes' work, cheaper than a pass through
//                memory), then project_pair -- the very function frame_labels_kernel runs -> camera_corners, boxes_2d
//   2. mean IoU  grid (ceil(n / 4), frames), four waves: a wave per prediction p, a lane per ground-truth slot g, so label_gt_boxes[l, g, :]
//                and label_visible[l, g] are contiguous across the wave and boxes_2d[l, p, :] is one broadcast.  Every lane sums ITS pair
//                over l = 0 .. l_f - 1 in ascending order (box_iou_or_zero where the view sees the slot): the float32 accumulation order
//                is the reference's and frame_labels_kernel's
//   3. assign    one wave per frame: -mean_iou into LDS, the solver of matching.h, matched_gt, confidences = the matched entries
//
// Steps, deviations (a slot no view sees: exactly 0.0) and the instance conventions are those of frame_labels.h.  The frame's own l_f sits in
// label_view_count (device, frame_stride apart like every other buffer; null: L), clamped to [1, L]; views l_f .. L - 1 and instances
// n_f .. N - 1 are never read and never written.  config->num_views and the header's view count are not read.
#pragma once
#include "frame_labels.h"

namespace vsrd {

constexpr int kGroupMaxViews = 4096;       // VSRD_MAX_LABEL_VIEWS
constexpr int kGroupWaves = 4, kGroupThreads = kGroupWaves * kWave;

struct GroupLabelBuffers {
    const float* raw_locations;      // [N,3]
    const float* raw_dimensions;     // [N,3]
    const float* raw_orientations;   // [N,2]
    const int* view_count;           // [1] or null
    const float* extrinsics;         // [L,16]
    const float* intrinsics;         // [L,9]
    const float* gt_boxes;           // [L,N,4]
    const unsigned char* visible;    // [L,N]
    float* camera_corners;           // out [L,N,8,3] or null
    float* boxes_2d;                 // out [L,N,4] (kernel 2 reads it back)
    float* mean_iou;                 // out [N,N] (kernel 3 reads it back)
    long long* matched_gt;           // out [N] or null
    float* confidences;              // out [N] or null
};

__device__ __forceinline__ void shift_frame(GroupLabelBuffers& b, long long shift) {
    b.raw_locations = of_frame(b.raw_locations, shift); b.raw_dimensions = of_frame(b.raw_dimensions, shift); b.raw_orientations = of_frame(b.raw_orientations, shift);
    b.view_count = of_frame(b.view_count, shift); b.extrinsics = of_frame(b.extrinsics, shift); b.intrinsics = of_frame(b.intrinsics, shift);
    b.gt_boxes = of_frame(b.gt_boxes, shift); b.visible = of_frame(b.visible, shift); b.camera_corners = of_frame(b.camera_corners, shift);
    b.boxes_2d = of_frame(b.boxes_2d, shift); b.mean_iou = of_frame(b.mean_iou, shift); b.matched_gt = of_frame(b.matched_gt, shift);
    b.confidences = of_frame(b.confidences, shift);
}

// l_f: the frame's own label views, a wave-uniform scalar clamped to [1, capacity]
__device__ __forceinline__ int group_views(const int* view_count, int capacity) {
    if (view_count == nullptr) return capacity;
    const int l = __builtin_amdgcn_readfirstlane(*view_count);
    return l < 1 ? 1 : (l > capacity ? capacity : l);
}

__global__ __launch_bounds__(kGroupThreads) void frame_group_project_kernel(FrameStepArgs a, GroupLabelBuffers b, int capacity) {
    if (a.frame_stride != 0) {             // a batch of frames (wave.h): blockIdx.y is the frame
        const long long shift = frame_shift(a.frame_stride, blockIdx.y);
        shift_frame(b, shift);
        a.header = of_frame(a.header, shift);
    }
    __shared__ float corners[kFrameMaxBoxes * 24];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & (kWave - 1);
    const int NS = a.num_boxes, L = group_views(b.view_count, capacity);
    const int n = a.header ? frame_count(a.header, NS) : NS;
    if (static_cast<int>(blockIdx.x) * kGroupWaves >= L) return;           // (the whole workgroup: the grid covers the capacity)
    if (tid < n) world_corners(decode_box(a, b.raw_locations + 3 * tid, b.raw_dimensions + 3 * tid, b.raw_orientations + 2 * tid), corners + tid * 24);
    __syncthreads();
    const int v = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kGroupWaves + tid / kWave);
    if (v >= L || lane >= n) return;
    float view[25];                        // (static indices after unrolling: registers, and scalar ones where the compiler proves the loads uniform)
#pragma unroll
    for (int r = 0; r < 16; ++r) view[r] = b.extrinsics[static_cast<size_t>(v) * 16 + r];
#pragma unroll
    for (int r = 0; r < 9; ++r) view[16 + r] = b.intrinsics[static_cast<size_t>(v) * 9 + r];
    const size_t pair = static_cast<size_t>(v) * NS + lane;
    float box[4];
    project_pair(view, corners + lane * 24, a.epsilon, a.height, a.width, b.camera_corners ? b.camera_corners + pair * 24 : nullptr, box);
#pragma unroll
    for (int k = 0; k < 4; ++k) b.boxes_2d[pair * 4 + k] = box[k];
}

__global__ __launch_bounds__(kGroupThreads) void frame_group_mean_iou_kernel(FrameStepArgs a, GroupLabelBuffers b, int capacity) {
    if (a.frame_stride != 0) {
        const long long shift = frame_shift(a.frame_stride, blockIdx.y);
        shift_frame(b, shift);
        a.header = of_frame(a.header, shift);
    }
    const int tid = static_cast<int>(threadIdx.x), g = tid & (kWave - 1);
    const int NS = a.num_boxes, L = group_views(b.view_count, capacity);
    const int n = a.header ? frame_count(a.header, NS) : NS;
    const int p = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kGroupWaves + tid / kWave);
    if (p >= n || g >= n) return;
    const float* predicted = b.boxes_2d + static_cast<size_t>(p) * 4;        // view l: + l NS 4, the same address in every lane
    const float* truth = b.gt_boxes + static_cast<size_t>(g) * 4;
    const unsigned char* seen = b.visible + g;
    float sum = 0.0f, count = 0.0f;
#pragma unroll 4
    for (int l = 0; l < L; ++l) {          // ascending: the reference's accumulation order (the loads do not depend on the sums)
        const size_t row = static_cast<size_t>(l) * NS;
        const float iou = box_iou_or_zero(predicted + row * 4, truth + row * 4);
        const bool sees = seen[row] != 0;  // (a select, not a branch: an unseen slot's term is dropped, never added)
        sum = sees ? sum + iou : sum;
        count = sees ? count + 1.0f : count;
    }
    b.mean_iou[p * NS + g] = count > 0.0f ? sum / count : 0.0f;
}

__global__ __launch_bounds__(kWave) void frame_group_assign_kernel(FrameStepArgs a, GroupLabelBuffers b) {
    if (a.frame_stride != 0) {             // one wave per frame
        const long long shift = frame_shift(a.frame_stride, blockIdx.x);
        shift_frame(b, shift);
        a.header = of_frame(a.header, shift);
    }
    __shared__ float negative_mean[kFrameMaxBoxes * kFrameMaxBoxes];    // [n,n]: the assignment's cost (the negation is exact)
    const int lane = static_cast<int>(threadIdx.x);
    const int NS = a.num_boxes;
    const int n = a.header ? frame_count(a.header, NS) : NS;
    for (int idx = lane; idx < n * n; idx += kWave) {
        const int p = idx / n, g = idx - p * n;
        negative_mean[idx] = -b.mean_iou[p * NS + g];
    }
    __syncthreads();
    const int col4row = lsap_rows_le_cols(negative_mean, n, n);
    if (lane < n) {
        if (b.matched_gt) b.matched_gt[lane] = col4row;
        if (b.confidences) b.confidences[lane] = -negative_mean[lane * n + col4row];
    }
}

}  // namespace vsrd
