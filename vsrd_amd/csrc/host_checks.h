// Host-side limits and argument checks that every translation unit of libvsrd_hip shares (api.hip, frame_surface.hip): a limit changed
// here changes in all of them.  Host code only -- nothing __device__, and nothing of namespace vsrd, which some units rename
// (split_front.hip, frame_surface.hip) -- so it means the same in each of them.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include "../../include/vsrd_hip.h"

namespace vsrd_host {

constexpr int kMaxBlocks = 16384;             // 256 CUs x 8 workgroups: many more workgroups than are resident: rays differ a lot in cost and the dispatcher is the load balancer (r01: 2048 -> 16384 workgroups = -12 % time); also sizes the partial buffer
constexpr int kMaxFrames = 1024;
constexpr int kFrameMaxViews = 32;            // the one view limit: the frame glue's tables (frame_step.h, frame_labels.h) and every entry point that takes a view of a frame
constexpr int kRunPixels = 64;                // a run: the pixels of an image row that one wave traces, a lane each (wave.h: kWave)

// VSRD_DEBUG: failed launches / LDS opt-ins are reported on stderr.  Read once, then a constant of the process.
inline bool debug() {
    static const bool frozen = getenv("VSRD_DEBUG") != nullptr;
    return frozen;
}

inline int launch_status() {
    const hipError_t error = hipGetLastError();
    if (error == hipSuccess) return VSRD_OK;
    if (debug()) fprintf(stderr, "libvsrd_hip: launch failed: %s\n", hipGetErrorString(error));
    return VSRD_E_LAUNCH;
}

inline bool valid_field(const vsrd_field* f) {
    return f != nullptr && f->instances != nullptr && f->num_instances >= 1 && f->num_instances <= VSRD_MAX_INSTANCES &&
           f->temperature > 0.0f;
}

// Frame batches (include/vsrd_hip.h, ABI 8): B copies of the one-frame grid along blockIdx.y, every pointer moved by frame_stride bytes per frame.
struct Frames {
    int count;              // B (1: one frame)
    long long stride;       // bytes; 0 for one frame (the kernels test this, not the count)
};
inline bool frames_of(int32_t num_frames, int64_t frame_stride, Frames* f) {
    f->count = num_frames <= 1 ? 1 : num_frames;
    f->stride = 0;
    if (f->count == 1) return true;
    if (f->count > kMaxFrames || frame_stride <= 0 || (frame_stride & 255) != 0) return false;
    f->stride = frame_stride;
    return true;
}

// "View `view` of a frame's `num_views` images of height x width, traced in `num_iterations` steps" (vsrd_frame_masks, vsrd_frame_surface):
// VSRD_E_INVALID_ARGUMENT for counts that name no such view, VSRD_E_UNSUPPORTED for an image whose pixel index leaves 30 bits.  The two
// are told apart because an entry point refuses its other invalid arguments before it calls an image unsupported.
inline int32_t image_view_status(int32_t num_views, int32_t view, int32_t height, int32_t width, int32_t num_iterations) {
    if (num_views < 1 || num_views > kFrameMaxViews || view < 0 || view >= num_views || height < 1 || width < 1 || num_iterations < 0)
        return VSRD_E_INVALID_ARGUMENT;
    return static_cast<int64_t>(height) * width >= (int64_t{1} << 30) ? VSRD_E_UNSUPPORTED : VSRD_OK;
}

// The runs of an image: every row in pieces of kRunPixels, the last one of a row a tail.
inline int image_runs(int32_t height, int32_t width) { return height * ((width + kRunPixels - 1) / kRunPixels); }

}  // namespace vsrd_host
