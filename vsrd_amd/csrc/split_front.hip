// Second translation unit of libvsrd_hip: the front kernels of vsrd_render_residual_step with the per-instance MLP's products on
// v_mfma_f32_16x16x32_bf16, both operands split into two bfloat16 parts (VSRD_FLAG_MLP_SPLIT_BF16; residual.h: forward_tile_split).
// Compiled WITHOUT -amdgpu-sched-strategy=iterative-ilp (see residual.h and __graft_entry__.py) and with the headers' namespace renamed,
// so that its copies of the kernels do not collide with api.hip's at link time.
#define VSRD_SPLIT_BF16 1
#define vsrd vsrd_split
#include "launch.h"
#undef vsrd

namespace vsrd_split_front {

int pack_images(const float* weights, int num_instances, int centred, unsigned* images, int frames, long long frame_stride, const void* frame_header,
                hipStream_t stream) {
    hipLaunchKernelGGL(vsrd_split::pack_mlp_images_kernel, dim3(num_instances, frames), dim3(256), 0, stream, weights, centred, images, frame_stride,
                       static_cast<const vsrd_split::FrameHeader*>(frame_header));
    return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

// (launch.h: this unit's copy of the dispatch that api.hip runs for the fp32 products)
int launch_front(const FrontLaunch& launch, hipStream_t stream, bool debug) { return vsrd_split::launch_front(launch, stream, debug); }

int launch_adjoint(int blocks, const float* instances, const float* images, int num_instances, const float* seeds, const unsigned char* masks,
                   long long slots_per_instance, long long used_slots, int items_per_instance, int slots_per_item, unsigned* next_item, float* item_rows,
                   unsigned char* item_flags, int frames, long long frame_stride, hipStream_t stream) {
    using namespace vsrd_split;
    const size_t lds = (static_cast<size_t>(kMlpImageWords) + static_cast<size_t>(kMlpSplitScratchTiles) * kTileFloats) * sizeof(float);
    hipLaunchKernelGGL(residual_mlp_adjoint_split_kernel, dim3(blocks, frames), dim3(kWave), lds, stream, instances, images, num_instances, 0u, seeds, masks,
                       slots_per_instance, used_slots, items_per_instance, slots_per_item, next_item, item_rows, item_flags, frame_stride);
    return hipGetLastError() == hipSuccess ? kOk : kLaunchFailed;
}

}  // namespace vsrd_split_front
