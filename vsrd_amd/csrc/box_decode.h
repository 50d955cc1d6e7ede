// The box decode's device functions that the frame kernels (frame_step.h) and the module path's decode kernels (box_decode.hip) share:
// single torch kernels each, written as ATen writes them.
#pragma once
#include <hip/hip_runtime.h>

namespace vsrd {

__device__ __forceinline__ float lerp_torch(float a, float b, float w) {           // ATen's lerp kernel
    const float diff = b - a;
    return (fabsf(w) < 0.5f) ? (a + w * diff) : (b - diff * (1.0f - w));
}
__device__ __forceinline__ float sigmoid_precise(float x) { return 1.0f / (1.0f + expf(-x)); }

// box_parameters.py:78-90: corner k = R_y (u_k * dim) + loc
__device__ __forceinline__ void unit_corner(int k, float* u) {
    const int table[8][3] = {{-1, -1, 1}, {1, -1, 1}, {1, -1, -1}, {-1, -1, -1}, {-1, 1, 1}, {1, 1, 1}, {1, 1, -1}, {-1, 1, -1}};
    u[0] = static_cast<float>(table[k][0]); u[1] = static_cast<float>(table[k][1]); u[2] = static_cast<float>(table[k][2]);
}

}  // namespace vsrd
