// BoxParameters3D.forward() and its autograd backward (vsrd_amd/models.py) as two kernels: raw locations / dimensions / orientations
// -> decoded boxes AND the packed instance block the render kernels read (fields.pack_instances), and the cotangents of those outputs
// -> the three raw gradients.  Eager torch spends ~35 element-wise launches of 4-5 us on this per optimisation step, every one of them on
// the step's dependent chain.
//
// The arithmetic is torch's, op for op and in torch's order, so that a module on this path computes what the eager module computes:
//   sigmoid              1 / (1 + exp(-x))                                  backward  (g (1 - y)) y
//   lerp(lo, hi, w)      ATen's two-sided form (lerp_torch)                 backward  g (hi - lo)         (only the weight has a gradient)
//   F.normalize          x / max(sqrt(x0 x0 + x1 x1), 1e-12)                backward  div, clamp_min, vector_norm as autograd chains them
//   yaw_matrix           (c 0 s | 0 1 0 | -s 0 c) with exact 0 and 1        backward  g_c = G00 + G22, g_s = G02 - G20
//   decode_box_3d        (u_k * dim) @ R^T + loc                            backward  the matmul's two products, the broadcasts' sums
// Each line of the list is a kernel of its own in eager torch, so nothing is contracted ACROSS two of them here: fp contract is off in the
// functions below, and this translation unit is compiled with hipcc's own -ffp-contract=fast-honor-pragmas (__graft_entry__.py), as
// torch's kernels are -- under the library's -ffp-contract=fast the backend fuses every multiply-add it finds, the pragma
// notwithstanding and inside expf's expansion too (measured: the sigmoid then differs from torch's in a fifth of the values, by up to
// 3 ulp; the norm in 3 %).  lerp_torch and sigmoid_precise (box_decode.h, shared with the frame kernels) are single torch kernels.
// One thread per box, one workgroup (N <= VSRD_MAX_INSTANCES).
#include <hip/hip_runtime.h>
#include "../../include/vsrd_hip.h"
#include "box_decode.h"

namespace vsrd {

constexpr int kBoxDecodeThreads = 64;
static_assert(kBoxDecodeThreads >= VSRD_MAX_INSTANCES, "one thread per box");

// F.normalize(raw, dim=-1) of a heading: the norm, its clamp and the unit vector
struct BoxHeading { float norm, denom, c, s; };
__device__ __forceinline__ BoxHeading box_heading(float x0, float x1) {
#pragma clang fp contract(off)
    BoxHeading h;
    h.norm = sqrtf(x0 * x0 + x1 * x1);
    h.denom = fmaxf(h.norm, 1.0e-12f);
    h.c = x0 / h.denom;
    h.s = x1 / h.denom;
    return h;
}

// row-major rotation about y
__device__ __forceinline__ void yaw_rows(float c, float s, float* R) {
    R[0] = c; R[1] = 0.0f; R[2] = s; R[3] = 0.0f; R[4] = 1.0f; R[5] = 0.0f; R[6] = -s; R[7] = 0.0f; R[8] = c;
}

// raw_* [N,3 / 3 / 2], ranges [2,3] (lo | hi)  ->  block [N,16] = loc | R | dim | 0, locations [N,3], dimensions [N,3], orientations [N,3,3],
// boxes_3d [N,8,3]
__global__ __launch_bounds__(kBoxDecodeThreads) void box_decode_forward_kernel(const float* __restrict__ raw_locations, const float* __restrict__ raw_dimensions,
                                                                               const float* __restrict__ raw_orientations, const float* __restrict__ location_range,
                                                                               const float* __restrict__ dimension_range, int N, float* __restrict__ block,
                                                                               float* __restrict__ locations, float* __restrict__ dimensions,
                                                                               float* __restrict__ orientations, float* __restrict__ boxes_3d) {
#pragma clang fp contract(off)
    const int i = threadIdx.x;
    if (i >= N) return;
    float loc[3], dim[3], R[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        loc[j] = lerp_torch(location_range[j], location_range[3 + j], sigmoid_precise(raw_locations[3 * i + j]));
        dim[j] = lerp_torch(dimension_range[j], dimension_range[3 + j], sigmoid_precise(raw_dimensions[3 * i + j]));
    }
    const BoxHeading h = box_heading(raw_orientations[2 * i], raw_orientations[2 * i + 1]);
    yaw_rows(h.c, h.s, R);
    float* row = block + 16 * i;
#pragma unroll
    for (int j = 0; j < 3; ++j) { row[j] = loc[j]; row[12 + j] = dim[j]; locations[3 * i + j] = loc[j]; dimensions[3 * i + j] = dim[j]; }
#pragma unroll
    for (int j = 0; j < 9; ++j) { row[3 + j] = R[j]; orientations[9 * i + j] = R[j]; }
    row[15] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float u[3];
        unit_corner(k, u);
        const float corner[3] = {u[0] * dim[0], u[1] * dim[1], u[2] * dim[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {            // the matmul's dot product as a chain of fused multiply-adds, then the broadcast add
            const float dot = __fmaf_rn(corner[2], R[3 * r + 2], __fmaf_rn(corner[1], R[3 * r + 1], corner[0] * R[3 * r]));
            boxes_3d[24 * i + 3 * k + r] = dot + loc[r];
        }
    }
}

// The cotangents (any of them may be null: that output was not used) -> grad_raw_locations [N,3], grad_raw_dimensions [N,3],
// grad_raw_orientations [N,2].  The block's, the tensor's own and the corners' contributions to a decoded value are added in that order.
__global__ __launch_bounds__(kBoxDecodeThreads) void box_decode_backward_kernel(const float* __restrict__ raw_locations, const float* __restrict__ raw_dimensions,
                                                                                const float* __restrict__ raw_orientations, const float* __restrict__ location_range,
                                                                                const float* __restrict__ dimension_range, int N, const float* __restrict__ grad_block,
                                                                                const float* __restrict__ grad_locations, const float* __restrict__ grad_dimensions,
                                                                                const float* __restrict__ grad_orientations, const float* __restrict__ grad_boxes_3d,
                                                                                float* __restrict__ grad_raw_locations, float* __restrict__ grad_raw_dimensions,
                                                                                float* __restrict__ grad_raw_orientations) {
#pragma clang fp contract(off)
    const int i = threadIdx.x;
    if (i >= N) return;
    float g_loc[3] = {0.0f, 0.0f, 0.0f}, g_dim[3] = {0.0f, 0.0f, 0.0f}, g_R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool any = false;                            // (the first contribution is taken as it is: 0 + g would turn a -0 into +0)
    auto add = [&](float* acc, float g, bool first) { *acc = first ? g : *acc + g; };
    if (grad_block) {
        const float* row = grad_block + 16 * i;
        for (int j = 0; j < 3; ++j) { add(g_loc + j, row[j], !any); add(g_dim + j, row[12 + j], !any); }
        for (int j = 0; j < 9; ++j) add(g_R + j, row[3 + j], !any);
        any = true;
    }
    bool any_loc = any, any_dim = any, any_R = any;
    if (grad_locations) { for (int j = 0; j < 3; ++j) add(g_loc + j, grad_locations[3 * i + j], !any_loc); any_loc = true; }
    if (grad_dimensions) { for (int j = 0; j < 3; ++j) add(g_dim + j, grad_dimensions[3 * i + j], !any_dim); any_dim = true; }
    if (grad_orientations) { for (int j = 0; j < 9; ++j) add(g_R + j, grad_orientations[9 * i + j], !any_R); any_R = true; }
    const BoxHeading h = box_heading(raw_orientations[2 * i], raw_orientations[2 * i + 1]);
    float sig_l[3], sig_d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { sig_l[j] = sigmoid_precise(raw_locations[3 * i + j]); sig_d[j] = sigmoid_precise(raw_dimensions[3 * i + j]); }
    if (grad_boxes_3d) {
        // boxes = (u * dim) @ R^T + loc:  g_loc = sum_k g_k,  g_corner_k = g_k @ R,  g_dim = sum_k u_k * g_corner_k,  g_R[r][c] = sum_k g_k[r] corner_k[c]
        float R[9], dim[3];
        yaw_rows(h.c, h.s, R);
        for (int j = 0; j < 3; ++j) dim[j] = lerp_torch(dimension_range[j], dimension_range[3 + j], sig_d[j]);
        float b_loc[3] = {0.0f, 0.0f, 0.0f}, b_dim[3] = {0.0f, 0.0f, 0.0f}, b_R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float u[3];
            unit_corner(k, u);
            const float* g = grad_boxes_3d + 24 * i + 3 * k;
            const float corner[3] = {u[0] * dim[0], u[1] * dim[1], u[2] * dim[2]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                b_loc[c] += g[c];
                const float g_corner = __fmaf_rn(g[2], R[6 + c], __fmaf_rn(g[1], R[3 + c], g[0] * R[c]));
                b_dim[c] += u[c] * g_corner;
#pragma unroll
                for (int r = 0; r < 3; ++r) b_R[3 * r + c] = __fmaf_rn(g[r], corner[c], b_R[3 * r + c]);
            }
        }
        for (int j = 0; j < 3; ++j) { add(g_loc + j, b_loc[j], !any_loc); add(g_dim + j, b_dim[j], !any_dim); }
        for (int j = 0; j < 9; ++j) add(g_R + j, b_R[j], !any_R);
    }
    // lerp (weight only), then sigmoid
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float gl = g_loc[j] * (location_range[3 + j] - location_range[j]);
        const float gd = g_dim[j] * (dimension_range[3 + j] - dimension_range[j]);
        grad_raw_locations[3 * i + j] = (gl * (1.0f - sig_l[j])) * sig_l[j];
        grad_raw_dimensions[3 * i + j] = (gd * (1.0f - sig_d[j])) * sig_d[j];
    }
    // yaw_matrix, then F.normalize = x / clamp_min(vector_norm(x), eps).expand_as(x)
    const float x[2] = {raw_orientations[2 * i], raw_orientations[2 * i + 1]};
    const float g_h[2] = {g_R[0] + g_R[8], g_R[2] + (-g_R[6])};
    const float g_denom = (-g_h[0]) * ((x[0] / h.denom) / h.denom) + (-g_h[1]) * ((x[1] / h.denom) / h.denom);      // div w.r.t. the divisor, summed by the expand
    const float g_norm = (h.norm >= 1.0e-12f) ? g_denom : 0.0f;                                                    // clamp_min
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float direction = (h.norm == 0.0f) ? 0.0f : x[j] / h.norm;                                           // vector_norm: grad * (x / norm), 0 where the norm is 0
        grad_raw_orientations[2 * i + j] = g_h[j] / h.denom + g_norm * direction;
    }
}

}  // namespace vsrd

extern "C" {

int32_t vsrd_box_decode_forward(const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                                const float* location_range, const float* dimension_range, int32_t num_instances,
                                float* instances, float* locations, float* dimensions, float* orientations, float* boxes_3d, void* stream) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES || !raw_locations || !raw_dimensions || !raw_orientations || !location_range || !dimension_range ||
        !instances || !locations || !dimensions || !orientations || !boxes_3d)
        return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(vsrd::box_decode_forward_kernel, dim3(1), dim3(vsrd::kBoxDecodeThreads), 0, static_cast<hipStream_t>(stream), raw_locations, raw_dimensions,
                       raw_orientations, location_range, dimension_range, num_instances, instances, locations, dimensions, orientations, boxes_3d);
    return hipGetLastError() == hipSuccess ? VSRD_OK : VSRD_E_LAUNCH;
}

int32_t vsrd_box_decode_backward(const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                                 const float* location_range, const float* dimension_range, int32_t num_instances,
                                 const float* grad_instances, const float* grad_locations, const float* grad_dimensions,
                                 const float* grad_orientations, const float* grad_boxes_3d,
                                 float* grad_raw_locations, float* grad_raw_dimensions, float* grad_raw_orientations, void* stream) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES || !raw_locations || !raw_dimensions || !raw_orientations || !location_range || !dimension_range ||
        !grad_raw_locations || !grad_raw_dimensions || !grad_raw_orientations)
        return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(vsrd::box_decode_backward_kernel, dim3(1), dim3(vsrd::kBoxDecodeThreads), 0, static_cast<hipStream_t>(stream), raw_locations, raw_dimensions,
                       raw_orientations, location_range, dimension_range, num_instances, grad_instances, grad_locations, grad_dimensions, grad_orientations,
                       grad_boxes_3d, grad_raw_locations, grad_raw_dimensions, grad_raw_orientations);
    return hipGetLastError() == hipSuccess ? VSRD_OK : VSRD_E_LAUNCH;
}

}  // extern "C"
