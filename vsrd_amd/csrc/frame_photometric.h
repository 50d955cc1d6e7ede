// vsrd_frame_photometric: the glue between the library launches of one frame's photometric term (scripts/main.py:689-853) -- the gather of
// the drawn rays, the Newton step of sphere_tracing(differentiable=True) (renderers.py:59-72), F.normalize of the hard union's gradient, the
// two adjoints of those and the accumulation into the render step's gradients.  One lane per ray (tails: any R), no LDS, no atomics; what
// sits between the glue kernels -- the trace, the field evaluations and their adjoints, the patch correlation -- are the library's own
// launches, issued by the entry point (api.hip) in stream order.
//
// The forward glue repeats torch's roundings, operator by operator, so that p1, n and with them the loss carry the BITS of the autograd
// composition rendering.sphere_tracing(differentiable=True) -> rendering.surface_normal -> losses.patch_correlation_loss: the hard union's
// normal is discontinuous at box edges and arg-min switches, an ulp in p1 is not harmless.  Every product and every sum is rounded on its
// own (`rounded`, frame_metrics.h: the library is built with -ffp-contract=fast, a pragma would not hold), and a sum over the three
// components is taken as ATen's reduction takes it for an inner dimension of 3 -- two lanes per output, lane 0 (x0 + x2), lane 1 x1, then
// the two partial sums: (x0 + x2) + x1.  Division and square root are the correctly rounded ones on both sides.
// The adjoint glue follows autograd's formulas; its roundings are free (its results are held to float64 bounds, not to bits).
//
// A batch of frames (vsrd_frame_photometric_with_header; wave.h): B copies of the one-frame grid along blockIdx.y, every pointer moved by
// frame_stride bytes per frame when frame_stride != 0, as in the step kernels.  Nothing else differs between the copies.
#pragma once
#include "frame_metrics.h"

namespace vsrd {

constexpr int kPhotometricThreads = 256;
constexpr int kPhotometricMaxRays = 2048;      // the table sampler's limit (ray_sampling.h)

// ATen's sum over an inner dimension of 3 (see above).
__device__ __forceinline__ float sum3_as_aten(float x0, float x1, float x2) { return rounded(rounded(x0 + x2) + x1); }
__device__ __forceinline__ float dot3_as_aten(const float* a, const float* b) {
    return sum3_as_aten(rounded(a[0] * b[0]), rounded(a[1] * b[1]), rounded(a[2] * b[2]));
}

// directions[r] = ray_directions[idx], pixels[r] = (idx % W, idx / W); lane 0 of the launch writes the backward's grad_loss = 1.
__global__ __launch_bounds__(kPhotometricThreads) void photometric_gather_kernel(int num_rays, int width, const long long* __restrict__ ray_indices,
                                                                                 const float* __restrict__ ray_directions, float* __restrict__ directions,
                                                                                 int* __restrict__ pixels, float* __restrict__ one, long long frame_stride) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(ray_indices, shift); VSRD_OF_FRAME_NONNULL(ray_directions, shift); VSRD_OF_FRAME_NONNULL(directions, shift);
        VSRD_OF_FRAME_NONNULL(pixels, shift); VSRD_OF_FRAME_NONNULL(one, shift);
    }
    const int r = static_cast<int>(blockIdx.x * kPhotometricThreads + threadIdx.x);
    if (r == 0) one[0] = 1.0f;
    if (r >= num_rays) return;
    const long long index = ray_indices[r];
    for (int k = 0; k < 3; ++k) directions[3 * r + k] = ray_directions[3 * index + k];
    pixels[2 * r] = static_cast<int>(index % width);
    pixels[2 * r + 1] = static_cast<int>(index / width);
}

// renderers.py:59-72 with the normal g0 as a constant: step = -d0 / sum(g0 * r), p1 = where(converged, p0 + r * step, p0).  `slopes` keeps
// g0 . r for the adjoint.
__global__ __launch_bounds__(kPhotometricThreads) void photometric_newton_kernel(int num_rays, const float* __restrict__ p0, const unsigned char* __restrict__ converged,
                                                                                 const float* __restrict__ d0, const float* __restrict__ g0,
                                                                                 const float* __restrict__ directions, float* __restrict__ p1, float* __restrict__ slopes,
                                                                                 long long frame_stride) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(p0, shift); VSRD_OF_FRAME_NONNULL(converged, shift); VSRD_OF_FRAME_NONNULL(d0, shift); VSRD_OF_FRAME_NONNULL(g0, shift);
        VSRD_OF_FRAME_NONNULL(directions, shift); VSRD_OF_FRAME_NONNULL(p1, shift); VSRD_OF_FRAME_NONNULL(slopes, shift);
    }
    const int r = static_cast<int>(blockIdx.x * kPhotometricThreads + threadIdx.x);
    if (r >= num_rays) return;
    const float slope = dot3_as_aten(g0 + 3 * r, directions + 3 * r);
    const float step = rounded(-d0[r] / slope);
    slopes[r] = slope;
    const bool hit = converged[r] != 0;
    for (int k = 0; k < 3; ++k) {
        const float start = p0[3 * r + k];
        p1[3 * r + k] = hit ? rounded(start + rounded(directions[3 * r + k] * step)) : start;
    }
}

// F.normalize: n = g1 / clamp_min(sqrt(sum(g1 * g1)), 1e-12) (a NaN norm stays NaN, as clamp_min leaves it).  `lengths` keeps the clamped norm.
__global__ __launch_bounds__(kPhotometricThreads) void photometric_normalise_kernel(int num_rays, const float* __restrict__ g1, float* __restrict__ normals,
                                                                                    float* __restrict__ lengths, long long frame_stride) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(g1, shift); VSRD_OF_FRAME_NONNULL(normals, shift); VSRD_OF_FRAME_NONNULL(lengths, shift);
    }
    const int r = static_cast<int>(blockIdx.x * kPhotometricThreads + threadIdx.x);
    if (r >= num_rays) return;
    const float norm = sqrtf(dot3_as_aten(g1 + 3 * r, g1 + 3 * r));
    const float length = norm < 1.0e-12f ? 1.0e-12f : norm;
    lengths[r] = length;
    for (int k = 0; k < 3; ++k) normals[3 * r + k] = g1[3 * r + k] / length;
}

// The adjoint of F.normalize: gamma = (n_bar - n (n . n_bar)) / max(|g1|, 1e-12); zero for a ray that did not converge (its n_bar is zero).
__global__ __launch_bounds__(kPhotometricThreads) void photometric_normal_adjoint_kernel(int num_rays, const unsigned char* __restrict__ converged,
                                                                                         const float* __restrict__ normals, const float* __restrict__ lengths,
                                                                                         const float* __restrict__ grad_normals, float* __restrict__ gamma,
                                                                                         long long frame_stride) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(converged, shift); VSRD_OF_FRAME_NONNULL(normals, shift); VSRD_OF_FRAME_NONNULL(lengths, shift);
        VSRD_OF_FRAME_NONNULL(grad_normals, shift); VSRD_OF_FRAME_NONNULL(gamma, shift);
    }
    const int r = static_cast<int>(blockIdx.x * kPhotometricThreads + threadIdx.x);
    if (r >= num_rays) return;
    const float* n = normals + 3 * r;
    const float* nb = grad_normals + 3 * r;
    const bool hit = converged[r] != 0;
    const float along = n[0] * nb[0] + n[1] * nb[1] + n[2] * nb[2];
    for (int k = 0; k < 3; ++k) gamma[3 * r + k] = hit ? (nb[k] - n[k] * along) / lengths[r] : 0.0f;
}

// The adjoint of the Newton step w.r.t. the distance d0: -((p1_bar + x_bar) . r) / (g0 . r), p1_bar from the patch correlation and x_bar from
// the normal's dependence on the point; zero for a ray that did not converge (torch.where passes it nothing).
__global__ __launch_bounds__(kPhotometricThreads) void photometric_newton_adjoint_kernel(int num_rays, const unsigned char* __restrict__ converged,
                                                                                         const float* __restrict__ grad_p1, const float* __restrict__ grad_x,
                                                                                         const float* __restrict__ directions, const float* __restrict__ slopes,
                                                                                         float* __restrict__ grad_d0, long long frame_stride) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(converged, shift); VSRD_OF_FRAME_NONNULL(grad_p1, shift); VSRD_OF_FRAME_NONNULL(grad_x, shift);
        VSRD_OF_FRAME_NONNULL(directions, shift); VSRD_OF_FRAME_NONNULL(slopes, shift); VSRD_OF_FRAME_NONNULL(grad_d0, shift);
    }
    const int r = static_cast<int>(blockIdx.x * kPhotometricThreads + threadIdx.x);
    if (r >= num_rays) return;
    float along = 0.0f;
    for (int k = 0; k < 3; ++k) along += (grad_p1[3 * r + k] + grad_x[3 * r + k]) * directions[3 * r + k];
    grad_d0[r] = converged[r] != 0 ? -(along / slopes[r]) : 0.0f;
}

// own[i] = first[i] + second[i] (the two field adjoints' parameter gradients), then total[i] = fma(scale, own[i], total[i]); with no converged
// ray (stats[1] == 0) own is zero and total keeps its bits.  One launch covers the instance block [count_instances] and, for residual
// fields, the MLP block [count_mlp].  In a batch with headers the counts are those of the capacity `num_instances`, and a frame covers the
// leading blocks of its own n_f instances: the rows n_f .. capacity - 1 of own and total are not touched.
__global__ __launch_bounds__(kPhotometricThreads) void photometric_accumulate_kernel(const float* __restrict__ stats, float scale, int count_instances, int count_mlp,
                                                                                     const float* __restrict__ first_instances, const float* __restrict__ second_instances,
                                                                                     const float* __restrict__ first_mlp, const float* __restrict__ second_mlp,
                                                                                     float* __restrict__ own_instances, float* __restrict__ own_mlp,
                                                                                     float* __restrict__ total_instances, float* __restrict__ total_mlp,
                                                                                     int num_instances, long long frame_stride,
                                                                                     const FrameHeader* __restrict__ frame_header) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(stats, shift); VSRD_OF_FRAME_NONNULL(first_instances, shift); VSRD_OF_FRAME_NONNULL(second_instances, shift);
        VSRD_OF_FRAME(first_mlp, shift); VSRD_OF_FRAME(second_mlp, shift); VSRD_OF_FRAME_NONNULL(own_instances, shift); VSRD_OF_FRAME(own_mlp, shift);
        VSRD_OF_FRAME_NONNULL(total_instances, shift); VSRD_OF_FRAME(total_mlp, shift);
    }
    if (frame_header != nullptr) {
        const int own = frame_count_of(frame_header, frame_stride, blockIdx.y, num_instances);
        count_instances = count_instances / num_instances * own;
        count_mlp = count_mlp / num_instances * own;
    }
    const bool any = stats[1] != 0.0f;
    const int stride = static_cast<int>(gridDim.x) * kPhotometricThreads;
    for (int i = static_cast<int>(blockIdx.x * kPhotometricThreads + threadIdx.x); i < count_instances + count_mlp; i += stride) {
        const bool mlp = i >= count_instances;
        const int j = mlp ? i - count_instances : i;
        const float* first = mlp ? first_mlp : first_instances;
        const float* second = mlp ? second_mlp : second_instances;
        float* own = mlp ? own_mlp : own_instances;
        float* total = mlp ? total_mlp : total_instances;
        if (!any) { own[j] = 0.0f; continue; }
        const float sum = first[j] + second[j];
        own[j] = sum;
        total[j] = __fmaf_rn(scale, sum, total[j]);
    }
}

// record[4] += weight * loss (the product rounded, then the sum: the eager loop's total + weight * loss); untouched when no ray converged.
// A batch: frame blockIdx.y.
__global__ void photometric_finish_kernel(const float* __restrict__ loss, const float* __restrict__ stats, float weight, float* __restrict__ record,
                                          long long frame_stride) {
    if (frame_stride != 0) {
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(loss, shift); VSRD_OF_FRAME_NONNULL(stats, shift); VSRD_OF_FRAME_NONNULL(record, shift);
    }
    if (threadIdx.x != 0 || blockIdx.x != 0 || stats[1] == 0.0f) return;
    record[4] = rounded(record[4] + rounded(weight * loss[0]));
}

}  // namespace vsrd
