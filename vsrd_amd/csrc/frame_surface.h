// vsrd_frame_surface: the dense surface render of one view of a frame -- position, range, normal, owning instance, shadow and a shaded
// image laid over the photograph: sphere_tracing, surface_normal, shadow_rendering and phong_shading (vsrd/rendering/renderers.py:21-174)
// as the dense logging branch of scripts/main.py:1028-1041 composes them.  One wave owns a run of 64 horizontally consecutive pixels of one
// image row of one frame, one lane per pixel (the shape of frame_masks.h):
//
//   1. trace     the march of sphere_trace_kernel (aux_kernels.h) with union_distance, soft or hard by a flag: foreground = finite origin,
//                no initialisation, a lane is finished once it is stationary -> position, `converged` per lane, its ballot per run.  A run
//                whose ballot is empty computes nothing further (its outputs are those of pixels that did not converge)
//   2. point     one evaluation of the union with its analytic gradient, the loops of field_eval_kernel (the whole wave stays in the
//                instance loop: the residual MLP is wave-cooperative): normal = g / max(|g|, 1e-12) (F.normalize), instance = the first
//                member with the smallest distance, range = |position - origin|
//   3. shadow    (a light and VSRD_SURFACE_SHADOWS) the same march from position + normal * shadow_offset along -light, only the converged
//                lanes foreground: shadow = converged AND this trace's converged (shadow_rendering with foreground_masks = converged)
//   4. shade     phong_shading with the diffuse material colour palette[instance]; the diffuse and specular terms times (1 - shadow) -- this
//                project's choice, the reference defines no combination; alpha-blended over the background pixel, stored as uint8
//   5. store     both bit planes: the ballots with the bits of each byte reversed (numpy.packbits: most significant bit first), 8 bytes at
//                once by lane 0 when the address is 8-byte aligned, else -- and for a tail shorter than 64 pixels -- byte j by lane j; pad
//                bits of a row's last byte are 0 (the lanes beyond the row never converge)
//
// shadow_offset is an argument of its own (the reference uses the convergence criteria c): at c a point at d(p) = delta < 0 starts its
// shadow ray at about delta + c < c, converges at once and reads as shadowed; with 2 c, d(start) ~ d(p) + 2 c > c because d(p) > -c.
// Box-only fields need no LDS, residual ones the per-wave staging of residual_forward's weights.  No floating-point atomics: every output
// element is written by the one lane that owns its pixel (the bit planes: its byte).
#pragma once
#include "aux_kernels.h"

namespace vsrd {

constexpr unsigned kSurfaceHardUnion = 1u, kSurfaceShadows = 2u;       // VSRD_SURFACE_*
constexpr int kSurfaceThreads = 256;

struct SurfaceArgs {
    int view, height, width;
    int num_iterations;
    float criteria, bounding_radius, shadow_offset;
    unsigned flags;
    float alpha, shininess;
    float background_color[3];
    float ambient[3];                   // material_emission + material_ambient * light_ambient
    float diffuse[3], specular[3];      // light_diffuse; material_specular * light_specular
};

struct SurfaceBuffers {
    const float* camera_positions; const float* directions; const float* light; const float* palette; const unsigned char* background;
    unsigned char* converged_bits; unsigned char* shadow_bits; unsigned char* instance; float* range; unsigned char* colors;
    float* positions; float* normals;
};

// the march of sphere_trace_kernel from (px, py, pz) along (dx, dy, dz); `done`: lanes that take no part (they still evaluate: the
// residual MLP is wave-cooperative).  Returns `converged`; the position is left where the trace ended.
template <bool kResidual>
__device__ __forceinline__ bool surface_march(const FieldArgs& f, const float* __restrict__ instances, const float* __restrict__ mlp, const SurfaceArgs& a,
                                              int hard, float& px, float& py, float& pz, float dx, float dy, float dz, bool fg, bool done, float* weights) {
    bool conv = false;
    for (int it = 0; it < a.num_iterations; ++it) {
        const float sd = union_distance<kResidual>(f, instances, mlp, px, py, pz, hard, weights);       // all lanes, stopped or not
        if (!done) {
            const bool moved = fg && !conv;
            if (moved) { px += dx * sd; py += dy * sd; pz += dz * sd; }
            if (a.bounding_radius > 0.0f) fg = fg && (sqrtf(px * px + py * py + pz * pz) < a.bounding_radius);
            conv = fabsf(sd) < a.criteria && isfinite(px) && isfinite(py) && isfinite(pz);
            done = !moved && !(fg && !conv);                   // stationary (aux_kernels.h)
        }
        if (!wave_any(!done)) break;
    }
    return conv;
}

__device__ __forceinline__ unsigned char surface_quantise(float c) { return static_cast<unsigned char>(static_cast<int>(255.0f * c + 0.5f)); }

// one bit plane's 64 bits of a run: byte j of the run = pixels x0 + 8 j .. + 7, most significant bit first (frame_masks.h step 4)
__device__ __forceinline__ void surface_store_bits(unsigned char* __restrict__ plane, unsigned long long bits, int y, int x0, int row_bytes, int lane) {
    const int first_byte = x0 >> 3;
    const int num_bytes = row_bytes - first_byte < 8 ? row_bytes - first_byte : 8;
    unsigned char* dst = plane + static_cast<size_t>(y) * row_bytes + first_byte;
    const unsigned long long packed = __builtin_bswap64(__builtin_bitreverse64(bits));
    if (num_bytes == 8 && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0u) {
        if (lane == 0) *reinterpret_cast<unsigned long long*>(dst) = packed;
    } else if (lane < num_bytes) {
        dst[lane] = static_cast<unsigned char>(packed >> (8 * lane));
    }
}

template <bool kResidual>
__global__ __launch_bounds__(kSurfaceThreads) void frame_surface_kernel(FieldArgs f, const float* __restrict__ instances, const float* __restrict__ mlp,
                                                                        const float* __restrict__ schedule, SurfaceArgs a, SurfaceBuffers b,
                                                                        long long frame_stride, const FrameHeader* __restrict__ frame_header) {
    // N: the instances this frame has; the capacity f.num_instances stays the stride of the palette (a mixed batch, wave.h)
    if (frame_stride != 0) {               // a batch of frames (wave.h): this workgroup's frame is blockIdx.y
        const long long shift = frame_shift(frame_stride, blockIdx.y);
        VSRD_OF_FRAME_NONNULL(instances, shift); VSRD_OF_FRAME(mlp, shift); VSRD_OF_FRAME(schedule, shift); VSRD_OF_FRAME(frame_header, shift);
        b.camera_positions = of_frame_nonnull(b.camera_positions, shift); b.directions = of_frame_nonnull(b.directions, shift);
        b.light = of_frame(b.light, shift); b.palette = of_frame(b.palette, shift); b.background = of_frame(b.background, shift);
        b.converged_bits = of_frame(b.converged_bits, shift); b.shadow_bits = of_frame(b.shadow_bits, shift); b.instance = of_frame(b.instance, shift);
        b.range = of_frame(b.range, shift); b.colors = of_frame(b.colors, shift); b.positions = of_frame(b.positions, shift);
        b.normals = of_frame(b.normals, shift);
    }
    if (frame_header != nullptr) f.num_instances = frame_count(frame_header, f.num_instances);
    if (schedule != nullptr) f.inv_t = 1.0f / schedule[0];      // (apply_device_schedule's temperature)
    // residual fields: this wave's staging area for residual_forward's weight operands (static LDS: 4 waves x 6.5 KB)
    __shared__ float forward_weights_all[kResidual ? (kSurfaceThreads / kWave) * kMlpWbarFloats : 1];
    float* weights = forward_weights_all + (kResidual ? wave_in_block() * kMlpWbarFloats : 0);
    const int wave = wave_in_block();
    const int lane = lane_id();
    const int hard = (a.flags & kSurfaceHardUnion) ? 1 : 0;
    const int H = a.height, W = a.width;
    const int runs_per_row = (W + kWave - 1) / kWave, num_runs = H * runs_per_row, row_bytes = (W + 7) >> 3;
    const float* __restrict__ directions = b.directions + static_cast<long long>(a.view) * H * W * 3;       // the view's first row
    const float ox = uniform(b.camera_positions[3 * a.view + 0]), oy = uniform(b.camera_positions[3 * a.view + 1]), oz = uniform(b.camera_positions[3 * a.view + 2]);
    const bool lit = b.light != nullptr;
    const float lx = lit ? uniform(b.light[0]) : 0.0f, ly = lit ? uniform(b.light[1]) : 0.0f, lz = lit ? uniform(b.light[2]) : 0.0f;
    const bool shadows = lit && (a.flags & kSurfaceShadows) != 0u;
    const int stride = static_cast<int>(gridDim.x) * (kSurfaceThreads / kWave);
    for (int run = static_cast<int>(blockIdx.x) * (kSurfaceThreads / kWave) + wave; run < num_runs; run += stride) {
        const int y = run / runs_per_row, x0 = (run - y * runs_per_row) * kWave;
        const bool valid = x0 + lane < W;
        const long long pixel = static_cast<long long>(y) * W + (valid ? x0 + lane : W - 1);      // (lanes beyond the row repeat its last pixel and never converge)
        // ---- 1. primary trace --------------------------------------------------------------------------------------------------------------
        float px = ox, py = oy, pz = oz;
        const float dx = directions[pixel * 3 + 0], dy = directions[pixel * 3 + 1], dz = directions[pixel * 3 + 2];
        const bool conv = surface_march<kResidual>(f, instances, mlp, a, hard, px, py, pz, dx, dy, dz, isfinite(px) && isfinite(py) && isfinite(pz), !valid, weights);
        const unsigned long long hit = __ballot(conv);
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, range = 0.0f;
        int owner = 255;
        bool shadow = false;
        if (hit != 0ull) {
            // ---- 2. surface point: the union's gradient and the arg-min member (field_eval_kernel) --------------------------------------------
            float gx, gy, gz, best = 3.0e38f;
            int best_index = 0;
            if (hard) {
                gx = gy = gz = 0.0f;
                for (int i = 0; i < f.num_instances; ++i) {
                    const BoxEval e = eval_instance<kResidual>(load_instance(instances, i), kResidual ? mlp + i * kMlpWeights : nullptr, px, py, pz, weights);
                    if (e.d < best) { best = e.d; best_index = i; gx = e.gwx; gy = e.gwy; gz = e.gwz; }   // argmin: first minimum
                }
            } else {
                UnionSums sums = union_init();
                for (int i = 0; i < f.num_instances; ++i) {
                    const BoxEval e = eval_instance<kResidual>(load_instance(instances, i), kResidual ? mlp + i * kMlpWeights : nullptr, px, py, pz, weights);
                    union_accumulate(sums, e.d, e.gwx, e.gwy, e.gwz, 0.0f, f.inv_t);
                    if (e.d < best) { best = e.d; best_index = i; }
                }
                const UnionValue v = union_finish(sums, f.inv_t);
                gx = v.gx; gy = v.gy; gz = v.gz;
            }
            if (conv) {
                const float norm = fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1.0e-12f);
                nx = gx / norm; ny = gy / norm; nz = gz / norm;
                const float ex = px - ox, ey = py - oy, ez = pz - oz;
                range = sqrtf(ex * ex + ey * ey + ez * ez);
                owner = best_index;
            }
            // ---- 3. shadow trace from just above the surface towards the light ---------------------------------------------------------------
            if (shadows) {
                float tx = nx * a.shadow_offset, ty = ny * a.shadow_offset, tz = nz * a.shadow_offset;
                asm volatile("" : "+v"(tx), "+v"(ty), "+v"(tz));      // (rounded products, then rounded sums: position + normal * offset as torch computes it)
                float sx = px + tx, sy = py + ty, sz = pz + tz;
                shadow = surface_march<kResidual>(f, instances, mlp, a, hard, sx, sy, sz, -lx, -ly, -lz, conv, !conv, weights) && conv;
            }
        }
        // ---- 4. shade ---------------------------------------------------------------------------------------------------------------------
        if (b.colors != nullptr && valid) {
            unsigned char out[3];
            float back[3] = {a.background_color[0], a.background_color[1], a.background_color[2]};
            if (b.background != nullptr) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { out[c] = b.background[pixel * 3 + c]; back[c] = static_cast<float>(out[c]) * (1.0f / 255.0f); }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c] = surface_quantise(fminf(fmaxf(back[c], 0.0f), 1.0f));
            }
            if (conv) {
                const float vn = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1.0e-12f), ln = 1.0f / fmaxf(sqrtf(lx * lx + ly * ly + lz * lz), 1.0e-12f);
                const float vx = dx * vn, vy = dy * vn, vz = dz * vn, ux = lx * ln, uy = ly * ln, uz = lz * ln;
                const float incidence = ux * nx + uy * ny + uz * nz;
                const float rx = ux - 2.0f * nx * incidence, ry = uy - 2.0f * ny * incidence, rz = uz - 2.0f * nz * incidence;
                const float unshadowed = shadow ? 0.0f : 1.0f;
                const float diffuse = fmaxf(-incidence, 0.0f) * unshadowed;
                const float specular = powf(fmaxf(-(rx * vx + ry * vy + rz * vz), 0.0f), a.shininess) * unshadowed;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float colour = fminf(fmaxf(a.ambient[c] + b.palette[owner * 3 + c] * a.diffuse[c] * diffuse + a.specular[c] * specular, 0.0f), 1.0f);
                    out[c] = surface_quantise(a.alpha * colour + (1.0f - a.alpha) * back[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) b.colors[pixel * 3 + c] = out[c];
        }
        // ---- 5. store ---------------------------------------------------------------------------------------------------------------------
        if (valid) {
            if (b.instance != nullptr) b.instance[pixel] = static_cast<unsigned char>(owner);
            if (b.range != nullptr) b.range[pixel] = range;
            if (b.positions != nullptr) { b.positions[pixel * 3 + 0] = px; b.positions[pixel * 3 + 1] = py; b.positions[pixel * 3 + 2] = pz; }
            if (b.normals != nullptr) { b.normals[pixel * 3 + 0] = nx; b.normals[pixel * 3 + 1] = ny; b.normals[pixel * 3 + 2] = nz; }
        }
        if (b.converged_bits != nullptr) surface_store_bits(b.converged_bits, hit, y, x0, row_bytes, lane);
        if (b.shadow_bits != nullptr) surface_store_bits(b.shadow_bits, __ballot(shadow), y, x0, row_bytes, lane);
    }
}

}  // namespace vsrd
