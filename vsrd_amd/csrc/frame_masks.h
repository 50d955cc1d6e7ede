// vsrd_frame_masks: a frame's dense predicted instance masks of one view, bit-packed -- what the reference renders every
// `image_intervals` steps (scripts/main.py:1011-1061): volume_masks = the two-pass hierarchical_volumetric_rendering of the soft union at
// every pixel, surface_masks = sphere_tracing(..., initialization=False, differentiable=False)[1], predicted masks = their product.
// One wave owns a run of 64 horizontally consecutive pixels of one image row of one frame:
//
//   1. trace     one lane per pixel: the march of sphere_trace_kernel (aux_kernels.h) with the soft union, foreground = finite origin, no
//                initialisation; a lane is finished once it is stationary, not at its first convergence (a ray that steps past a rim
//                un-converges, as in the reference) -> `converged` per lane, its ballot per run
//   2. render    only the converged pixels of the run, one ray at a time with the whole wave: the body of render_hierarchical_kernel
//                (render_kernels.h: cull_ray_setup, stage_ray_samples, render_pass, importance_merge, render_pass); a run without a
//                converged pixel renders nothing.  Ray p = y W + x reads row p of the recorded uniforms, or the Philox stream keyed by p
//   3. collect   after pixel i's labels are known lane n ORs (label_n > threshold) << i into a 64-bit accumulator of its own: at the end
//                of the run lane n holds instance n's 64 pixel bits
//   4. store     lane n reverses the bits of each byte (numpy.packbits: most significant bit first) and stores 8 bytes at once when the
//                address is 8-byte aligned, else -- and for a tail shorter than 64 pixels -- byte by byte; pad bits of a row's last byte
//                are 0 (the lanes beyond the row never converge)
//   5. count     (optional) the target bits of the run, one ballot per instance, then popcounts of prediction, target and their
//                intersection, added to counts [N,3] with integer atomics (order-independent)
//
// soft [H W, N] (optional; production passes NULL) is the only per-pixel float output: labels where the trace converged, exactly 0.0
// elsewhere.  Instances n_f .. N - 1 of a row laid out for a capacity N (a header, wave.h: mixed batches) are never read and never written.
#pragma once
#include "aux_kernels.h"

namespace vsrd {

struct MaskArgs {
    int view, height, width;
    int num_iterations;
    float criteria, bounding_radius, threshold;
    int target_stride;
};

// counts [N,3] of every frame of the launch start at zero, rows n_f .. N - 1 left alone: one workgroup per frame
__global__ __launch_bounds__(256) void frame_masks_clear_kernel(int* __restrict__ counts, int capacity, long long frame_stride,
                                                                const FrameHeader* __restrict__ frame_header) {
    const long long shift = frame_shift(frame_stride, blockIdx.x);
    counts = of_frame_nonnull(counts, shift);
    const int n = frame_header ? frame_count(of_frame_nonnull(frame_header, shift), capacity) : capacity;
    for (int idx = static_cast<int>(threadIdx.x); idx < 3 * n; idx += static_cast<int>(blockDim.x)) counts[idx] = 0;
}

template <int kRounds, bool kResidual>
__global__ __launch_bounds__(kBlockThreads) void frame_masks_kernel(
    FieldArgs f, const float* __restrict__ instances, const float* __restrict__ mlp, RenderArgs c, MaskArgs m,
    const float* __restrict__ camera_positions, const float* __restrict__ directions, const float* __restrict__ u_coarse, const float* __restrict__ u_fine,
    const float* __restrict__ targets, const int* __restrict__ target_columns,
    unsigned char* __restrict__ mask_bits, float* __restrict__ soft, int* __restrict__ counts, const FrameHeader* __restrict__ frame_header) {
    // N: the instances this frame has; NS: the stride of the per-instance rows (a mixed batch's capacity, wave.h; N without a header)
    const int NS = f.num_instances;
    if (c.frame_stride != 0) {             // a batch of frames (wave.h): this workgroup's frame is blockIdx.y
        const long long shift = frame_shift(c.frame_stride, blockIdx.y);
        shift_frame(c, shift);
        VSRD_OF_FRAME_NONNULL(instances, shift); VSRD_OF_FRAME(mlp, shift); VSRD_OF_FRAME_NONNULL(camera_positions, shift); VSRD_OF_FRAME_NONNULL(directions, shift);
        VSRD_OF_FRAME(u_coarse, shift); VSRD_OF_FRAME(u_fine, shift); VSRD_OF_FRAME(targets, shift); VSRD_OF_FRAME(target_columns, shift);
        VSRD_OF_FRAME_NONNULL(mask_bits, shift); VSRD_OF_FRAME(soft, shift); VSRD_OF_FRAME(counts, shift); VSRD_OF_FRAME(frame_header, shift);
    }
    const int N = frame_header ? frame_count(frame_header, NS) : NS;
    f.num_instances = N;
    apply_device_schedule(f, c);
    constexpr int kRoundsS = (kRounds + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = wave_in_block();
    const int lane = lane_id();
    const int S = c.num_samples, D = 2 * S;
    float* mine = lds + wave * hierarchical_lds_floats(S, NS, kResidual);         // (the host sizes a wave's partition for the capacity)
    const WaveLds l = carve_lds(mine + forward_weights_floats(kResidual), S, N);
    const bool sorted_input = (u_fine != nullptr) && (c.flags & 1u);
    Shading sh = c.sh;
    sh.mlp_lds = mine;                     // residual fields: the staging area of the trace's and the render's residual_forward alike
    const FieldBounds bounds = field_bounds(instances, N, f.inv_t, kResidual, c.flags);
    sh.cull = bounds.margin; sh.reach = bounds.reach; sh.yaw = bounds.yaw;
    sh.mlp_bits = (c.flags & 8u) ? kMlpCentredBit : 0u;
    const int H = m.height, W = m.width;
    const int runs_per_row = (W + kWave - 1) / kWave, num_runs = H * runs_per_row, row_bytes = (W + 7) >> 3;
    const long long view_first = static_cast<long long>(m.view) * H * W;          // the view's first row of the per-pixel tensors
    directions += view_first * 3;
    if (targets != nullptr) targets += view_first * m.target_stride;
    const float ox = uniform(camera_positions[3 * m.view + 0]), oy = uniform(camera_positions[3 * m.view + 1]), oz = uniform(camera_positions[3 * m.view + 2]);
    const int stride = static_cast<int>(gridDim.x) * waves_per_block();
    for (int run = static_cast<int>(blockIdx.x) * waves_per_block() + wave; run < num_runs; run += stride) {
        const int y = run / runs_per_row, x0 = (run - y * runs_per_row) * kWave;
        const bool valid = x0 + lane < W;
        const int pixel = y * W + (valid ? x0 + lane : W - 1);                    // (lanes beyond the row repeat its last pixel and never converge)
        // ---- 1. trace (sphere_trace_kernel: soft union, foreground = finite origin, no initialisation) ---------------------------------
        float px = ox, py = oy, pz = oz;
        const float dx = directions[pixel * 3ll + 0], dy = directions[pixel * 3ll + 1], dz = directions[pixel * 3ll + 2];
        bool fg = isfinite(px) && isfinite(py) && isfinite(pz);
        bool conv = false, done = !valid;
        for (int it = 0; it < m.num_iterations; ++it) {
            const float sd = union_distance<kResidual>(f, instances, mlp, px, py, pz, 0, mine);       // all lanes, stopped or not
            if (!done) {
                const bool moved = fg && !conv;
                if (moved) { px += dx * sd; py += dy * sd; pz += dz * sd; }
                if (m.bounding_radius > 0.0f) fg = fg && (sqrtf(px * px + py * py + pz * pz) < m.bounding_radius);
                conv = fabsf(sd) < m.criteria && isfinite(px) && isfinite(py) && isfinite(pz);
                done = !moved && !(fg && !conv);                   // stationary (aux_kernels.h)
            }
            if (!wave_any(!done)) break;
        }
        unsigned long long todo = __ballot(conv);
        if (soft != nullptr && valid && !conv)
            for (int n = 0; n < N; ++n) soft[static_cast<size_t>(pixel) * NS + n] = 0.0f;
        // ---- 2./3. render the converged pixels, one ray per turn of the wave; lane n collects instance n's bits -----------------------
        unsigned long long bits = 0ull;
        while (todo != 0ull) {
            const int i = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const int ray = y * W + x0 + i;
            Ray r;
            r.ox = ox; r.oy = oy; r.oz = oz;
            r.rx = read_lane(dx, i); r.ry = read_lane(dy, i); r.rz = read_lane(dz, i);
            const RayCull rc = cull_ray_setup(instances, N, r.ox, r.oy, r.oz, r.rx, r.ry, r.rz, l.cull, lane);
            stage_ray_samples<kRoundsS>(l, c, S, ray, u_coarse, u_fine, nullptr, nullptr, sorted_input, lane);
            float w1[kRoundsS];
            render_pass<kRoundsS, false, kResidual>(instances, mlp, N, sh, r, rc, l.coarse, S, l.dcache, w1, nullptr, nullptr);
            bool missed = false;
            if (c.flags & 2u) {                                                   // VSRD_FLAG_SKIP_EXACT_MISSES: labels exactly 0
                float total = 0.0f;
#pragma unroll
                for (int k = 0; k < kRoundsS; ++k) total += wave_sum(w1[k]);
                missed = total == 0.0f;                                           // wave-uniform
            }
            float label = 0.0f;
            if (!missed) {
                importance_merge<kRoundsS>(l, S, w1);
                float w2[kRounds];
                label = render_pass<kRounds, true, kResidual>(instances, mlp, N, sh, r, rc, l.merged, D, l.dcache, w2, nullptr, nullptr);
            }
            if (lane < N) {
                if (soft != nullptr) soft[static_cast<size_t>(ray) * NS + lane] = label;
                if (label > m.threshold) bits |= 1ull << i;
            }
            wave_lds_sync();
        }
        // ---- 4. store: byte j of the run = pixels x0 + 8 j .. + 7, most significant bit first ----------------------------------------------
        if (lane < N) {
            const int first_byte = x0 >> 3;
            const int num_bytes = row_bytes - first_byte < 8 ? row_bytes - first_byte : 8;
            unsigned char* dst = mask_bits + (static_cast<size_t>(lane) * H + y) * row_bytes + first_byte;
            const unsigned long long packed = __builtin_bswap64(__builtin_bitreverse64(bits));
            if (num_bytes == 8 && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0u) {
                *reinterpret_cast<unsigned long long*>(dst) = packed;
            } else {
                for (int j = 0; j < num_bytes; ++j) dst[j] = static_cast<unsigned char>(packed >> (8 * j));
            }
        }
        // ---- 5. counts: (#pred, #target, #pred and target) of the run ------------------------------------------------------------------------
        if (counts != nullptr) {
            unsigned long long target_bits = 0ull;
            for (int n = 0; n < N; ++n) {
                const int column = target_columns ? target_columns[n] : n;       // wave-uniform
                const bool set = valid && column >= 0 && targets[static_cast<size_t>(pixel) * m.target_stride + column] > m.threshold;
                const unsigned long long word = __ballot(set);
                if (lane == n) target_bits = word;
            }
            if (lane < N) {
                const int pred = __builtin_popcountll(bits), target = __builtin_popcountll(target_bits), both = __builtin_popcountll(bits & target_bits);
                if (pred != 0) atomicAdd(counts + 3 * lane + 0, pred);
                if (target != 0) atomicAdd(counts + 3 * lane + 1, target);
                if (both != 0) atomicAdd(counts + 3 * lane + 2, both);
            }
        }
    }
}

}  // namespace vsrd
