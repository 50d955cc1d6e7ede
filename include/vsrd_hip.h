/*
 * libvsrd_hip -- C ABI of the MI355X (gfx950) implementation of VSRD's instance-aware
 * volumetric silhouette renderer and the geometry around it.
 *
 * The reference (skmhrk1209/VSRD) is pure Python on PyTorch and defines no FFI; the
 * boundary it offers is the Python call surface of vsrd.rendering / vsrd.operations as
 * used by scripts/main.py.  Every entry point below names the
 * reference function it replaces (file:line under the reference checkout).  The Python
 * package vsrd_amd/ binds these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - all pointers are DEVICE pointers to fp32 (or the stated type), caller-owned;
 *   - per-sample tensors are ray-major: [R, D] (the reference's sample-major [D, R, 1]
 *     is a permuted view of the same buffer);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), touches no
 *     global state and is re-entrant;
 *   - return value: 0 on success, a negative VSRD_E_* code otherwise (never throws);
 *     vsrd_error_string() describes a code.
 */
#ifndef VSRD_HIP_H
#define VSRD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSRD_ABI_VERSION 12

#define VSRD_OK 0
#define VSRD_E_INVALID_ARGUMENT (-1) /* null pointer, non-positive size, unsupported N / S */
#define VSRD_E_UNSUPPORTED (-2)      /* valid request this build does not implement        */
#define VSRD_E_LAUNCH (-3)           /* hipGetLastError() != hipSuccess after the launch   */
#define VSRD_E_WORKSPACE (-4)        /* workspace too small (see vsrd_workspace_bytes)     */

#define VSRD_MAX_INSTANCES 64  /* N, instances per soft-min union                         */
#define VSRD_MAX_SAMPLES 256   /* S, num_samples of hierarchical_volumetric_rendering      */
#define VSRD_INSTANCE_STRIDE 16 /* floats per packed instance: t[3] R[9] (row-major) dim[3] pad */
#define VSRD_MLP_WEIGHTS 1617  /* per-instance residual MLP, hyper_distance_field.py:18-25 */

/* ---- frame batches (ABI 8) --------------------------------------------------------------------------------------------------
 * The reference's unit of work is one target frame optimised for 3000 steps of 1000 rays (scripts/main.py:323-865), and its loop carries
 * a batch dimension: BoxParameters3D(batch_size, num_instances) (vsrd/models/detectors/box_parameters.py:34-49), lists over the batch
 * of distance fields, camera positions, ray directions and soft masks (scripts/main.py:525-651).  One frame's launches leave most of the
 * GPU idle (about one wave per SIMD), so the entry points of the per-frame step take a batch of INDEPENDENT frames in one launch each:
 *
 *     num_frames   B >= 2 (0 or 1: one frame, the meaning of every earlier ABI);
 *     frame_stride bytes, a positive multiple of 256: EVERY device pointer of the call -- arguments, struct members, workspaces --
 *                  addresses frame 0's buffer, and frame f's buffer lies f * frame_stride bytes behind it.
 *
 * The caller keeps each frame's buffers at the same offsets of one arena row per frame.  By-value arguments (sizes, seeds, flags, Adam's
 * constants) are shared; per-frame state (parameters, Adam's moments and counters, learning rates, the step counter that keys the Philox
 * streams, schedules, ray tables, scratch) lies behind the pointers and is therefore the frame's own.  There is no arithmetic across
 * frames: frame f's results are BIT-IDENTICAL to those of the same call on frame f alone (the launch is B copies of the one-frame grid,
 * tests/test_hip_step.py::test_frame_batch_walks_each_frames_own_trajectory).
 * The fields sit at the end of vsrd_render_config, vsrd_frame_config and vsrd_hypernetwork.  Entry points that accept B >= 2:
 * vsrd_frame_prologue, vsrd_frame_prologue_sample, vsrd_frame_epilogue, vsrd_frame_labels (ABI 11), vsrd_hypernetwork_forward, vsrd_hypernetwork_backward_step,
 * vsrd_render_silhouette_step (gathered launches in the split-ray form: at most 2048 rays per frame) and vsrd_render_residual_step
 * (two-kernel form, one chunk of rays per frame); every other entry point returns VSRD_E_UNSUPPORTED for B >= 2.
 *
 * Mixed batches (ABI 9): frames whose instance counts differ.  The batch keeps ONE layout for all of its rows, sized for a CAPACITY
 * N_cap, and every frame carries its own count 1 <= n_f <= N_cap in a vsrd_frame_header in device memory.  The entry points that take
 * a header are the *_with_header twins below; frame_header addresses frame 0's header and frame f's lies f * frame_stride bytes behind
 * it, like every other buffer of the call (a header for one frame is accepted too).  With a header set:
 *   - the by-value N (vsrd_field::num_instances, vsrd_frame_config::num_boxes) is the capacity: the stride of every per-instance array
 *     ([N,16] instances, [V,N,4] ground-truth boxes, [V,N] visibility, rows of targets with target_stride = N, ...);
 *   - each kernel reads the frame's count once, as a wave-uniform scalar, clamps it to [1, N] and loops, matches, reduces and
 *     normalises over that count only; instances n_f .. N_cap - 1 of a row are never read and never written;
 *   - loss_scale (the silhouette normaliser 1 / (R n_f)) is the header's, not the by-value argument.
 * Frame f then computes, bit for bit, what the same call computes on a frame of its own with N = n_f.  The old entry points are the
 * twins with frame_header = NULL: every frame has the by-value N, the by-value loss_scale applies.  A header on a launch form that does
 * not batch (the dense multi-ray kernels of vsrd_render_silhouette_step) is answered with VSRD_E_UNSUPPORTED, as B >= 2 is.
 * Twins: vsrd_frame_prologue, vsrd_frame_prologue_sample, vsrd_frame_epilogue, vsrd_render_silhouette_step (split-ray form),
 * vsrd_render_residual_step (two-kernel form with the ray split over a pair of waves, both MLP product forms), vsrd_hypernetwork_forward,
 * vsrd_hypernetwork_backward_step (N = vsrd_hypernetwork::num_instances is the capacity: the stride of the embeddings and the workspace).
 *
 * Frames that differ in VIEW count (ABI 12).  A frame's view count is not a constant of a job (vsrd/datasets/kitti_360_dataset.py:192-197
 * drops the empty parts of a target's source frames: 1 .. 1 + num_source_frames views), so the header carries it too, behind its two
 * ABI-9 fields.  A caller of ABI 9-11 allocated 8 bytes per header, so the tail is read ONLY from a header that says it has one:
 * num_instances = n_f | VSRD_FRAME_HEADER_HAS_VIEWS.  Without that bit a header means exactly what it meant in ABI 9 (and every kernel
 * masks the bit off before it uses the count).  With it:
 *   - the by-value vsrd_frame_config::num_views is the view capacity V_cap: the stride and extent of the row's per-view arrays
 *     ([V,16] extrinsics, [V,9] intrinsics, [V,N,4] ground-truth boxes, [V,N] visibility, [V,N,8,3] / [V,N,4] label outputs), as
 *     num_boxes is for N; every per-view array is view-major, so a frame with fewer views fills a prefix of each;
 *   - num_views = v_f (0: the by-value V; else clamped to [1, V_cap]): vsrd_frame_prologue_with_header,
 *     vsrd_frame_prologue_sample_with_header and vsrd_frame_labels read it once, as a wave-uniform scalar, and project, match, reduce
 *     and normalise over v_f views only; views v_f .. V_cap - 1 of every per-view input and output are never read and never written.
 *     The prologue's choice between LDS and the global scratch (V N <= 256) and its offsets into the scratch follow the frame's OWN
 *     v_f n_f -- the path the frame takes alone; vsrd_frame_scratch_bytes stays sized by the capacities;
 *   - num_pixels = v_f H W (0, or more than the by-value count: the by-value count): the count of the frame's sampling table, from
 *     which the sampler half of vsrd_frame_prologue_sample_with_header derives the table's layout (chunk sums, guide) and guide bits.
 *     The table inside the row is the one vsrd_ray_table_build(weights, v_f H W, ...) builds for the frame alone; only the row's
 *     allocation is sized for V_cap H W (vsrd_ray_table_bytes is monotone in the count).
 * Frame f then computes, bit for bit, what the same call computes on a frame of its own with V = v_f and N = n_f.  The epilogue, the
 * hypernetwork twins and the two render-step twins read no view count: the render kernels gather rays by pixel index and never see V.
 * vsrd_frame_ingest, vsrd_ray_directions and vsrd_ray_table_build are per-frame calls that take the frame's own V or count by value
 * and write a prefix of a row laid out for V_cap, nothing behind it. */
#define VSRD_FRAME_HEADER_HAS_VIEWS 0x10000 /* or-ed into vsrd_frame_header::num_instances: the header is the full ABI-12 struct */
typedef struct vsrd_frame_header {
    int32_t num_instances;      /* n_f, 1..N_cap (clamped) [| VSRD_FRAME_HEADER_HAS_VIEWS]                        */
    float loss_scale;           /* the silhouette loss normaliser of the frame: 1 / (R * n_f) as float32        */
    /* ---- ABI 12: read only when num_instances carries VSRD_FRAME_HEADER_HAS_VIEWS ---- */
    int32_t num_views;          /* v_f: 0 = the by-value V; else clamped to [1, V]                              */
    int32_t reserved;           /* 0                                                                            */
    int64_t num_pixels;         /* the sampler's count of this frame, v_f * H * W: 0 = the by-value count       */
} vsrd_frame_header;

/* Field = temperature soft-min union of N oriented boxes (+ optional residual MLP).
 * Replaces the closure tree scripts/main.py:525-618 builds from
 *   vsrd/rendering/sdfs.py:9-37 (box, rotation, translation),
 *   scripts/main.py:433-492     (residual field/composition, instance_field, soft_union). */
typedef struct vsrd_field {
    int32_t num_instances;      /* N, 1..VSRD_MAX_INSTANCES                                */
    float temperature;          /* sdf_union_temperature, main.py:423-426                  */
    const float* instances;     /* [N, 16] packed: location, rotation matrix, half extents */
    const float* mlp_weights;   /* [N, 1617] or NULL (box-only)                            */
} vsrd_field;

/* Scalars of vsrd.rendering.hierarchical_volumetric_rendering (renderers.py:177-188). */
typedef struct vsrd_render_config {
    int32_t num_rays;           /* R                                                        */
    int32_t num_samples;        /* S ("num_samples"); pass 1 renders S-1, pass 2 2S-1 points */
    float distance_near;        /* distance_range[0]                                        */
    float distance_far;         /* distance_range[1]                                        */
    float sdf_std_deviation;    /* NeuS logistic std                                        */
    float cosine_ratio;         /* cos anneal ratio, renderers.py:234-239                   */
    float epsilon;              /* opacity denominator guard, default 1e-6                  */
    int32_t origin_stride;      /* floats between ray origins: 3, or 0 for one shared origin */
    uint64_t seed;              /* Philox key when uniforms are generated in-kernel         */
    uint64_t stream_offset;     /* Philox counter offset (step index)                       */
    uint32_t flags;             /* VSRD_FLAG_*                                              */
    /* Optional, DEVICE memory: per-step values that a captured hipGraph must not freeze in its kernel arguments.  When set, the
     * render kernels read them at start and use them INSTEAD of the by-value fields above / field->temperature
     * (the annealing schedules of scripts/main.py:420-431 and the Philox counter of the step). */
    const float* device_schedule;          /* [3] = soft-min temperature, sdf_std_deviation, cosine_ratio; or NULL */
    const uint64_t* device_stream_offset;  /* [1] replaces stream_offset; or NULL                                   */
    /* Optional gather (the two fused step entry points only; the others reject it): the step's rays are rows of FRAME-RESIDENT
     * tensors picked by index, so that no per-step copies of directions / origins / targets are made (scripts/main.py:629-671 indexes
     * multi_ray_directions, multi_camera_positions and multi_soft_masks with multi_ray_indices).  With ray_indices set, ray r reads
     * directions[ray_indices[r]], origins[ray_indices[r] / rays_per_origin] (one camera position per view, origin_stride 3) and
     * the targets row ray_indices[r]; labels (if requested) stay [R,N] in step order. */
    const int64_t* ray_indices;            /* [R] or NULL                                                           */
    int32_t rays_per_origin;               /* pixels per view (H * W); 0: origins are per ray, gathered like the directions */
    /* Optional column map of the targets: a targets row has target_stride columns (ground-truth instance order) and predicted
     * instance n is compared with column target_columns[n] (the Hungarian assignment, main.py:653-671); NULL: targets are [.,N]
     * in prediction order. */
    const int32_t* target_columns;         /* [N] or NULL                                                           */
    int32_t target_stride;                 /* columns of a targets row when target_columns is set                   */
    /* Optional outputs of vsrd_render_silhouette_step (ABI 7) and vsrd_render_residual_step (ABI 8: two-kernel form, num_samples in
     * (32, 64], one ray per wave; VSRD_E_UNSUPPORTED otherwise); every other entry point rejects them: the per-ray state between the
     * step's passes, written by the step launch itself -- what pass 1 of scripts/main.py:511-523 returns (`sampled_weights`), the
     * uniforms it used, and the sorted pass-2 distances its labels, loss and gradients were computed at.  Rows are in STEP order (ray r
     * of the launch).  A step that writes them takes the multi-ray or the one-ray kernels (never the split-ray form). */
    float* out_distances;                  /* [R,2S] or NULL; row of an exact miss (VSRD_FLAG_SKIP_EXACT_MISSES): [r,0] = NaN, rest untouched */
    float* out_coarse_weights;             /* [R,S-1] or NULL: pass 1's compositing weights                           */
    float* out_u_coarse;                   /* [R,S] or NULL: the stratified uniforms used                            */
    float* out_u_fine;                     /* [R,S] or NULL: the fine uniforms used (SORTED when drawn in the kernel) */
    /* Frame batch (ABI 8, see "frame batches" above): num_rays etc. are PER FRAME. */
    int32_t num_frames;                    /* 0 or 1: one frame                                                       */
    int64_t frame_stride;                  /* bytes between the frames' copies of every buffer of the call            */
    /* vsrd_render_residual_step, two-kernel form (ABI 8): slots (= 64-sample rounds of a ray) per work item of the MLP-adjoint kernel,
     * 1..64; 0: planned from the launch's own size (about 16384 items per frame: 4 slots at 1000 rays, at most 32 -- and 64 for launches that
     * leave 32 k items even then: config 3's chunks of 110 k rays).  An item keeps its instance's
     * weight adjoints in registers and leaves ONE partial row of 6.6 KB, so larger items mean fewer rows to write and to sum -- what a
     * batch of frames wants, whose items are B times as many (8 frames x 1000 rays: 16 slots, -14 % per frame-step) -- and coarser load
     * balance.  The order of summation, and with it the last bits of grad_mlp_weights, depends on this number and on nothing else of the
     * launch geometry: equal numbers give bit-identical results for a frame alone and in a batch.  (A number below the planned one
     * needs more rows than vsrd_residual_step_workspace_bytes provides for: VSRD_E_WORKSPACE.) */
    int32_t adjoint_slots_per_item;
} vsrd_render_config;

#define VSRD_FLAG_FINE_UNIFORMS_SORTED 1u /* u_fine is already sorted ascending per ray     */
#define VSRD_FLAG_SKIP_EXACT_MISSES 2u    /* rays whose coarse weights are all exactly 0 skip pass 2:
                                             labels = 0 (exact); distances/gradients/weights of such
                                             rays are NOT produced (fused-loss mode only).  In the kernels
                                             that put several rays in a wave (dense box-only launches) the
                                             rays of a wave share the soft-min mode, so the OTHER rays of a
                                             wave agree with the un-skipped run to rounding, not bit for bit */

#define VSRD_FLAG_MLP_WEIGHTS_CENTRED 8u   /* residual fields: the caller guarantees that, in each of the four linears that feed a
                                             LayerNorm (rows [out][in+1] of mlp_weights), every column -- bias column included -- has
                                             zero mean over the 16 output channels.  LayerNorm makes the field invariant to that
                                             centring, and gradients w.r.t. centred weights equal those w.r.t. the originals; the
                                             kernels then skip centring the weight operands on every evaluation.                     */

#define VSRD_FLAG_NO_CULLING 4u           /* evaluate every instance at every sample (A/B switch for the
                                             conservative soft-min culling described in DESIGN.md)        */

#define VSRD_FLAG_RUNNING_MINIMUM 16u      /* shift the soft-min by the running minimum of the instance distances instead of the
                                             lower bound known before the instance loop (A/B switch; the kernels fall back to it by
                                             themselves wherever the bound is unavailable or too loose)                              */

#define VSRD_FLAG_RESIDUAL_SINGLE_KERNEL 64u /* vsrd_render_residual_step: run the whole step in ONE kernel (render + loss + adjoint of a
                                             batch of rays per wave, 427 registers, one wave per SIMD) instead of the default two
                                             kernels per chunk of rays (front part + MLP adjoint distributed by instance, two waves per
                                             SIMD each); the results agree to rounding (A/B switch)                         */

#define VSRD_FLAG_RESIDUAL_WAVE_PER_RAY 128u /* vsrd_render_residual_step: keep one wave per ray in the front kernel.  By default every
                                             ray is split over the two waves of a workgroup when num_samples > 64 (four wave rounds: the
                                             split kernel fits two waves per SIMD, the unsplit one does not) and, for num_samples in
                                             (32, 64], when the launch has <= 2048 rays (the reference's own 1000 rays per step then put
                                             two waves on every SIMD).  A/B switch.                                                   */

#define VSRD_FLAG_GENERAL_ROTATIONS 32u     /* do not use the shortened rotation products the kernels select by themselves when every
                                             instance's rotation is exactly one about the y axis (r01 = r10 = r12 = r21 = 0, r11 = 1,
                                             what rotation_matrix_y produces); the results agree to rounding (A/B switch)              */

#define VSRD_FLAG_STEP_WAVE_PER_RAY 256u    /* vsrd_render_silhouette_step: keep one wave per ray.  By default dense launches
                                             (ray_indices == NULL) with num_samples <= 64 and <= 16 instances put FOUR consecutive rays
                                             in a wave (16 sample points of each per round): the wave-uniform instance culling then
                                             works on a quarter of the depth range, and one parameter-adjoint reduction serves four
                                             rays; the results agree to rounding (A/B switch)                              */

#define VSRD_FLAG_STEP_SPLIT_RAY 512u       /* vsrd_render_silhouette_step: split every ray over the two waves of a workgroup, half of its
                                             rounds each (num_samples in (32, 128]: 2 or 4 rounds of 64 pass-2 points; for fewer samples the flag has no
                                             effect and the launch keeps one wave per ray).  By default launches of at most 2048 rays that are
                                             not dense launches of the shapes above -- the reference's 1000 importance-sampled rays
                                             per step -- do this by themselves (two waves on every SIMD instead of one: a small launch
                                             is latency); the flag forces it for any launch, VSRD_FLAG_STEP_WAVE_PER_RAY forbids it; the
                                             results agree to rounding (A/B switch)                                                     */

#define VSRD_FLAG_YAW_GRADIENTS 1024u       /* the caller differentiates the rotations only through rotation_matrix_y(cos, sin)
                                             (box_parameters.py:5-13: what BoxParameters3D decodes to): grad_instances then carries the
                                             adjoints of r00, r02, r20, r22 only -- the five entries that rotation_matrix_y keeps constant
                                             (r01, r10, r11, r12, r21) get ZERO instead of their adjoint, which nobody would read.  Only
                                             honoured when every rotation of the field IS of that form (checked on the device), by the
                                             multi-ray kernels of vsrd_render_silhouette_step / vsrd_render_backward; never set it for
                                             rotation matrices that are parameters themselves                                          */

#define VSRD_FLAG_MLP_SPLIT_BF16 2048u      /* vsrd_render_residual_step (two-kernel form): the per-instance MLP's matrix products of the FRONT
                                             kernel (pass 1, pass 2: value and gradient of every residual) run on v_mfma_f32_16x16x32_bf16 with
                                             both operands split into two bfloat16 parts (x = hi + lo to 2^-18; fp32 accumulation) instead of the
                                             exact-fp32 matrix instruction.  The C ABI's default is the exact-fp32 form; optimization.FrameOptimizer / FrameBatch
                                             (the native loop) set the flag by default (OptimizationConfig.mlp_split_bf16).  Measured on the GPU under the
                                             residual goldens' tests with both forms, against the reference's goldens: labels within 1.1e-6 (tolerance
                                             1e-4), gradients within 4.2e-4 of the largest entry (tolerance 5e-3; exact fp32: 1.5e-4).  Other entry
                                             points ignore it.                                                                          */

int32_t vsrd_abi_version(void);
const char* vsrd_error_string(int32_t code);

/* Bytes of scratch vsrd_render_backward needs for a field of N instances (residual != 0: with per-instance MLP). */
size_t vsrd_workspace_bytes(int32_t num_instances, int32_t residual);

/* Bytes of scratch with which vsrd_render_backward runs its fastest form for a launch of num_rays rays with num_distances sorted
 * distances each (>= vsrd_workspace_bytes).  Residual fields: the adjoint of renderers.py:177-270 through the per-instance MLPs
 * (scripts/main.py:433-458) runs as two kernels per chunk of rays -- the renderer's part, then the MLP adjoints by instance over the
 * whole chunk, as in vsrd_render_residual_step -- when the workspace holds the seeds of at least min(num_rays, 64) rays (2560 bytes per
 * (ray, instance, 64-sample round)); with less it keeps the one-kernel form (one wave per SIMD). */
size_t vsrd_render_backward_workspace_bytes(int32_t num_instances, int32_t residual, int32_t num_distances, int32_t num_rays);

/* The same fusion for RESIDUAL fields (BASELINE config 3; the reference's steps after warm-up): two-pass render + silhouette BCE
 * (scripts/main.py:653-671) + eikonal term (main.py:679-687: mean over all R (2S-1) samples of (|grad sdf| - 1)^2) + adjoint, one
 * launch.  The differentiated quantity is  losses[0] + eikonal_ratio * losses[1]  with
 *   losses[0] = sum_{r,n} w_n BCE(...) * loss_scale      losses[1] = mean (|grad sdf| - 1)^2 ;
 * grad_instances [N,16] and grad_mlp_weights [N,1617] are its gradients.  Needs vsrd_residual_step_workspace_bytes(N, S, R) of
 * scratch (seeds of the MLP adjoint for a chunk of rays: the launch is cut into chunks of at most 3 GiB of them).
 * VSRD_FLAG_SKIP_EXACT_MISSES is ignored (the eikonal term needs every ray). */
size_t vsrd_residual_step_workspace_bytes(int32_t num_instances, int32_t num_samples, int32_t num_rays);
int32_t vsrd_render_residual_step(const vsrd_field* field, const vsrd_render_config* config,
                                  const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                  const float* targets /* [R,N] */, const float* instance_weights /* [N] or NULL */, float loss_scale,
                                  float eikonal_ratio, void* workspace, size_t workspace_bytes,
                                  float* losses /* [2] */, float* grad_instances, float* grad_mlp_weights, float* labels /* [R,N] or NULL */,
                                  void* stream);

/* vsrd_render_residual_step with a per-frame header (mixed batches, "frame batches" above): the two-kernel form whose front kernel splits
 * a ray over a pair of waves (launches of <= 2048 rays per frame, or S > 64), one chunk of rays, no sample outputs; VSRD_E_UNSUPPORTED
 * otherwise.  The MLP adjoint's work items of instances >= n_f find no seeds and do nothing; its item geometry depends on the capacity only. */
int32_t vsrd_render_residual_step_with_header(const vsrd_field* field, const vsrd_render_config* config,
                                              const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                              const float* targets, const float* instance_weights, float loss_scale,
                                              float eikonal_ratio, void* workspace, size_t workspace_bytes,
                                              float* losses, float* grad_instances, float* grad_mlp_weights, float* labels,
                                              const vsrd_frame_header* frame_header, void* stream);

/* Hungarian matching of predicted to ground-truth 2-D boxes of the target view (scripts/main.py:374-386:
 * scipy.optimize.linear_sum_assignment(-torchvision.ops.distance_box_iou(pd, gt).cpu())), on the device -- no host
 * synchronisation, capturable in a hipGraph.  pd_boxes [P,4], gt_boxes [G,4] (x1,y1,x2,y2), 1 <= P,G <= 64.
 * pd_indices / gt_indices [min(P,G)] (int64): the matched pairs ordered by pd index, exactly what scipy returns
 * (same shortest-augmenting-path algorithm, float64 duals, same tie rule). */
int32_t vsrd_match_boxes(const float* pd_boxes, const float* gt_boxes, int32_t num_pd, int32_t num_gt,
                         int64_t* pd_indices, int64_t* gt_indices, void* stream);

/* The assignment alone on a given cost matrix [P,G] (float32, row-major): scipy.optimize.linear_sum_assignment(cost). */
int32_t vsrd_linear_sum_assignment(const float* cost, int32_t num_rows, int32_t num_cols,
                                   int64_t* row_indices, int64_t* col_indices, void* stream);

/* Importance sampling of rays (scripts/main.py:620-627: torch.multinomial(weights, num_rays, replacement=False)): num_samples
 * (<= 2048) distinct indices with probability proportional to weights [count] (>= 0), by ATen's own algorithm (exponential race,
 * keep the largest keys) with Philox4x32-10 keyed by (seed, stream_offset; index); deterministic in its arguments.
 * device_stream_offset (device memory, may be NULL) replaces stream_offset (hipGraph replay).  Needs vsrd_sample_rays_workspace_bytes()
 * of scratch.  indices [num_samples] int64, best key first; -1 fills the tail when fewer than num_samples weights are positive. */
size_t vsrd_sample_rays_workspace_bytes(void);
int32_t vsrd_sample_rays(const float* weights, int64_t count, int32_t num_samples, uint64_t seed, uint64_t stream_offset,
                         const uint64_t* device_stream_offset, void* workspace, size_t workspace_bytes, int64_t* indices, void* stream);

/* The same draw for weights that stay fixed over many calls (a frame's soft masks do not change over its 3000 steps,
 * scripts/main.py:204-265, 620-627): vsrd_ray_table_build turns weights [count] into a table once (fixed-point weights and their
 * 64-bit integer prefix sums: exact, so the table does not depend on the order of summation), and vsrd_sample_rays_table draws from it
 * in ONE single-workgroup launch: i.i.d. picks from the table in a fixed order, Philox4x32-10 keyed by (seed, stream_offset; pick
 * number), repeats skipped, the first num_samples (<= 2048) distinct picks kept -- successive sampling without replacement, the
 * distribution of torch.multinomial(replacement=False) and of vsrd_sample_rays (the sequences themselves differ from theirs).
 * remap (may be NULL): indices[i] = remap[pick] (the caller's compaction of the positive weights).  Skipping repeats needs about
 * num_samples / (weight mass outside the num_samples - 1 heaviest entries) picks; a call gives up after 32768, fills the rest with
 * repeats of its first picks and sets a sticky flag in the table (the uint32 at byte 28; reading it back is a host
 * synchronisation), so callers check that mass once per table and keep vsrd_sample_rays for weights that fail it
 * (vsrd_amd/rendering/samplers.py::RayTable.suits).
 * count < 2^32 - 1.  Fewer than num_samples positive weights: -1 fills the tail, as above. */
size_t vsrd_ray_table_bytes(int64_t count);
int32_t vsrd_ray_table_build(const float* weights, int64_t count, void* table, size_t table_bytes, void* stream);
int32_t vsrd_sample_rays_table(void* table, int64_t count, int32_t num_samples, uint64_t seed, uint64_t stream_offset,
                               const uint64_t* device_stream_offset, const int64_t* remap, int64_t* indices, void* stream);

/* vsrd.rendering.ray_casting (vsrd/rendering/utils.py:5-18), the per-pixel part:
 * directions[v,y,x,:] = normalize(inverse_projection[v] @ (x, y, 1)), integer pixel centres.
 * inverse_projection [V,9] = inv(E)[:3,:3] @ inv(K) (row-major), computed by the caller. */
int32_t vsrd_ray_directions(const float* inverse_projection, int32_t num_views, int32_t height, int32_t width,
                            float* directions /* [V,H,W,3] */, void* stream);

/* Evaluate the field at arbitrary points: what calling the distance_field closure does
 * (scripts/main.py:477-492) plus the autograd normal of renderers.py:76-113 / :218-228.
 * Any of distances [P], gradients [P,3], labels [P,N] may be NULL.
 * hard_union != 0 selects the arg-min union of scripts/main.py:494-509 (distances only). */
int32_t vsrd_field_eval(const vsrd_field* field, const float* positions /* [P,3] */, int64_t num_points,
                        float* distances, float* gradients, float* labels, int32_t hard_union, void* stream);

/* Adjoint of vsrd_field_eval w.r.t. the field parameters and the positions: the reference's closure call is differentiable
 * (autograd), e.g. sphere_tracing(differentiable=True) (renderers.py:59-72).  grad_distances [P] and/or grad_labels [P,N] (soft
 * union only) may be NULL.  This entry takes no cotangent of the `gradients` output: it is vsrd_field_eval_adjoint (below) with
 * grad_gradients = NULL, bit for bit, except that it also accepts a call without any cotangent (all gradients are zero then).
 * Needs vsrd_workspace_bytes(N, residual) of scratch.  grad_positions [P,3] or NULL; grad_instances [N,16];
 * grad_mlp_weights [N,1617] (required for residual fields). */
int32_t vsrd_field_eval_backward(const vsrd_field* field, const float* positions, int64_t num_points,
                                 const float* grad_distances, const float* grad_labels, int32_t hard_union,
                                 void* workspace, size_t workspace_bytes, float* grad_positions,
                                 float* grad_instances, float* grad_mlp_weights, void* stream);

/* The full adjoint of vsrd_field_eval, the analytic normal included (second order): the reference's surface_normal
 * (renderers.py:100-109) takes the normal with create_graph, so the normal is differentiable w.r.t. the boxes, the residual-MLP
 * weights and the positions, and the photometric term (scripts/main.py:747-851) reaches the box rotations through it.
 * grad_gradients [P,3] is the cotangent of vsrd_field_eval's `gradients` output (the UN-normalised union gradient; soft union: through
 * the soft-min weights and every member's gradient, hard union: through the arg-min member's gradient); the box Hessian and the MLP's
 * second-order adjoint are taken where they exist -- the kinks of the box SDF (sign(p), the interior arg max, relu(q) = 0, the hard
 * arg min) contribute nothing, as in autograd.  Contract of vsrd_field_eval_backward: same workspace, same refusals, no allocation, no
 * host synchronisation, deterministic; in addition at least one of grad_distances, grad_labels, grad_gradients must be non-NULL.
 * Added within ABI 12: probe for the symbol. */
int32_t vsrd_field_eval_adjoint(const vsrd_field* field, const float* positions, int64_t num_points,
                                const float* grad_distances /* [P] or NULL */, const float* grad_labels /* [P,N] or NULL, soft only */,
                                const float* grad_gradients /* [P,3] or NULL: cotangent of vsrd_field_eval's `gradients` */,
                                int32_t hard_union, void* workspace, size_t workspace_bytes,
                                float* grad_positions, float* grad_instances, float* grad_mlp_weights, void* stream);

/* vsrd.rendering.sphere_tracing, non-differentiable part (renderers.py:21-59): the reference's loop without its batch-wide early exit,
 * so that a ray's outputs depend on that ray alone -- not on its place in the launch nor on the other rays (the loop with and without
 * that exit gives identical output on every fixture: tests/test_sphere_trace_reference.py).  Per iteration: evaluate the
 * union distance d at the position; move by d along the direction if the ray is foreground and was not converged by the previous
 * iteration; clear foreground (for good) once the position is on or beyond the bounding sphere; set converged = |d| < convergence_criteria.
 * converged is overwritten in every iteration: a converged ray stays put for one iteration and is judged again by the distance at the
 * point it reached; a ray that stepped past a rim un-converges and marches on.  A ray is finished, before num_iterations, only once
 * it is stationary (it did not move and may not move next).  A ray that is not foreground never moves; its flag is |d| < criteria at
 * its position.  A position that is not finite is never converged.  num_iterations = 0: positions are the origins (or entry points),
 * converged 0.
 * origins [R,3] (origin_stride 3) or [3] (stride 0); foreground [R] uint8 or NULL (= all finite origins);
 * bounding_radius <= 0: none; initialise != 0: start from the bounding-sphere entry point (renderers.py:36-43).
 * Outputs: positions [R,3], converged [R] uint8 (the reference's convergence_masks). */
int32_t vsrd_sphere_trace(const vsrd_field* field, const float* origins, int32_t origin_stride, const float* directions,
                          const uint8_t* foreground, int64_t num_rays, int32_t num_iterations, float convergence_criteria,
                          float bounding_radius, int32_t initialise, int32_t hard_union,
                          float* positions, uint8_t* converged, void* stream);

/* SoftRasterizer.make_distance_map + soft masks (vsrd/transforms/geometric_transforms.py:265-317), the step that produces the
 * path's targets: per instance, distance of every pixel to the closed polygon [count,2] (x,y), then
 * soft = sigmoid((inside ? d : -d) / temperature).  polygons [B,Pmax,2] (rows beyond counts[b] ignored), counts [B] int32,
 * inside [B,H,W] uint8 (required for soft_masks).  distance_maps / soft_masks [B,H,W], either may be NULL. */
int32_t vsrd_polygon_soft_masks(const float* polygons, const int32_t* counts, int32_t num_polygons, int32_t max_vertices,
                                int32_t height, int32_t width, const uint8_t* inside, float temperature,
                                float* distance_maps, float* soft_masks, void* stream);

/* Frame ingest (ABI 10): one frame's compact pack (vsrd_amd/frames.py: one polygon and one bit-packed binary mask per (view, instance)
 * ENTRY, as the reference's dataset keeps them) straight into the buffers a frame's step reads -- SoftRasterizer
 * (geometric_transforms.py:265-317), BoxGenerator (:151-159), the re-indexing of every view to the target's instance order
 * (scripts/main.py:204-265) and the importance weights (main.py:620-624) in one call, with no [V,H,W,N] temporary.
 *   polygon_vertices [num_vertices,2] int32 (x, y), all entries concatenated; polygon_offsets [num_entries + 1] int32 (every entry has
 *   at least one vertex; one vertex is a single-pixel contour, two a line);
 *   entry_table [V,N] int32, IN/OUT: the entry of (view, target slot), -1 where the instance is absent from the view.  An entry without a
 *   set bit counts as invisible: the call REPLACES it by -1 (so do entries that do not address the pack);
 *   inside [num_entries, H, ceil(W/8)] uint8: the binary masks, eight pixels per byte, most significant bit first (numpy.packbits);
 *   target_stride >= N: the row's capacity, the stride of every output's instance axis.  V <= 32, N <= VSRD_MAX_INSTANCES.
 * Outputs, each may be NULL; only instances 0..N-1 are written, columns N..target_stride-1 are left alone:
 *   soft_masks [V*H*W, target_stride]: sigmoid((inside ? d : -d) / temperature), d the distance of the pixel centre to the closed polygon
 *     with the reference's + 1e-6 in the projection's denominator; exactly 0.0 for an invisible pair (16-byte stores when target_stride
 *     is a multiple of 4 and the buffer is 16-byte aligned);
 *   sampling_weights [V*H*W]: the maximum over the N written columns, bit-equal to amax of them;
 *   gt_boxes [V, target_stride, 4]: (xmin, ymin, xmax, ymax) of the set bits as inclusive pixel indices, zeros for an invisible pair.
 *     These are the extremes of the ENTRY's bits -- the filled largest contour.  The reference's BoxGenerator takes the extremes of
 *     `masks > threshold`, every component of the mask: the two agree for masks of one component; a mask with detached parts gets the box
 *     of its largest part here;
 *   visible [V, target_stride] uint8.
 * vsrd_frame_ingest_chunk(): the polygon sides the pixel pass stages per round (longer polygons take several rounds). */
int32_t vsrd_frame_ingest_chunk(void);
int32_t vsrd_frame_ingest(const int32_t* polygon_vertices, int32_t num_vertices, const int32_t* polygon_offsets, int32_t num_entries,
                          int32_t* entry_table, const uint8_t* inside, int32_t height, int32_t width, int32_t num_views, int32_t num_instances,
                          int32_t target_stride, float temperature, float* soft_masks, float* sampling_weights, float* gt_boxes,
                          uint8_t* visible, void* stream);

/* samplers.quadrature_sampler over linspace bins (renderers.py:191-194, samplers.py:5-8).
 * u_coarse [R,S] in [0,1) -> distances [R,S]. */
int32_t vsrd_sample_stratified(const vsrd_render_config* config, const float* u_coarse, float* distances, void* stream);

/* Pass-2 distances: cat(coarse, inverse_transform_sampler(coarse, weights)) sorted
 * (renderers.py:198-210, samplers.py:11-36).  coarse_distances [R,S], coarse_weights [R,S-1],
 * u_fine [R,S] (raw draws, or sorted with VSRD_FLAG_FINE_UNIFORMS_SORTED) -> merged [R,2S] and/or the sampler's own
 * output fine [R,S] (either may be NULL). */
int32_t vsrd_sample_importance(const vsrd_render_config* config, const float* coarse_distances,
                               const float* coarse_weights, const float* u_fine, float* merged, float* fine, void* stream);

/* renderers.py:212-270 for given sorted distances [R,D]: evaluates the field and its normal at
 * the D-1 interval mid-points, converts to opacities, composites front to back.
 * Outputs: labels [R,N]; gradients [R,D-1,3] (may be NULL); weights [R,D-1] (may be NULL). */
int32_t vsrd_render_forward(const vsrd_field* field, const vsrd_render_config* config,
                            const float* origins, const float* directions,
                            const float* distances, int32_t num_distances,
                            float* labels, float* gradients, float* weights, void* stream);

/* Adjoint of vsrd_render_forward w.r.t. the packed instances (what autograd, including the
 * double-backward through the SDF normal, produces in the reference -- renderers.py:218-228).
 * grad_labels [R,N]; grad_gradients [R,D-1,3] or NULL; grad_weights [R,D-1] or NULL.
 * grad_instances [N,16] is OVERWRITTEN (pad column = 0); grad_mlp_weights [N,1617] likewise (required iff the field
 * carries mlp_weights, else NULL).  workspace: vsrd_workspace_bytes(N, residual). */
int32_t vsrd_render_backward(const vsrd_field* field, const vsrd_render_config* config,
                             const float* origins, const float* directions,
                             const float* distances, int32_t num_distances,
                             const float* grad_labels, const float* grad_gradients, const float* grad_weights,
                             void* workspace, size_t workspace_bytes,
                             float* grad_instances, float* grad_mlp_weights, void* stream);

/* The two-pass wrapper scripts/main.py:511-523 around renderers.py:177-270 in ONE launch:
 * pass 1 (stratified, no grad) -> importance sampling -> merge -> pass 2.
 * u_coarse / u_fine [R,S]: recorded uniforms, or NULL -> Philox4x32-10 keyed by (seed, stream_offset, ray).
 * Outputs: labels [R,N]; distances [R,2S] (needed by vsrd_render_backward; may be NULL for
 * inference); gradients [R,2S-1,3] / weights [R,2S-1] may be NULL;
 * coarse_weights [R,S-1] (may be NULL; ABI 7): pass 1's compositing weights, i.e. the `sampled_weights` pass 1 of
 * main.py:511-523 returns and samplers.py:11-36 turns into the importance samples (its `sampled_distances` are
 * torch.lerp(linspace bins, u_coarse), vsrd_sample_stratified);
 * u_coarse_out / u_fine_out [R,S] (may be NULL) export the uniforms actually used (u_fine_out: SORTED when they
 * were generated in the kernel).  Box-only launches that ask for neither `gradients` nor `weights` run in the
 * fused step's own mappings (several rays per wave), so these outputs are the step kernels' own pass-1 state. */
int32_t vsrd_render_hierarchical_forward(const vsrd_field* field, const vsrd_render_config* config,
                                         const float* origins, const float* directions,
                                         const float* u_coarse, const float* u_fine,
                                         float* labels, float* distances, float* gradients, float* weights, float* coarse_weights,
                                         float* u_coarse_out, float* u_fine_out, void* stream);

/* One fused optimisation-step launch for box-only fields: the two-pass render of vsrd_render_hierarchical_forward, the
 * silhouette loss of scripts/main.py:653-671  --  loss = loss_scale * sum_{r,n} w_n BCE(clamp(labels[r,n], 1e-6, 1-1e-6), targets[r,n])
 * --  and its gradient w.r.t. the packed instances, without writing any per-sample data to HBM.
 * targets [R,N] in prediction order; instance_weights [N] or NULL (all 1; 0 drops an unmatched instance);
 * loss_scale = 1 / (R * number of kept instances) gives the reference's mean.  Outputs: loss [1], grad_instances [N,16]
 * (d loss / d instances), labels [R,N] or NULL.  workspace: vsrd_workspace_bytes(N, 0). */
int32_t vsrd_render_silhouette_step(const vsrd_field* field, const vsrd_render_config* config,
                                    const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                    const float* targets, const float* instance_weights, float loss_scale,
                                    void* workspace, size_t workspace_bytes,
                                    float* loss, float* grad_instances, float* labels, void* stream);

/* vsrd_render_silhouette_step with a per-frame header (mixed batches, "frame batches" above): the split-ray form only. */
int32_t vsrd_render_silhouette_step_with_header(const vsrd_field* field, const vsrd_render_config* config,
                                                const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                                const float* targets, const float* instance_weights, float loss_scale,
                                                void* workspace, size_t workspace_bytes,
                                                float* loss, float* grad_instances, float* labels, const vsrd_frame_header* frame_header, void* stream);

/* Multi-view projection of N boxes (8 corners each, world frame) into V cameras and reduction to clipped 2-D boxes:
 * scripts/main.py:339-362 = einsum with E + divide by w, vsrd.operations.project_box_3d / clip_lines_to_front
 * (geometric_operations.py:343-389) per box, torchvision.ops.clip_boxes_to_image.  One launch for all V*N boxes.
 * world_corners [N,8,3]; extrinsics [V,16]; intrinsics [V,9] (row-major); edges [E,2] corner indices (E <= 32).
 * height/width <= 0 skips the image clamp (plain project_box_3d).
 * Outputs: boxes_2d [V,N,4] = (x1,y1,x2,y2); camera_corners [V,N,8,3] or NULL; selection [V,N,4] (int32: which edge end
 * point attained each extreme, -1 = no gradient) -- consumed by the backward. */
int32_t vsrd_project_boxes_forward(const float* world_corners, const float* extrinsics, const float* intrinsics,
                                   const int32_t* edges, int32_t num_edges, int32_t num_views, int32_t num_boxes,
                                   int32_t height, int32_t width, float epsilon,
                                   float* boxes_2d, float* camera_corners, int32_t* selection, void* stream);

/* Adjoint of the above (torch min/max/clamp/where backward semantics): grad_boxes_2d [V,N,4] ->
 * grad_world_per_view [V,N,8,3]; the caller sums over V (fixed order: deterministic). */
int32_t vsrd_project_boxes_backward(const float* world_corners, const float* extrinsics, const float* intrinsics,
                                    const int32_t* edges, int32_t num_edges, int32_t num_views, int32_t num_boxes, float epsilon,
                                    const float* grad_boxes_2d, const int32_t* selection, float* grad_world_per_view, void* stream);

/* ---- the rest of one optimisation step of scripts/main.py around the render launch, for <= 64 boxes and <= 32 views ------------
 * In the reference these are a few hundred small ATen launches per step (box decode, V x N project_box_3d calls, DIoU matching
 * through scipy on the host, projection losses, schedules, autograd through all of it, Adam, ExponentialLR); here two
 * single-workgroup launches, so that the reference's native mode (1000 rays per step) is bound by its render launch. */
typedef struct vsrd_frame_config {
    int32_t num_boxes;              /* N (predictions = ground-truth slots, main.py:204-265 pads the sources to the target's N) */
    int32_t num_views;              /* V, view 0 = target view                                                               */
    float height, width;            /* image size for clip_boxes_to_image                                                     */
    float epsilon;                  /* project_box_3d / clip_lines_to_front guard, 1e-6                                       */
    float location_lo[3], location_hi[3];     /* BoxParameters3D.location_range (box_parameters.py:23-26)                     */
    float dimension_lo[3], dimension_hi[3];   /* BoxParameters3D.dimension_range (box_parameters.py:27-30)                    */
    int32_t num_steps;              /* optimisation steps of the schedules (config.json:167)                                  */
    float max_temperature, min_temperature, max_std, min_std;   /* config.json:230-233                                        */
    float weight_iou, weight_l1, weight_silhouette;             /* config.json:120-127                                        */
    float beta1, beta2, adam_epsilon; /* torch.optim.Adam defaults 0.9, 0.999, 1e-8                                           */
    float lr_gamma;                 /* ExponentialLR gamma (config.json:209-215)                                              */
    int32_t num_frames;             /* frame batch (ABI 8, "frame batches" above): 0 or 1 = one frame                         */
    int64_t frame_stride;           /* bytes between the frames' copies of every buffer of the call                           */
} vsrd_frame_config;

size_t vsrd_frame_scratch_bytes(int32_t num_views, int32_t num_boxes);

/* Before the render launch.  scripts/main.py:332 (BoxParameters3D.forward, box_parameters.py:124-146), :339-367 (projection),
 * :374-386 (matching: -DIoU + linear_sum_assignment, as vsrd_match_boxes), :391-415 (distance_box_iou_loss + smooth_l1_loss over
 * matched, visible instances), :420-431 (schedules from the device step counter).
 * raw_locations / raw_dimensions [N,3], raw_orientations [N,2]; extrinsics [V,16], intrinsics [V,9]; gt_boxes [V,N,4];
 * visible [V,N] uint8 (by ground-truth instance); step [1] int64 (device).
 * Outputs: instances [N,16] (the renderer's field block); pd_indices / gt_indices [N] int64; target_columns [N] int32 and
 * instance_weights [N] (for vsrd_render_config.target_columns / the step entry points); schedule [3] (for
 * vsrd_render_config.device_schedule); projection_losses [2] = (iou, l1); grad_raw [N,8] = d (weight_iou * iou + weight_l1 * l1) /
 * d (raw location 3 | raw dimension 3 | raw orientation 2). */
int32_t vsrd_frame_prologue(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                            const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                            const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                            float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                            float* schedule, float* projection_losses, float* grad_raw, void* stream);

/* vsrd_frame_prologue and the draw of the step's rays (vsrd_sample_rays_table keyed by the same device step counter `step`) in ONE launch
 * of two workgroups: neither needs the other, and as two launches on two streams they meet again through a cross-queue dependency that
 * costs as much as the draw itself.  ray_table / count / remap as for vsrd_sample_rays_table; ray_indices [num_rays] int64 out. */
int32_t vsrd_frame_prologue_sample(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                                   const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                                   const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                                   float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                                   float* schedule, float* projection_losses, float* grad_raw,
                                   void* ray_table, int64_t count, int32_t num_rays, uint64_t seed, const int64_t* remap, int64_t* ray_indices, void* stream);

/* The two prologues with a per-frame header (mixed batches, "frame batches" above): num_boxes is the capacity, the stride of gt_boxes
 * [V,N,4] and visible [V,N]; decode, projection, the matching (an n_f x n_f problem) and the projection losses cover the frame's n_f boxes. */
int32_t vsrd_frame_prologue_with_header(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                                        const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                                        const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                                        float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                                        float* schedule, float* projection_losses, float* grad_raw, const vsrd_frame_header* frame_header, void* stream);
int32_t vsrd_frame_prologue_sample_with_header(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                                               const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                                               const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                                               float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                                               float* schedule, float* projection_losses, float* grad_raw,
                                               void* ray_table, int64_t count, int32_t num_rays, uint64_t seed, const int64_t* remap, int64_t* ray_indices,
                                               const vsrd_frame_header* frame_header, void* stream);

/* torch.optim.Adam(capturable=True) state of one parameter tensor: all device memory, updated in place. */
typedef struct vsrd_adam_tensors {
    float* parameter;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;                    /* [1] float32                                                                            */
    float* learning_rate;           /* [1] float32, multiplied by lr_gamma after the update (ExponentialLR)                   */
} vsrd_adam_tensors;

/* After the render launch.  scripts/main.py:855-865: total loss, backward through the decode (box_parameters.py:60-90), Adam step
 * on locations / dimensions / orientations, scheduler step, step counter.  grad_instances [N,16] = d (silhouette + eikonal_ratio *
 * eikonal) / d instances from the render step; grad_raw_projection [N,8] and projection_losses [2] from the prologue;
 * render_losses [2] = (silhouette, eikonal).  other_learning_rates: two more [1] float32 rates decayed by lr_gamma (embeddings,
 * hypernetwork groups), either may be NULL.  Outputs: record [5] = (iou, l1, silhouette, eikonal, total); raw_gradients [N,8] or NULL. */
int32_t vsrd_frame_epilogue(const vsrd_frame_config* config, const float* grad_instances, const float* grad_raw_projection,
                            const float* projection_losses, const float* render_losses, float eikonal_ratio,
                            const vsrd_adam_tensors* locations, const vsrd_adam_tensors* dimensions, const vsrd_adam_tensors* orientations,
                            float* other_learning_rate_0, float* other_learning_rate_1, int64_t* step,
                            float* record, float* raw_gradients, void* stream);

/* vsrd_frame_epilogue with a per-frame header (mixed batches, "frame batches" above): Adam on the frame's n_f boxes. */
int32_t vsrd_frame_epilogue_with_header(const vsrd_frame_config* config, const float* grad_instances, const float* grad_raw_projection,
                                        const float* projection_losses, const float* render_losses, float eikonal_ratio,
                                        const vsrd_adam_tensors* locations, const vsrd_adam_tensors* dimensions, const vsrd_adam_tensors* orientations,
                                        float* other_learning_rate_0, float* other_learning_rate_1, int64_t* step,
                                        float* record, float* raw_gradients, const vsrd_frame_header* frame_header, void* stream);

/* Frame labels (ABI 11): a frame's pseudo-labels from the buffers its steps read, at the end of the optimisation -- the second pass of
 * tools/kitti_360/make_predictions.py:61-192 in ONE single-workgroup launch per frame, no host synchronisation, no allocation, capturable:
 * decode the boxes (box_parameters.py:124-146), camera corners = E_v corner / w and project_box_3d + clip_boxes_to_image in every view
 * (main.py:339-362), torchvision.ops.box_iou against every view's ground-truth boxes (no epsilon; a NaN, 0/0, counts as 0: nan_to_num),
 * the mean over the views in which the ground-truth instance exists (summed in ascending view order), then
 * scipy.optimize.linear_sum_assignment(mean_iou, maximize=True) -- the solver of vsrd_linear_sum_assignment on -mean_iou, ties included --
 * and confidence = the matched mean IoU.
 * The inputs and their conventions are those of vsrd_frame_prologue_with_header: config->num_boxes is the capacity N and the stride of
 * every instance axis, num_views V <= 32, N <= VSRD_MAX_INSTANCES, num_frames / frame_stride batch the call, frame_header (may be NULL:
 * every frame has N boxes) carries the frame's own count n_f, clamped to [1, N].  Of config, the call reads the sizes, height / width /
 * epsilon, the location and dimension ranges and the batch fields.  gt_boxes [V,N,4] and visible [V,N] are in the target's instance
 * order (the table of make_predictions.py:142-162 is applied by vsrd_frame_ingest or by the caller), the extrinsics relative to the
 * target view (make_predictions.py:74-109).
 * Outputs, each may be NULL and is then skipped; entries of instances n_f .. N-1 are never read and never written (the rows and columns
 * of mean_iou beyond n_f included):
 *   camera_corners [V,N,8,3]  the boxes' corners in every view's camera frame, the reference's corner order;
 *   boxes_2d [V,N,4]          (x1, y1, x2, y2), clipped to the image;
 *   mean_iou [N,N]            [p,g]: prediction p against ground-truth slot g;
 *   matched_gt [N]            the slot matched to prediction p;
 *   confidences [N]           mean_iou[p, matched_gt[p]], bit for bit.
 * A stated deviation: a ground-truth slot that NO view sees gets mean_iou exactly 0.0 in its column, where the reference divides 0 by 0
 * and scipy raises on the NaN (vsrd_frame_ingest produces such slots: a target entry without a set bit). */
int32_t vsrd_frame_labels(const vsrd_frame_config* config,
                          const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                          const float* extrinsics, const float* intrinsics, const float* gt_boxes, const uint8_t* visible,
                          float* camera_corners /* [V,N,8,3] */, float* boxes_2d /* [V,N,4] */, float* mean_iou /* [N,N] */,
                          int64_t* matched_gt /* [N] */, float* confidences /* [N] */,
                          const vsrd_frame_header* frame_header /* may be NULL */, void* stream);

/* Frame group labels (added within ABI 12; probe for the symbol -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field):
 * vsrd_frame_labels in label views of the call's own, any number up to VSRD_MAX_LABEL_VIEWS -- the frame's GROUP, what
 * tools/kitti_360/make_predictions.py:50-192 labels: every frame of grouped_image_filenames.txt whose filtered instance-id set equals the
 * target's (sample_annotations.py:133,164-170).  The views a frame is optimised on are another set (the target and the medians of at most 16
 * chunks of its sources, of which a source needs only half the target's instances): a group can hold far more frames, and need not hold
 * the sources.  Up to three launches inside the call, ordered by the stream, no host synchronisation, no allocation, capturable:
 *   project    (blocks of four label views, frame): a wave per view, a lane per box -> camera_corners, boxes_2d;
 *   mean IoU   (blocks of four predictions, frame): a wave per prediction, a lane per ground-truth slot, every lane sums its own pair
 *              over the views in ascending order -> mean_iou;
 *   assign     one wave per frame -> matched_gt, confidences (skipped when both are NULL).
 * Semantics are vsrd_frame_labels' step by step with the label views in place of the row's views -- the same device functions: handed a
 * row's own E, K, gt_boxes and visible, the call writes the bits vsrd_frame_labels writes.  The stated deviation is the same (a slot NO
 * label view sees: mean_iou exactly 0.0 in its column).
 * Conventions as for vsrd_frame_labels: config->num_boxes is the capacity N (1..VSRD_MAX_INSTANCES) and the stride of every instance axis,
 * num_frames / frame_stride batch the call, frame_header (may be NULL) carries n_f, clamped to [1, N], VSRD_FRAME_HEADER_HAS_VIEWS masked
 * off.  config->num_views and the header's num_views are NOT read: of config the call reads num_boxes, height / width / epsilon, the
 * location and dimension ranges and the batch fields.
 *   num_label_views L         capacity and stride of every label-view axis, 1..VSRD_MAX_LABEL_VIEWS;
 *   label_view_count [1]      device, per frame (it follows frame_stride like every other pointer): the frame's own l_f, clamped to [1, L]
 *                             (a group always holds its target); NULL: every frame has L;
 *   label_extrinsics [L,16], label_intrinsics [L,9]   relative to the rectified target view, like a row's own;
 *   label_gt_boxes [L,N,4], label_visible [L,N]        in the target's instance order.
 * Views l_f .. L-1 of every label-view input and output are never read and never written; instances n_f .. N-1 are never read and never
 * written, rows and columns of mean_iou included.  camera_corners, matched_gt and confidences may each be NULL and are then skipped;
 * boxes_2d and mean_iou are REQUIRED (the next kernel reads them back).  A NULL required pointer, L outside 1..VSRD_MAX_LABEL_VIEWS or N
 * outside 1..VSRD_MAX_INSTANCES: VSRD_E_INVALID_ARGUMENT before any launch, nothing written. */
#define VSRD_MAX_LABEL_VIEWS 4096
int32_t vsrd_frame_group_labels(const vsrd_frame_config* config,
                                const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                                int32_t num_label_views, const int32_t* label_view_count /* [1] or NULL */,
                                const float* label_extrinsics /* [L,16] */, const float* label_intrinsics /* [L,9] */,
                                const float* label_gt_boxes /* [L,N,4] */, const uint8_t* label_visible /* [L,N] */,
                                float* camera_corners /* [L,N,8,3] or NULL */, float* boxes_2d /* [L,N,4] */, float* mean_iou /* [N,N] */,
                                int64_t* matched_gt /* [N] */, float* confidences /* [N] */,
                                const vsrd_frame_header* frame_header /* may be NULL */, void* stream);

/* Frame masks (added within ABI 12; probe for the symbol -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field): the dense
 * predicted instance masks of ONE view of a frame, bit-packed -- what the reference renders every `image_intervals` steps
 * (scripts/main.py:1011-1061): volume_masks (the two-pass hierarchical_volumetric_rendering of the soft union at every pixel) times
 * surface_masks (sphere_tracing(..., initialization=False, differentiable=False)[1]) -- in ONE launch (plus a single-workgroup launch
 * that zeroes `counts`), no host synchronisation, no allocation, capturable.  A wave traces a run of 64 pixels of an image row, one lane
 * each, and then renders only the pixels whose trace converged; a run without one renders nothing.
 * Conventions as for the *_with_header twins: field->num_instances is the capacity N and the stride of every instance axis;
 * config->num_frames / frame_stride batch the call (every pointer addresses frame 0, frame f lies f * frame_stride bytes behind it);
 * frame_header (may be NULL: every frame has N instances) carries the frame's own n_f, clamped to [1, N], VSRD_FRAME_HEADER_HAS_VIEWS
 * masked off; instances n_f .. N-1 of every output are neither read nor written.  config->device_schedule / device_stream_offset are
 * honoured as in the step kernels; config->num_rays is ignored (the ray count is H W); config->ray_indices, out_* and target_columns
 * inside `config` are rejected, like `view` outside 0 .. num_views-1, N outside 1..VSRD_MAX_INSTANCES, num_samples outside what
 * vsrd_render_hierarchical_forward's one-ray kernel serves (2..256 box-only, 2..128 residual), and `targets` without `counts` or the
 * reverse: VSRD_E_INVALID_ARGUMENT.  The residual form evaluates the MLPs with the exact-fp32 products (VSRD_FLAG_MLP_SPLIT_BF16 is ignored).
 * Pixel p = y W + x of view `view`: origin camera_positions[view], direction ray_directions[view H W + p];
 *   converged = what vsrd_sphere_trace computes with the soft union, foreground = NULL, initialise = 0 (bounding_radius <= 0: none);
 *   labels[N] = what vsrd_render_hierarchical_forward's one-ray kernel computes for that ray at the launch's schedule: ray p uses row p
 *               of u_coarse / u_fine [H W, S], or with NULL the Philox stream keyed by (seed, stream_offset, ray = p);
 *   soft[p, n] = converged ? labels[n] : 0.0f (exactly 0 where the trace did not converge);
 *   bit (n, y, x) = soft[p, n] > threshold, laid out as numpy.packbits of [N, H, W] along W: most significant bit first, pad bits of a
 *               row's last byte 0 -- the `inside` layout of vsrd_frame_ingest;
 *   counts[n] = (#pred, #target, #pred and target) over the view's pixels, target bit = targets[view H W + p, col] > threshold with
 *               col = target_columns ? target_columns[n] : n (a negative column: no target bit); int32, integer atomics, zeroed by the
 *               call itself for n < n_f. */
typedef struct vsrd_frame_masks_config {
    int32_t view;               /* which view of the row, 0 = target                                              */
    int32_t num_views;          /* V (the view capacity of the row): rows of camera_positions, views of ray_directions / targets */
    int32_t height, width;
    int32_t num_iterations;     /* sphere_tracing, initialization=False                                           */
    float convergence_criteria;
    float bounding_radius;
    float threshold;            /* a bit is set where label * converged > threshold                               */
    int32_t target_stride;      /* columns of a flat_masks row (the capacity)                                     */
} vsrd_frame_masks_config;

int32_t vsrd_frame_masks(const vsrd_field* field, const vsrd_render_config* config, const vsrd_frame_masks_config* masks,
                         const float* camera_positions /* [V,3] */, const float* ray_directions /* [V*H*W,3] */,
                         const float* u_coarse, const float* u_fine /* [H*W,S] recorded, or NULL: Philox keyed by pixel */,
                         const float* targets /* flat_masks [V*H*W,stride] or NULL */, const int32_t* target_columns /* [N] or NULL */,
                         uint8_t* mask_bits /* [N,H,ceil(W/8)] */, float* soft /* [H*W,N] or NULL */, int32_t* counts /* [N,3] or NULL */,
                         const vsrd_frame_header* frame_header /* may be NULL */, void* stream);

/* Frame surface (added within ABI 12; probe for the symbol -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field): the dense
 * surface render of ONE view of a frame -- the surface of the field in a camera view with range, normal, owning instance, shadow and a
 * shaded image laid over the photograph: sphere_tracing, surface_normal, shadow_rendering and phong_shading (vsrd/rendering/renderers.py:21-174)
 * as the dense logging branch of scripts/main.py:1028-1041 composes them -- in ONE launch for all frames of a batch, no host synchronisation,
 * no allocation, capturable.  A wave owns a run of 64 pixels of an image row, one lane each; everything behind the primary trace is done
 * only in runs where some pixel converged.
 * Conventions as for vsrd_frame_masks: field->num_instances is the capacity N (1..VSRD_MAX_INSTANCES) and the stride of every instance axis
 * (palette); config->num_frames / frame_stride batch the call (every pointer addresses frame 0, frame f lies f * frame_stride bytes behind
 * it); frame_header (may be NULL: every frame has N instances) carries the frame's own n_f, clamped to [1, N]; instances n_f .. N-1 are
 * neither read nor written.  Of config the call reads num_frames, frame_stride and device_schedule (its temperature, as in the step
 * kernels) and nothing else.  The residual form evaluates the MLPs with the exact-fp32 products.
 * Pixel p = y W + x of view `view`: origin o = camera_positions[view], direction r = ray_directions[view H W + p];
 *   1. primary trace   what vsrd_sphere_trace computes with foreground = NULL, initialise = 0 and hard_union = (flags & VSRD_SURFACE_HARD_UNION)
 *                      -> position, converged.  Which union to trace is the caller's choice;
 *   2. surface point   (converged pixels) one evaluation of the union with its analytic gradient g, as vsrd_field_eval:
 *                      normal = g / max(|g|, 1e-12); instance = the first member with the smallest distance (the arg-min of the hard
 *                      union, the arg-max label of the soft one); range = |position - o|;
 *   3. shadow trace    (light != NULL and flags & VSRD_SURFACE_SHADOWS) the same march -- same union, iteration count, criteria and
 *                      bounding radius, no initialisation -- from position + normal * shadow_offset (product and sum rounded on their
 *                      own) along -light; shadow = converged AND this trace's converged: shadow_rendering with foreground_masks = the
 *                      primary convergence.  Without it shadow = 0;
 *   4. shade           phong_shading (renderers.py:116-146) with view = r, the normal and the light all normalised:
 *                      reflected = l - 2 n (l.n), diffuse = relu(-l.n), specular = relu(-reflected.view)^shininess,
 *                      colour = clamp(material_emission + material_ambient light_ambient
 *                                     + (1 - shadow) (palette[instance] light_diffuse diffuse + material_specular light_specular specular), 0, 1);
 *                      a converged pixel is alpha colour + (1 - alpha) background / 255, any other the background pixel itself (or
 *                      background_color when background is NULL); stored as (int)(255 c + 0.5).
 * Stated deviations from the reference:
 *   - the reference defines no way to combine shadow and shading; the (1 - shadow) factor on the diffuse and specular terms is this
 *     project's choice;
 *   - shadow_offset is a field of its own where the reference offsets by convergence_criteria c: with c a point at d(p) = delta < 0 starts
 *     its shadow ray at about delta + c < c, converges at once and reads as shadowed.  Callers should pass 2 c (the launcher's default):
 *     because d(p) > -c, d(start) ~ d(p) + 2 c > c for a field with unit gradient;
 *   - FrameOptimizer.surface() traces the hard union by default; the reference's logging trace uses the soft union (hard = False).
 * Outputs, each may be NULL and is then skipped:
 *   converged_bits, shadow_bits [H, ceil(W/8)]  numpy.packbits along W: most significant bit first, pad bits 0 (the `inside` layout);
 *   instance [H W] uint8                        255 where not converged;
 *   range [H W] float32                         exactly 0 where not converged;
 *   colors [H W,3] uint8                        needs light and palette;
 *   positions [H W,3] float32                   where not converged the position the trace ended at, as vsrd_sphere_trace writes;
 *   normals [H W,3] float32                     exactly 0 where not converged.
 * No floating-point atomics; no output depends on the grid or on where a pixel sits in the launch.
 * VSRD_E_INVALID_ARGUMENT before any launch, nothing written: a NULL field, config, surface, camera_positions or ray_directions; N outside
 * 1..VSRD_MAX_INSTANCES; view outside 0..num_views-1; height, width < 1 or num_iterations < 0; colors without light or without palette;
 * a background whose background_pixels is not H W. */
#define VSRD_SURFACE_HARD_UNION 1u
#define VSRD_SURFACE_SHADOWS 2u
typedef struct vsrd_frame_surface_config {
    int32_t view;               /* which view of the row, 0 = target                                              */
    int32_t num_views;          /* V (the view capacity of the row): rows of camera_positions, views of ray_directions */
    int32_t height, width;
    int32_t num_iterations;     /* sphere_tracing, initialization=False: both traces                              */
    float convergence_criteria;
    float bounding_radius;      /* <= 0: none                                                                     */
    float shadow_offset;        /* the shadow ray starts at position + normal * shadow_offset                     */
    uint32_t flags;             /* VSRD_SURFACE_*                                                                 */
    int32_t background_pixels;  /* H W of the `background` image; must be H W when background is given            */
    float alpha;                /* weight of the shaded colour over the background                                */
    float shininess;
    float background_color[3];  /* where nothing converged and background is NULL                                 */
    float light_ambient[3], light_diffuse[3], light_specular[3];
    float material_ambient[3], material_specular[3], material_emission[3];
} vsrd_frame_surface_config;

int32_t vsrd_frame_surface(const vsrd_field* field, const vsrd_render_config* config, const vsrd_frame_surface_config* surface,
                           const float* camera_positions /* [V,3] */, const float* ray_directions /* [V*H*W,3] */,
                           const float* light /* [3] device: the direction the light travels, or NULL */,
                           const float* palette /* [N,3] device: the instances' diffuse colours, or NULL */,
                           const uint8_t* background /* [H*W,3] or NULL */,
                           uint8_t* converged_bits, uint8_t* shadow_bits, uint8_t* instance, float* range, uint8_t* colors,
                           float* positions, float* normals,
                           const vsrd_frame_header* frame_header /* may be NULL */, void* stream);

/* Frame metrics (added within ABI 12; probe for the symbol -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field): a frame's
 * evaluation against its 3-D ground truth -- what the reference logs every `scalar_intervals` steps (scripts/main.py:870-924) -- in ONE
 * launch, one wave per frame, no host synchronisation, no allocation, capturable.  Lane k handles the matched pair
 * k = (p = pd_indices[k], g = gt_indices[k]) (both NULL: pair k = (k, k); exactly one NULL: VSRD_E_INVALID_ARGUMENT):
 *   decode box p in float32 (box_parameters.py:124-146, the decode of vsrd_frame_labels) -> `corners`;
 *   rectify both boxes in float32, c' = Rect c as (R0 c0 + R1 c1) + R2 c2, every product and sum rounded on its own, then turn them z-up
 *     by the exact map (x, y, z) -> (x, z, -y);
 *   vsrd.operations.box_3d_iou (kitti360_operations.py:82-108) in double on those float32 numbers, with its quirks: the footprint is
 *     corners 3, 2, 1, 0; Sutherland-Hodgman with the strict inside test; crossings divide by determinant + 0.01; the intersection area is
 *     the area of the clipped polygon's convex hull, capped by the smaller footprint; volumes from three edge lengths, heights from
 *     corners 0 and 4.
 * Stated deviations: the reference turns the boxes with the float32 matrix rotation_matrix_x(-pi/2), whose cosine is -4.37e-8 and not 0
 * (the effect on the IoUs stays within a few 1e-6: tests/test_hip_frame_metrics.py); a clipped polygon with fewer than three distinct
 * points or a hull of zero area has area 0, where the reference's qhull raises.
 * Conventions as for vsrd_frame_labels: config->num_boxes is the capacity N (1..VSRD_MAX_INSTANCES) and the stride of every instance
 * axis, num_frames / frame_stride batch the call, frame_header (may be NULL: every frame has N boxes) carries the frame's own count n_f,
 * clamped to [1, N]; instances n_f .. N-1 are never read and never written.  Of config, the call reads num_boxes, the location and
 * dimension ranges and the batch fields.  A pair whose index lies outside 0 .. n_f-1 is skipped.
 *   gt_boxes_3d [N,8,3]  ground-truth corners in the frame of the decoded boxes, the reference's corner order, by ground-truth slot; a slot
 *                        with any non-finite entry has no annotation;
 *   rectification [3,3]  row-major, or NULL: the identity;
 *   corners [N,8,3]      out or NULL: the decoded corners of every box, unrectified;
 *   ious [N,2]           out: (iou_3d, iou_bev) of pair k at the PREDICTION's slot p; NaN where its ground truth has no annotation;
 *   summary [8]          out: (count, iou_3d, iou_bev, accuracy_3d_25, accuracy_bev_25, accuracy_3d_50, accuracy_bev_50, 0) over the pairs
 *                        with an annotation, summed in ascending k in double: the means, and the shares of pairs with IoU > 0.25 / > 0.5
 *                        (main.py:908-915); count == 0: eight zeros (the reference logs no metrics then).
 * NULL gt_boxes_3d, ious or summary: VSRD_E_INVALID_ARGUMENT. */
int32_t vsrd_frame_metrics(const vsrd_frame_config* config,
                           const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                           const float* gt_boxes_3d /* [N,8,3] */, const float* rectification /* [3,3] or NULL */,
                           const int64_t* pd_indices, const int64_t* gt_indices /* [N], or both NULL */,
                           float* corners /* [N,8,3] or NULL */, float* ious /* [N,2] */, float* summary /* [8] */,
                           const vsrd_frame_header* frame_header /* may be NULL */, void* stream);

/* Frame log (added within ABI 12; probe for the symbol -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field): the scalar
 * history and the step snapshots of a frame's optimisation, kept on the device -- what the reference's loop leaves behind every
 * `scalar_intervals` steps (the named losses, metrics, learning rates and annealed hyperparameters, scripts/main.py:870-953) and every
 * `ckpt_intervals` steps (step_{step}.pt, main.py:1109-1121) -- in ONE launch between two replays of the step graphs, no host
 * synchronisation, no allocation, capturable.  The call is pure gather and copy: every value is moved as the 32 bits it is (int32 sources
 * such as pixel counts included), nothing is computed from it.
 * EVERY pointer of the structure is device memory and addresses frame 0's buffer; num_frames / frame_stride batch the call as in
 * vsrd_frame_config (frame f's copy of every buffer, its pointer list and its segment table included, lies f * frame_stride bytes behind).
 * Each frame reads its own step counter `step` once -- the int64 vsrd_frame_epilogue increments: after step s it holds c = s + 1 -- and
 * decides by it alone, so frames of one call whose counters differ each log what their own counter says:
 *   history   if scalar_interval > 0, c > 0 and c % scalar_interval == 0: row c / scalar_interval - 1 of history
 *             [history_capacity, VSRD_LOG_SCALARS] = (the step c - 1 as an int32 bit pattern | record[5] | *learning_rates[0..5) |
 *             schedule[3] | summary[8], or eight quiet NaNs (0x7fc00000) when summary is NULL);
 *   snapshot  if checkpoint_interval > 0, c > 0 and c % checkpoint_interval == 0: for every entry of `segments`, `count` 32-bit words from
 *             `source` to word `offset` of slot c / checkpoint_interval - 1 of snapshots [snapshot_capacity, snapshot_floats], and
 *             snapshot_steps[slot] = c - 1.  Sources and destinations that are 16-byte aligned are copied with 16-byte accesses (lay the
 *             offsets out on multiples of four words); anything else word by word.  An entry with a NULL source, a count < 1 or a range
 *             outside the slot is skipped.
 * A row or slot at or beyond its capacity is dropped and counted.  counters [4] int32 = (rows_written, rows_dropped, slots_written,
 * slots_dropped): *_written is the highest row / slot written plus one, never lowered by the call; the caller zeroes the counters when a
 * frame starts over.  Nothing outside the written row, the written slot's segments, snapshot_steps[slot] and the counters is written.
 * What a frame with n_f < N instances in a row laid out for N copies is the caller's choice: the table is the frame's own, so its counts
 * cover the frame's n_f instances while its offsets are laid out for N -- the call reads nothing but what the entries name.
 * Both intervals 0: VSRD_OK without a launch.  Refused with VSRD_E_INVALID_ARGUMENT before any launch: a negative interval or capacity;
 * NULL step or counters; scalar_interval > 0 with NULL record, learning_rates, schedule or history; checkpoint_interval > 0 with NULL
 * segments, snapshots or snapshot_steps, num_segments outside 0..VSRD_LOG_MAX_SEGMENTS, snapshot_floats negative or no multiple of 4, or
 * snapshots not 16-byte aligned; num_frames / frame_stride as everywhere. */
#define VSRD_LOG_SCALARS 22
#define VSRD_LOG_MAX_SEGMENTS 32
typedef struct vsrd_log_segment {   /* device memory */
    const void* source;
    int64_t count;                  /* 32-bit words                                                                           */
    int64_t offset;                 /* 32-bit words from the start of a slot                                                  */
} vsrd_log_segment;

typedef struct vsrd_frame_log_config {
    int32_t scalar_interval;        /* 0: no history                                                                          */
    int32_t checkpoint_interval;    /* 0: no snapshots                                                                        */
    int32_t history_capacity;       /* rows                                                                                   */
    int32_t snapshot_capacity;      /* slots                                                                                  */
    int64_t snapshot_floats;        /* 32-bit words per slot, a multiple of 4                                                 */
    int32_t num_segments;
    int32_t num_frames;             /* 0 or 1 = one frame                                                                     */
    int64_t frame_stride;           /* bytes between the frames' copies of every buffer of the call                           */
    const int64_t* step;            /* [1]                                                                                    */
    const float* record;            /* [5] vsrd_frame_epilogue's record                                                       */
    const void* learning_rates;     /* [5] device pointers (const float*), each to a [1] rate                                 */
    const float* schedule;          /* [3]                                                                                    */
    const float* summary;           /* [8] vsrd_frame_metrics' summary, or NULL                                               */
    const vsrd_log_segment* segments;   /* [num_segments]                                                                     */
    float* history;                 /* [history_capacity, VSRD_LOG_SCALARS]                                                   */
    float* snapshots;               /* [snapshot_capacity, snapshot_floats]                                                   */
    int32_t* snapshot_steps;        /* [snapshot_capacity]                                                                    */
    int32_t* counters;              /* [4]                                                                                    */
} vsrd_frame_log_config;

int32_t vsrd_frame_log(const vsrd_frame_log_config* log, void* stream);

/* Multi-view patch-correlation photometric loss (added within ABI 12; probe for the symbols -- VSRD_ABI_VERSION is unchanged, no existing
 * struct has a new field): the homography / patch-correlation part of the reference's photometric branch (scripts/main.py:783-851) for ONE
 * frame, forward and backward, without host synchronisation or allocation, capturable.  The arithmetic is tiny (100 rays x 17 views x 121
 * pixels); what the calls buy is launch count -- three launches forward, two backward, where the reference issues V grid_sample calls, V R
 * matrix chains and a Python loop with cov / diag / sqrt / topk per converged ray -- not throughput.
 * What is computed, the reference's quirks included:
 *   patch grid   offsets arange(pw) - pw / 2 in x and arange(ph) - ph / 2 in y (integer division: size 4 gives -2..1), x the fast index,
 *                P = pw ph; q = (x + dx, y + dy, 1) for the ray's target pixel (x, y);
 *   homography   for EVERY view s, the target included: H = K_s (R_s R_t^T - R_s (R_s^T t_s - R_t^T t_t) n^T / -(n.p)) K_t^-1, evaluated as
 *                A_s + b_s (K_t^-T n)^T / (n.p) with A_s = K_s R_s R_t^T K_t^-1 and b_s = K_s R_s (R_s^T t_s - R_t^T t_t) computed once per
 *                call in double (K_t^-1 by adjugate: no assumption about the skew); h = H q, s = h_xy / (h_z + sample_epsilon);
 *   sampling     the reference maps [0, W-1] -> [-1, 1] (align-corners) and then calls grid_sample with align_corners=False: the sampled
 *                pixel coordinate is s_x W / (W - 1) - 0.5 (likewise y) -- even the identity homography interpolates.  Bilinear, zeros
 *                padding: a tap outside the image contributes 0;
 *   correlation  per converged ray the V patches [V,P]: unbiased covariance (/ (P - 1)), c_ij = cov_ij / sqrt(cov_ii cov_jj +
 *                correlation_epsilon) -- a constant patch has coefficient 0 with everything, itself included, not NaN --, the top_k largest
 *                of every row (the self-coefficient is among the candidates; NaN ranks above every number, as in torch.topk; ties go to the
 *                lowest index);
 *   loss         (1 - nanmean(all selected coefficients of all converged rays)) / 2; unconverged rays contribute nothing.
 * Two stated deviations from the reference:
 *   gray first   the reference samples the three colour planes and applies 0.2989 r + 0.587 g + 0.114 b afterwards; here
 *                vsrd_grayscale_images makes the gray planes once per frame and the loss samples those.  Both maps are linear, so the two
 *                orders agree in exact arithmetic; they differ in rounding only, and the gathers are a third;
 *   no ray       with no converged ray the reference adds no term; here the loss is 0 and every gradient 0 -- the same weighted sum.
 * Hazards: a plane that passes near a source camera's centre sends sample coordinates to +-5e8 and beyond, h_z + sample_epsilon == 0 makes
 * them non-finite.  Inside-ness is decided in floating point before any conversion to integer; a sample that is outside or non-finite reads
 * 0 and passes no gradient.
 * Deterministic: every reduction has a fixed order, there are no floating-point atomics.
 * Limits, refused with VSRD_E_INVALID_ARGUMENT before any launch: 1 <= top_k <= num_views <= VSRD_PATCH_MAX_VIEWS; 1 <= patch_width,
 * patch_height and P <= VSRD_PATCH_MAX_PIXELS; 1 <= num_rays <= VSRD_PATCH_MAX_RAYS; height, width >= 2; 0 <= target_view < num_views; a
 * NULL config or required pointer.  A workspace smaller than vsrd_patch_correlation_workspace_bytes: VSRD_E_WORKSPACE. */
#define VSRD_PATCH_MAX_VIEWS 32
#define VSRD_PATCH_MAX_PIXELS 256
#define VSRD_PATCH_MAX_RAYS 65535
typedef struct vsrd_patch_correlation_config {
    int32_t num_views;              /* V                                                                                      */
    int32_t num_rays;               /* R                                                                                      */
    int32_t height, width;          /* of every image                                                                         */
    int32_t patch_width;            /* pw: the reference's patch_size[0]                                                      */
    int32_t patch_height;           /* ph: patch_size[1]                                                                      */
    int32_t top_k;                  /* the reference: 4                                                                       */
    int32_t target_view;            /* t: the view the pixels, positions and normals belong to                                */
    float sample_epsilon;           /* the reference: 1e-6                                                                    */
    float correlation_epsilon;      /* the reference: 1e-12                                                                   */
} vsrd_patch_correlation_config;

/* images [V,3,H,W] -> gray [V,H,W] = fma(0.114, b, fma(0.587, g, 0.2989 r)) (torchvision's rgb_to_grayscale weights, the products fused as
 * written here, whatever the compiler's contraction mode).  Once per frame: the images do not change over its steps.  H W need not be a
 * multiple of 4. */
int32_t vsrd_grayscale_images(const float* images, int32_t num_views, int32_t height, int32_t width, float* gray, void* stream);

/* Bytes of the calls' workspace: the per-view constants and one (sum, count) pair per ray.  Grows with num_views and num_rays;
 * patch_pixels is validated with them (the patches themselves live in LDS) and adds nothing today.  0 for a shape outside the limits. */
size_t vsrd_patch_correlation_workspace_bytes(int32_t num_views, int32_t num_rays, int32_t patch_pixels);

/* gray [V,H,W]; intrinsics [V,3,3] and extrinsics [V,4,4] row-major, the reference's own matrices; pixels [R,2] = (x, y) of the target
 * view; positions, normals [R,3] in the frame of the extrinsics' input; converged [R].
 * Out: loss [1]; stats [2] = (sum, count) of the selected non-NaN coefficients.  Optional (NULL: not written): patches [V,R,P], the
 * reference's sampled_patches without the singleton -- of every ray, converged or not; coefficients [R,V,V] and selected [R,V] (bit j of
 * entry (r, i): coefficient (i, j) is among row i's top_k), zero rows for unconverged rays. */
int32_t vsrd_patch_correlation_forward(const vsrd_patch_correlation_config* config, const float* gray, const float* intrinsics, const float* extrinsics,
                                       const int32_t* pixels, const float* positions, const float* normals, const uint8_t* converged,
                                       void* workspace, size_t workspace_bytes, float* loss, float* stats,
                                       float* patches, float* coefficients, int32_t* selected, void* stream);

/* The same inputs, the forward's stats and the upstream gradient of the loss grad_loss [1] (device memory) -> grad_positions, grad_normals
 * [R,3]; zero rows for unconverged rays.  Every ray's forward is recomputed with the forward's own device functions (the selection is the
 * forward's bit for bit); the workspace need not be the forward's, nor keep its contents in between.  No gradient with respect to images
 * or cameras. */
int32_t vsrd_patch_correlation_backward(const vsrd_patch_correlation_config* config, const float* gray, const float* intrinsics, const float* extrinsics,
                                        const int32_t* pixels, const float* positions, const float* normals, const uint8_t* converged,
                                        void* workspace, size_t workspace_bytes, const float* stats, const float* grad_loss,
                                        float* grad_positions, float* grad_normals, void* stream);

/* Frame photometric term (added within ABI 12; probe for the symbols -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field):
 * the multi-view patch-correlation term of ONE frame's optimisation step (scripts/main.py:689-853), forward and backward, in ONE call between
 * the step's render launch and its epilogue -- no host synchronisation, no allocation, capturable.  In stream order, R = patch->num_rays rays:
 *   gather      directions[r] = ray_directions[ray_indices[r]], pixels[r] = (index % W, index / W);
 *   trace       vsrd_sphere_trace from camera_position along the directions, HARD union, initialise = 0 -> p0, converged;
 *   evaluate    vsrd_field_eval at p0 (hard) -> d0, g0;
 *   newton      p1 = converged ? p0 + r * (-d0 / (g0 . r)) : p0 (renderers.py:59-72, g0 a constant);
 *   evaluate    vsrd_field_eval at p1 (hard) -> g1;
 *   normalise   n = g1 / max(|g1|, 1e-12) (F.normalize);
 *   forward     vsrd_patch_correlation_forward(pixels, p1, n, converged) -> loss, stats;
 *   backward    vsrd_patch_correlation_backward with grad_loss = 1 -> p1_bar, n_bar;
 *   adjoints    gamma = (n_bar - n (n . n_bar)) / max(|g1|, 1e-12); vsrd_field_eval_adjoint at p1 with grad_gradients = gamma -> x_bar, G_a, M_a;
 *               d_bar = converged ? -((p1_bar + x_bar) . r) / (g0 . r) : 0; vsrd_field_eval_backward at p0 with grad_distances = d_bar -> G_b, M_b;
 *   accumulate  photometric_grad_instances [N,16] = G_a + G_b and photometric_grad_mlp [N,1617] = M_a + M_b (the term's own gradients), then
 *               grad_instances += scale * photometric_grad_instances and grad_mlp += scale * photometric_grad_mlp IN PLACE (one fused
 *               multiply-add per element) on the buffers the render step has written.  Those are in units of the silhouette term -- the
 *               epilogue and vsrd_hypernetwork_backward_step multiply them by the silhouette weight -- so scale = photometric weight /
 *               silhouette weight, as eikonal_ratio is.
 * The glue between the library's launches repeats torch's roundings operator by operator: given the same field and rays, p1, converged, n,
 * the loss and stats carry the bits of the autograd composition sphere_tracing(differentiable=True) -> surface_normal ->
 * patch_correlation_loss.  The field evaluations of this call use the exact-fp32 products of the per-instance MLP: the second-order adjoint
 * exists in that form only (the step's render launch may still use VSRD_FLAG_MLP_SPLIT_BF16).
 * No converged ray: loss 0, stats (0, 0), both photometric_grad_* all zero, grad_instances / grad_mlp keep their bits (the stated deviation of
 * vsrd_patch_correlation_forward).  Deterministic: every reduction has a fixed order, there are no floating-point atomics.
 *   field              the field as the step's render launch sees it: the row's instances and, in the residual phase, the centred MLP weights;
 *   camera_position    [3], the origin of every ray; ray_directions [H W,3], the target view's slice;
 *   gray, intrinsics, extrinsics, patch   as for vsrd_patch_correlation_forward; patch->num_rays is R;
 *   ray_indices        [R] int64, pixel indices of the target view, each in 0 .. H W - 1 (not checked: device memory);
 *   workspace          vsrd_frame_photometric_workspace_bytes(N, residual, V, R, patch pixels) bytes, 256-byte aligned;
 *   loss [1], stats [2]; photometric_grad_mlp and grad_mlp are required for residual fields and ignored otherwise;
 *   positions [R,3] = p1, normals [R,3] = n, converged [R]: optional outputs (NULL: kept in the workspace).
 * Refused with VSRD_E_INVALID_ARGUMENT before any launch: a NULL config, patch, field or required pointer; N outside 1..VSRD_MAX_INSTANCES;
 * R outside 1..VSRD_PHOTOMETRIC_MAX_RAYS (the table sampler's limit); top_k > V, V > VSRD_PATCH_MAX_VIEWS, patch pixels >
 * VSRD_PATCH_MAX_PIXELS and the other limits of vsrd_patch_correlation_forward; num_iterations < 0.  A workspace that is too small:
 * VSRD_E_WORKSPACE.  num_frames >= 2: VSRD_E_UNSUPPORTED before any launch -- a batch of frames goes through
 * vsrd_frame_photometric_with_header below. */
#define VSRD_PHOTOMETRIC_MAX_RAYS 2048
typedef struct vsrd_frame_photometric_config {
    int32_t num_iterations;         /* of the trace (config.json: surface_num_iterations)                                     */
    float convergence_criteria;
    float bounding_radius;          /* <= 0: none                                                                             */
    float scale;                    /* photometric weight / silhouette weight                                                 */
    int32_t num_frames;             /* 0 or 1 = one frame; >= 2: vsrd_frame_photometric_with_header only (here VSRD_E_UNSUPPORTED) */
    int64_t frame_stride;           /* bytes between the frames' copies of every buffer of the call                           */
} vsrd_frame_photometric_config;

/* 0 for a shape outside the limits. */
size_t vsrd_frame_photometric_workspace_bytes(int32_t num_instances, int32_t residual, int32_t num_views, int32_t num_rays, int32_t patch_pixels);

int32_t vsrd_frame_photometric(const vsrd_frame_photometric_config* config, const vsrd_patch_correlation_config* patch, const vsrd_field* field,
                               const float* camera_position, const float* ray_directions, const float* gray, const float* intrinsics,
                               const float* extrinsics, const int64_t* ray_indices, void* workspace, size_t workspace_bytes,
                               float* loss, float* stats, float* photometric_grad_instances, float* photometric_grad_mlp,
                               float* grad_instances, float* grad_mlp, float* positions, float* normals, uint8_t* converged, void* stream);

/* After vsrd_frame_epilogue: record[4] += weight * loss (the product rounded, then the sum), one single-lane launch; with no converged ray
 * (stats[1] == 0) record keeps its bits.  loss, stats: vsrd_frame_photometric's outputs; record [5]: the epilogue's. */
int32_t vsrd_frame_photometric_finish(const float* loss, const float* stats, float weight, float* record, void* stream);

/* The photometric term over a batch of frames (added within ABI 12; probe for the symbols): vsrd_frame_photometric for every frame of a
 * batch in the SAME number of launches -- every launch of the call is B copies of its one-frame grid stacked along blockIdx.y ("frame
 * batches" above), so the frames' traces run side by side instead of one after the other.  The arguments are vsrd_frame_photometric's, and
 * config->num_frames / frame_stride are honoured: every device pointer -- the arguments, the members of `field`, the workspace and the three
 * optional outputs -- addresses frame 0's buffer, frame f's lies f * frame_stride bytes behind it (a positive multiple of 256), by-value
 * arguments are shared; workspace_bytes is the size of ONE frame's workspace (vsrd_frame_photometric_workspace_bytes stays per frame).
 * frame_header (device memory, frame_stride apart like every buffer; may be NULL: every frame has field->num_instances instances and
 * patch->num_views views) makes field->num_instances the capacity and the stride of every instance axis and patch->num_views the capacity
 * of every view axis; the frame's own n_f and v_f come from its header (n_f clamped to [1, N]; v_f read when num_instances carries
 * VSRD_FRAME_HEADER_HAS_VIEWS, 0 = V, clamped to [1, V]).  Instances n_f .. N-1 and views v_f .. V-1 of every input and output are neither
 * read nor written; the patch correlation is the one over the frame's own v_f views.
 * Frame f's loss, stats, own gradients, accumulated totals, positions, normals and converged flags carry the bits of a one-frame call on
 * frame f laid out for its own n_f and v_f; a call with one frame and a NULL header issues the launches of vsrd_frame_photometric.
 * Refused before any launch: everything vsrd_frame_photometric refuses (VSRD_E_UNSUPPORTED for a batch excepted), and a malformed batch
 * (num_frames > 1024, a frame_stride that is not a positive multiple of 256): VSRD_E_INVALID_ARGUMENT.  top_k > v_f cannot be seen from
 * the host side of the call (the header is device memory): such a frame gets loss 0, stats (0, 0), zero own gradients and untouched
 * totals, exactly as a frame without a converged ray. */
int32_t vsrd_frame_photometric_with_header(const vsrd_frame_photometric_config* config, const vsrd_patch_correlation_config* patch, const vsrd_field* field,
                                           const float* camera_position, const float* ray_directions, const float* gray, const float* intrinsics,
                                           const float* extrinsics, const int64_t* ray_indices, void* workspace, size_t workspace_bytes,
                                           float* loss, float* stats, float* photometric_grad_instances, float* photometric_grad_mlp,
                                           float* grad_instances, float* grad_mlp, float* positions, float* normals, uint8_t* converged,
                                           const vsrd_frame_header* frame_header, void* stream);

/* vsrd_frame_photometric_finish for every frame of a batch in one launch (grid y is the frame): loss, stats and record address frame 0's,
 * frame f's lie f * frame_stride bytes behind; the weight is shared.  A malformed batch: VSRD_E_INVALID_ARGUMENT. */
int32_t vsrd_frame_photometric_finish_with_header(const float* loss, const float* stats, float weight, float* record, int32_t num_frames,
                                                  int64_t frame_stride, void* stream);

/* vsrd_sample_rays_table for every frame of a batch in one launch (grid y is the frame): frame f draws num_samples indices from ITS table
 * (built over `count` weights, like every frame's), keyed by (seed, ITS step counter *device_stream_offset), into ITS indices -- the
 * indices vsrd_sample_rays_table gives it alone.  table, device_stream_offset (required) and indices address frame 0's, frame f's lie
 * f * frame_stride bytes behind.  No remap.  Refusals as for vsrd_sample_rays_table, and a malformed batch: VSRD_E_INVALID_ARGUMENT. */
int32_t vsrd_sample_rays_table_frames(void* table, int64_t count, int32_t num_samples, uint64_t seed, const uint64_t* device_stream_offset,
                                      int64_t* indices, int32_t num_frames, int64_t frame_stride, void* stream);

/* Box decode (added within ABI 12; probe for the symbols -- VSRD_ABI_VERSION is unchanged, no existing struct has a new field): the forward
 * of the reference's BoxParameters3D (vsrd/models/detectors/box_parameters.py:16-146) for ONE frame and its autograd backward, one launch
 * each, without host synchronisation or allocation, capturable.  The arithmetic is tiny; what the calls buy is launch count on the
 * optimisation step's dependent chain (eager torch: ~35 element-wise launches per step).  It is torch's arithmetic op for op -- sigmoid as
 * 1 / (1 + exp(-x)), lerp in ATen's two-sided form, F.normalize with its 1e-12 clamp, the rotation about y with exact 0 and 1 entries,
 * corners (u_k * dim) R^T + loc -- and the backward chains the cotangents as torch's autograd does.
 * In: raw_locations, raw_dimensions [N,3], raw_orientations [N,2]; location_range, dimension_range [2,3] (lower | upper bounds), device memory.
 * Out: instances [N,16] = location | rotation row-major | dimensions | 0 (a vsrd_field's instances); locations, dimensions [N,3];
 * orientations [N,3,3]; boxes_3d [N,8,3].  Every pointer is required.
 * N outside 1..VSRD_MAX_INSTANCES or a NULL pointer: VSRD_E_INVALID_ARGUMENT before any launch, nothing written. */
int32_t vsrd_box_decode_forward(const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                                const float* location_range, const float* dimension_range, int32_t num_instances,
                                float* instances, float* locations, float* dimensions, float* orientations, float* boxes_3d, void* stream);

/* The same inputs and the cotangents of the five outputs -- each may be NULL: that output was not used -- -> grad_raw_locations,
 * grad_raw_dimensions [N,3], grad_raw_orientations [N,2] (required; written, not accumulated).  The forward is recomputed. */
int32_t vsrd_box_decode_backward(const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                                 const float* location_range, const float* dimension_range, int32_t num_instances,
                                 const float* grad_instances, const float* grad_locations, const float* grad_dimensions,
                                 const float* grad_orientations, const float* grad_boxes_3d,
                                 float* grad_raw_locations, float* grad_raw_dimensions, float* grad_raw_orientations, void* stream);

/* ---- the hypernetwork that generates the residual MLPs' weights (vsrd/models/fields/hyper_distance_field.py:27-55, 75-77) --------
 * embeddings [N,256] -> (VSRD_HYPER_LAYERS - 1) x [weight_norm(Linear 256 -> 256) -> LayerNorm(256, affine) -> exact GELU]
 * -> weight_norm(Linear 256 -> 1617) = mlp_weights [N,1617].  weight_norm over dim 0: W[o,:] = g[o] v[o,:] / |v[o,:]|.
 * Every tensor is given with its torch.optim.Adam(capturable=True) state: the backward entry point also takes the Adam step
 * (main.py:860-865; embeddings and hypernetwork are parameter groups 3 and 4 with their own rates) and decays the two rates.
 * With ATen this is ~130 launches of a few microseconds per step; here 6 forwards and 12 backwards. */
#define VSRD_HYPER_LAYERS 5
#define VSRD_HYPER_WIDTH 256
typedef struct vsrd_hypernetwork {
    int32_t num_instances;                                   /* N <= 64                                                       */
    int32_t num_outputs;                                     /* 1617                                                          */
    float beta1, beta2, adam_epsilon, lr_gamma;
    vsrd_adam_tensors embeddings;                            /* [N,256]                                                       */
    vsrd_adam_tensors weight_v[VSRD_HYPER_LAYERS];           /* [256,256] x 4, [1617,256]                                     */
    vsrd_adam_tensors weight_g[VSRD_HYPER_LAYERS];           /* [256] x 4, [1617]                                             */
    vsrd_adam_tensors bias[VSRD_HYPER_LAYERS];
    vsrd_adam_tensors norm_weight[VSRD_HYPER_LAYERS - 1];    /* LayerNorm gamma [256]                                         */
    vsrd_adam_tensors norm_bias[VSRD_HYPER_LAYERS - 1];
    int32_t num_frames;                                      /* frame batch (ABI 8, "frame batches" above): every frame its OWN hypernetwork, */
    int64_t frame_stride;                                    /* embeddings and Adam state, frame_stride bytes apart                           */
} vsrd_hypernetwork;

size_t vsrd_hypernetwork_workspace_bytes(int32_t num_instances);

/* mlp_weights [N,1617] (what HyperDistanceField.hypernetwork(embeddings) returns); centred [N,1617] or NULL: the same with the
 * column means of the four LayerNorm-feeding linears removed (VSRD_FLAG_MLP_WEIGHTS_CENTRED).  The workspace keeps the
 * activations for the backward call. */
int32_t vsrd_hypernetwork_forward(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                  float* mlp_weights, float* centred, void* stream);

/* grad_mlp_weights [N,1617], multiplied by grad_scale (the loss weight) on the way in.  Backward through the hypernetwork, Adam on
 * every tensor of `net` (in place, torch's update), step counters + 1, both learning rates * lr_gamma.  Deterministic. */
int32_t vsrd_hypernetwork_backward_step(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                        const float* grad_mlp_weights, float grad_scale, void* stream);

/* The two with a per-frame header (mixed batches, "frame batches" above): the forward, the weight gradients (summed over the frame's
 * n_f instances in the order of the one-frame call) and Adam on the frame's n_f embedding rows. */
int32_t vsrd_hypernetwork_forward_with_header(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                              float* mlp_weights, float* centred, const vsrd_frame_header* frame_header, void* stream);
int32_t vsrd_hypernetwork_backward_step_with_header(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                                    const float* grad_mlp_weights, float grad_scale, const vsrd_frame_header* frame_header, void* stream);

/* The centred copy of per-instance MLP weights [N,1617] that VSRD_FLAG_MLP_WEIGHTS_CENTRED announces: in the four linears that feed a
 * LayerNorm (hyper_distance_field.py:57-73) every column, bias column included, has its mean over the 16 output channels removed.
 * LayerNorm makes the field invariant to it, and the adjoints w.r.t. the centred weights are the adjoints w.r.t. the originals. */
int32_t vsrd_centre_mlp_weights(const float* mlp_weights, int32_t num_instances, float* centred, void* stream);

/* ---- self-tests of device building blocks (used by tests/, not by the product path) --------------------------------------------
 * vsrd_selftest_wave: the wave64 primitives of csrc/wave.h (sums, scans, the reduce-scatter butterflies) on one wave: in64 [64] ->
 * out [576].  vsrd_selftest_gelu: erf_gelu / erf_gelu_derivative of csrc/hypernetwork.h at n points: out[0..n) values, out[n..2n)
 * derivatives (the hypernetwork's exact GELU, hyper_distance_field.py:38-41). */
int32_t vsrd_selftest_wave(const float* in64, float* out576, void* stream);
int32_t vsrd_selftest_gelu(const float* x, int32_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRD_HIP_H */
