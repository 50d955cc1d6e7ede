// C ABI of libvsrd_hip (include/vsrd_hip.h): argument validation, launch geometry, dispatch on the
// number of 64-sample rounds.  No torch types, no allocation, and no state beyond the experiment switches below, which are read from
// the environment ONCE (first call) and frozen: no entry point calls getenv per launch.
#include "host_checks.h"
#include "aux_kernels.h"
#include "quad_step.h"
#include "matching.h"
#include "ray_sampling.h"
#include "projection.h"
#include "frame_step.h"
#include "hypernetwork.h"
#include "frame_ingest.h"
#include "frame_labels.h"
#include "frame_group_labels.h"
#include "frame_masks.h"
#include "frame_metrics.h"
#include "frame_log.h"
#include "patch_correlation.h"
#include "frame_photometric.h"
#include "launch.h"

namespace {

using namespace vsrd;
using namespace vsrd_host;       // (kMaxBlocks, kMaxFrames, Frames / frames_of, valid_field, launch_status and the image checks: shared with frame_surface.hip)

// Experiment / A-B switches of the library, all of them: read once, then constants of the process.
struct Switches {
    int grid_blocks;          // VSRD_GRID_BLOCKS=<n> (<= kMaxBlocks): cap of the render grids
    bool cap_to_residency;    // VSRD_CAP_TO_RESIDENCY=1: fit_to_residency really caps
    int split_max_rays;       // VSRD_SPLIT_MAX_RAYS: box-only step, launches of at most this many rays split every ray over two waves (0: never)
    bool no_full_shape;       // VSRD_NO_FULL_SHAPE: the step keeps the run-time-shape kernels (quad_step.h: kFull)
    int pair_max_rays;        // VSRD_PAIR_MAX_RAYS: residual step, 0 turns the pair kernel off for two-round launches
    int slots_per_item;       // VSRD_SLOTS_PER_ITEM: forced item size of the MLP adjoint (0: planned)
};
const Switches& switches() {
    static const Switches frozen = [] {
        auto number = [](const char* name, int fallback) { const char* e = getenv(name); return e ? atoi(e) : fallback; };
        Switches w;
        const int blocks = number("VSRD_GRID_BLOCKS", 0);
        w.grid_blocks = (blocks > 0 && blocks <= kMaxBlocks) ? blocks : kMaxBlocks;
        const char* cap = getenv("VSRD_CAP_TO_RESIDENCY");
        w.cap_to_residency = cap != nullptr && cap[0] == '1';
        w.split_max_rays = number("VSRD_SPLIT_MAX_RAYS", 2048);
        w.no_full_shape = getenv("VSRD_NO_FULL_SHAPE") != nullptr;
        w.pair_max_rays = number("VSRD_PAIR_MAX_RAYS", 2048);
        w.slots_per_item = number("VSRD_SLOTS_PER_ITEM", 0);
        return w;
    }();
    return frozen;
}

struct Geometry {
    int blocks;
    int threads;
    size_t lds_bytes;
};

// Pick the number of waves per workgroup so the wave-private LDS partitions fit.
bool plan(int num_rays, size_t floats_per_wave, Geometry* g) {
    const size_t per_wave = floats_per_wave * sizeof(float);
    if (per_wave > kLdsLimit) return false;
    int waves = kMaxWavesPerBlock;
    while (waves > 1 && per_wave * waves > kLdsDefault) waves >>= 1;
    g->threads = waves * kWave;
    g->lds_bytes = per_wave * waves;
    const long long want = (static_cast<long long>(num_rays) + waves - 1) / waves;
    const int cap = switches().grid_blocks;
    g->blocks = static_cast<int>(want < 1 ? 1 : (want > cap ? cap : want));
    return true;
}

// Size a persistent launch to what is actually co-resident: with a static ray -> wave assignment a grid larger than the
// residency runs in "phases", and a partially filled last phase idles most of the chip (2048 workgroups at 6 resident per CU
// = 1.33 phases cost 2).  Performance only -- correctness never depends on residency (no inter-workgroup communication).
template <typename Kernel>
void fit_to_residency(Kernel kernel, Geometry* g) {
    // Measured on C2 (r01): capping the grid at `resident` (one phase) is 5 % SLOWER than 2048 workgroups -- rays differ a lot in
    // cost (culling, early outs) and the extra workgroups act as dynamic load balancing -- so the grid is left alone unless the
    // experiment switch asks for it.
    if (!switches().cap_to_residency) return;
    static int num_cus = 0;
    if (num_cus == 0) {
        int device = 0;
        hipDeviceProp_t props;
        if (hipGetDevice(&device) == hipSuccess && hipGetDeviceProperties(&props, device) == hipSuccess) num_cus = props.multiProcessorCount;
        if (num_cus <= 0) num_cus = 256;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), g->threads, g->lds_bytes) != hipSuccess || per_cu < 1)
        return;
    if (g->blocks > per_cu * num_cus) g->blocks = per_cu * num_cus;
}

template <typename Kernel>
int opt_in_lds(Kernel kernel, size_t bytes) {
    return opt_in(kernel, bytes, debug()) ? VSRD_OK : VSRD_E_LAUNCH;
}

// one fill for every frame's copy of a scratch region (masks, counters)
bool clear_frames(void* first, size_t bytes, const Frames& frames, hipStream_t s) {
    if (frames.count == 1) return hipMemsetAsync(first, 0, bytes, s) == hipSuccess;
    return hipMemset2DAsync(first, static_cast<size_t>(frames.stride), 0, bytes, static_cast<size_t>(frames.count), s) == hipSuccess;
}

bool wants_samples(const vsrd_render_config* c) { return c->out_distances || c->out_coarse_weights || c->out_u_coarse || c->out_u_fine; }

bool valid_config(const vsrd_render_config* c, bool gather_allowed = false, bool samples_allowed = false) {
    if (c == nullptr || c->num_rays < 0 || c->num_samples < 2 || c->num_samples > VSRD_MAX_SAMPLES || !(c->sdf_std_deviation > 0.0f) ||
        (c->origin_stride != 0 && c->origin_stride != 3))
        return false;
    Frames frames;
    if (!frames_of(c->num_frames, c->frame_stride, &frames)) return false;
    if (wants_samples(c) && !samples_allowed) return false;      // only vsrd_render_silhouette_step writes its samples out
    const bool gather = c->ray_indices != nullptr || c->target_columns != nullptr;
    if (gather && !gather_allowed) return false;                 // only the fused step kernels read through an index
    if (c->ray_indices != nullptr && c->rays_per_origin < 0) return false;
    if (c->target_columns != nullptr && c->target_stride < 1) return false;
    return true;
}

FieldArgs field_args(const vsrd_field* f) {
    FieldArgs a;
    a.num_instances = f->num_instances;
    a.inv_t = 1.0f / f->temperature;
    return a;
}

RenderArgs render_args(const vsrd_render_config* c) {
    RenderArgs a;
    a.num_rays = c->num_rays;
    a.num_samples = c->num_samples;
    a.near = c->distance_near;
    a.far = c->distance_far;
    a.sh.inv_t = 0.0f;  // filled from the field
    a.sh.cull = 0.0f;   // computed in-kernel (field.h: field_bounds)
    a.sh.reach = -1.0f; // likewise
    a.sh.yaw = false;   // likewise
    a.sh.yaw_gradients = false;
    a.sh.std = c->sdf_std_deviation;
    a.sh.inv_std = 1.0f / c->sdf_std_deviation;
    a.sh.ratio = c->cosine_ratio;
    a.sh.eps = c->epsilon;
    a.sh.mlp_bits = 0u;  // set in-kernel from the flags
    a.sh.mlp_stride = kMlpWeights;   // (the two front kernels of the residual step switch to the image table under VSRD_FLAG_MLP_SPLIT_BF16)
    a.origin_stride = c->origin_stride;
    a.seed = c->seed;
    a.stream_offset = c->stream_offset;
    a.flags = c->flags;
    a.dynamic = c->device_schedule;
    a.dynamic_offset = reinterpret_cast<const unsigned long long*>(c->device_stream_offset);
    a.ray_indices = reinterpret_cast<const long long*>(c->ray_indices);
    a.rays_per_origin = c->rays_per_origin;
    a.target_columns = c->target_columns;
    a.target_stride = c->target_stride;
    a.out_distances = c->out_distances; a.out_coarse_weights = c->out_coarse_weights;
    a.out_u_coarse = c->out_u_coarse; a.out_u_fine = c->out_u_fine;
    a.frame_stride = (c->num_frames > 1) ? c->frame_stride : 0;      // (only the two fused step entry points launch batches; the others reject them)
    return a;
}

// rounds of 64 lanes needed for `points` sample points, rounded up to the instantiated {1,2,4,8}
int rounds_for(int points) {
    const int need = (points + kWave - 1) / kWave;
    if (need <= 1) return 1;
    if (need <= 2) return 2;
    if (need <= 4) return 4;
    if (need <= 8) return 8;
    return 0;
}

// The residual adjoint needs >= 17 KB of LDS per wave (residual.h: kMlpLdsFloats): at most two waves fit the 64 KB of a workgroup.
constexpr int kResidualWaves = 2;
constexpr int kMaxBlocksResidual = 512;     // residual adjoint: one wave per SIMD resident; more workgroups than CUs = load balancing (each wave owns N x 1617 partials)

// A workspace carved into regions of floats, in order.  `base` may be null (a *_workspace_bytes call): `at`, the floats taken so far, is
// then all that means anything -- so each workspace below is sized by the function that lays it out.
struct Carver {
    float* base;
    size_t at = 0;
    float* take(size_t floats) { float* p = base ? base + at : nullptr; at += floats; return p; }
};

// The workspace of the one-kernel forms (`bytes`: vsrd_workspace_bytes): the box partials of the largest grid, then -- residual fields --
// per wave of kMaxBlocksResidual x kResidualWaves the MLP
// partials, the residual jets (value + local gradient) the forward sweep leaves for the per-instance phase [round <= 4][N][64] float4 + a
// word per (round, instance) (render_kernels.h: jet_wave_float4s), and the seeds that phase leaves for the MLP adjoint
// [ray of batch][round <= 4][N][7][64].
struct OneKernelWorkspace {
    float* partials; float* mlp_partials; float4* jets; float* seeds;
    size_t bytes;
};
OneKernelWorkspace one_kernel_workspace(void* workspace, int num_instances, bool residual) {
    Carver c{static_cast<float*>(workspace)};
    const size_t waves = residual ? static_cast<size_t>(kMaxBlocksResidual) * kResidualWaves : 0;
    OneKernelWorkspace w;
    w.partials = c.take(static_cast<size_t>(kMaxBlocks) * kMaxWavesPerBlock * num_instances * kGradStride);
    w.mlp_partials = c.take(waves * num_instances * kMlpWeights);
    w.jets = reinterpret_cast<float4*>(c.take(waves * jet_wave_float4s(4, num_instances) * 4));
    w.seeds = c.take(waves * kMlpBatch * 4 * num_instances * kSeedFloats * kWave);
    w.bytes = c.at * sizeof(float);
    return w;
}

// The multi-ray ("rows") mappings of quad_step.h, box-only fields: four neighbouring rays per wave, 16 lanes each (quad: N <= 16,
// S <= 64), or two, 32 lanes each (pair: N <= 64, S <= 128: BASELINE config 5).  A launch that fills its shape (S = 4 x lanes, more than half
// of the shape's instance slots: BASELINE configs 2 and 5) runs the hot kernel instantiated for that S with the instance tables padded
// to the shape's count (quad_step.h: kFull).
struct RowsPlan {
    bool rows;                  // one of the two mappings takes the launch
    bool quad, full;            // (pair: rows && !quad)
    int lanes, rays_per_wave, shape_instances;
    int rounds;                 // rounds of `lanes` samples of a pass, rounded up to the instantiated {1, 2, 4} (pair: {2, 4}); only the silhouette step is instantiated by it
    size_t lds_floats;          // per wave
    size_t num_groups;          // groups of rays_per_wave rays, one per wave and turn
    size_t flag_bytes;          // behind the waves' partial rows: two summary words + one byte per group, "the hot kernel could not serve this group"
};
// num_distances: a ray's merged samples, 2 S (vsrd_render_backward is handed that number, and it may be odd: only 8 x lanes is `full`)
RowsPlan plan_rows(int num_instances, int num_distances, int num_rays, uint32_t flags, bool allowed) {
    RowsPlan r = {};
    r.rows = allowed && !(flags & VSRD_FLAG_STEP_WAVE_PER_RAY) && num_instances <= kPairMaxInstances && num_distances <= 2 * kPairMaxSamples;
    if (!r.rows) return r;
    const int S = (num_distances + 1) / 2;
    r.quad = num_instances <= kQuadMaxInstances && num_distances <= 2 * kQuadMaxSamples;
    r.lanes = r.quad ? kRowLanes : 32;
    r.rays_per_wave = kWave / r.lanes;
    r.shape_instances = r.quad ? kQuadMaxInstances : kPairMaxInstances;
    r.full = num_distances == 8 * r.lanes && 2 * num_instances > r.shape_instances && !switches().no_full_shape;
    r.rounds = (r.quad && S <= r.lanes) ? 1 : (S <= 2 * r.lanes ? 2 : 4);
    r.lds_floats = static_cast<size_t>(quad_lds_floats(S, r.full ? r.shape_instances : num_instances, r.lanes));
    r.num_groups = (static_cast<size_t>(num_rays) + r.rays_per_wave - 1) / r.rays_per_wave;
    r.flag_bytes = 16 + ((r.num_groups + 15) & ~static_cast<size_t>(15));
    return r;
}

// The partial buffer holds one row of `width` floats per wave (a gradient row; + 1: the wave's loss partial, in the tail of the same
// budget) and behind the rows `flag_bytes` (RowsPlan): cap the grid to what `bytes` hold.  False: not even one workgroup's rows fit.
bool cap_to_workspace(size_t bytes, int width, size_t flag_bytes, Geometry* g) {
    const int waves_per_block = g->threads / kWave;
    if (flag_bytes + static_cast<size_t>(waves_per_block) * width * sizeof(float) > bytes) return false;
    const int max_waves = static_cast<int>((bytes - flag_bytes) / sizeof(float) / width);
    if (g->blocks * waves_per_block > max_waves) g->blocks = max_waves / waves_per_block;
    return true;
}

// The reduction behind a rows launch: reduce_partials_kernel, led by reduce_partials_residues_kernel (render_kernels.h: coalesced reads,
// the same additions in the same order) whenever the tail of the workspace holds the 256 x (row + row2) residues behind the waves' rows
// and the flags' two summary words.  The groups' flag bytes may lie there: both kernels that read them have run by then.  (A launch
// whose rows and flags fill the buffer and whose flags are fewer than the residues -- N = 16: 64 k to 263 k groups -- keeps the one kernel.)
void launch_reduce_rows(const float* partials, int num_waves, int row, float* out, const float* partials2, int row2, float* out2, void* workspace,
                        size_t bytes, hipStream_t s) {
    const size_t rows_end = (static_cast<size_t>(num_waves) * (row + row2) * sizeof(float) + 16 + 15) & ~static_cast<size_t>(15);
    const size_t residue_bytes = (static_cast<size_t>(kReduceResidues) * (row + row2) * sizeof(float) + 15) & ~static_cast<size_t>(15);
    if (rows_end + residue_bytes > bytes) {
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(row + row2), dim3(256), 0, s, partials, num_waves, row, out, nullptr, partials2, row2, out2);
        return;
    }
    float* residues = reinterpret_cast<float*>(static_cast<char*>(workspace) + ((bytes - residue_bytes) & ~static_cast<size_t>(15)));
    float* residues2 = residues + static_cast<size_t>(kReduceResidues) * row;
    hipLaunchKernelGGL(reduce_partials_residues_kernel, dim3(kReduceResidues, (row + 255) / 256 + (row2 > 0 ? 1 : 0)), dim3(256), 0, s, partials, num_waves, row,
                       partials2, row2, residues, residues2);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(row + row2), dim3(256), 0, s, residues, kReduceResidues, row, out, nullptr, row2 > 0 ? residues2 : nullptr, row2, out2);
}

// two kernels on one grid (quad_step.h): the hot body (rotations about y, fixed soft-min shift), then everything it left over
template <typename Kernel, typename... Args>
void launch_hot_then_rest(Kernel hot, Kernel rest, const Geometry& g, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(hot, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, args...);
    hipLaunchKernelGGL(rest, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, args...);
}

// ---- the split form of the residual step and of vsrd_render_backward on residual fields (render_kernels.h: a front kernel +
// residual_mlp_adjoint_kernel), the default --------------------------------------------------------------------------------------
constexpr size_t kSeedBudgetBytes = size_t(6) << 30;     // seeds of one chunk of rays: N x chunk x rounds x 1792 B (a launch is cut into chunks that fit)
constexpr int kFrontBlocks = 512;                        // x 4 waves = two waves on each of the 1024 SIMDs
constexpr int kMlpAdjointBlocks = 4096;                  // single-wave workgroups, dynamic item fetch (two per SIMD are resident)
constexpr int kPairBlocks = 1024;                        // residual_step_pair_kernel: x 2 waves = two waves on each of the 1024 SIMDs

struct ResidualStepPlan {
    int rounds, chunk, front_blocks, front_waves, slots_per_item, items_per_instance;
    bool pair;                     // few rays: residual_step_pair_kernel (a ray split over the two waves of a workgroup)
    long long slots_per_instance;
    size_t front_lds;
    // workspace layout, in floats from the base
    size_t box_partials, loss_partials, jets, box_extra, counter, segment_sums, seeds, item_rows, masks, item_flags, images, total_bytes;
};

// a chunk's front grid (one wave per ray) and its slots; returns the item size that balances it, before the caller's clamps: enough
// items to balance ~2000 waves, few enough that an item amortises its partial row (6.6 KB written and read once)
long long size_chunk(ResidualStepPlan* p, long long chunk, int N) {
    p->chunk = static_cast<int>(chunk);
    const long long want = (chunk + kMaxWavesPerBlock - 1) / kMaxWavesPerBlock;
    p->front_blocks = static_cast<int>(want > kFrontBlocks ? kFrontBlocks : want);
    p->front_waves = p->front_blocks * kMaxWavesPerBlock;
    p->slots_per_instance = chunk * p->rounds;
    return (p->slots_per_instance * N) / 16384;
}

// The regions of the workspace, from the plan's front_waves, rounds, slots and items.  loss_floats: the front waves' loss partials.
void lay_out(ResidualStepPlan* p, int N, long long per_item, size_t loss_floats, bool with_images) {
    p->slots_per_item = static_cast<int>(per_item);
    p->items_per_instance = static_cast<int>((p->slots_per_instance + per_item - 1) / per_item);
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t here = at; at += (floats + 3) & ~size_t(3); return here; };
    p->box_partials = take(static_cast<size_t>(p->front_waves) * N * kGradStride);
    p->loss_partials = take(loss_floats);
    p->jets = take(static_cast<size_t>(p->front_waves) * jet_wave_float4s(p->rounds, N) * 4);
    p->box_extra = take(static_cast<size_t>(N) * kGradStride);
    p->segment_sums = take(static_cast<size_t>(N) * kItemSegments * kItemRowFloats);
    p->seeds = take(static_cast<size_t>(N) * p->slots_per_instance * kSeedFloats * kWave);
    p->item_rows = take(static_cast<size_t>(N) * p->items_per_instance * kItemRowFloats);
    p->masks = take((static_cast<size_t>(N) * p->slots_per_instance + 3) / 4);
    p->counter = take(4);                                // right behind the masks: one memset clears both
    p->item_flags = take((static_cast<size_t>(N) * p->items_per_instance + 3) / 4);
    p->images = with_images ? take(static_cast<size_t>(N) * kMlpImageWords) : at;       // VSRD_FLAG_MLP_SPLIT_BF16: the instances' operand images (residual.h)
    p->total_bytes = at * sizeof(float);
}

bool plan_residual_step(int N, int S, int num_rays, bool allow_pair, ResidualStepPlan* p, int slots_per_item = 0) {
    p->rounds = rounds_for(2 * S - 1);
    if (p->rounds < 1 || p->rounds > 4) return false;
    // four rounds (S in (64, 128]): the one-wave-per-ray kernel needs 308 registers (one wave per SIMD), the pair kernel 256 -- the pair
    // kernel wins at every launch size (132 k rays, S = 100: 90.3 against 97.9 ms); two rounds: only while a launch cannot fill the SIMDs
    // (VSRD_PAIR_MAX_RAYS = 0 turns the pair kernel off for them)
    p->pair = allow_pair && num_rays >= 1 && (p->rounds == 4 || (p->rounds == 2 && num_rays <= switches().pair_max_rays));
    p->front_lds = p->pair ? static_cast<size_t>(residual_pair_lds_floats(S, N)) * sizeof(float)
                           : static_cast<size_t>(residual_front_lds_floats(S, N)) * sizeof(float) * kMaxWavesPerBlock;
    if (p->front_lds > kLdsLimit / 2) return false;     // two workgroups per CU = two waves per SIMD (one wave per ray at N = 64, S = 128: 93 KB -> the single-kernel form)
    const size_t per_ray = static_cast<size_t>(N) * p->rounds * kSeedFloats * kWave * sizeof(float);
    long long chunk = static_cast<long long>(kSeedBudgetBytes / per_ray);
    if (chunk < 256) chunk = 256;
    if (chunk > num_rays) chunk = num_rays < 1 ? 1 : num_rays;
    long long per_item = size_chunk(p, chunk, N);
    if (p->pair) {
        p->front_blocks = static_cast<int>(chunk > kPairBlocks ? kPairBlocks : chunk);
        p->front_waves = p->front_blocks * kPairWaves;
    }
    // (round 6: launches that leave >= 32 k items even at the largest item -- config 3's chunks of 110 k rays -- take 64 slots per item: same
    //  speed as 32 or 48 (3.66-3.70 Mrays/s, tools/gpu_r06q.sh), half the partial rows written and reduced: 35 -> 17 GB per config-3 step)
    per_item = per_item < 4 ? 4 : (per_item >= 128 ? 64 : (per_item > 32 ? 32 : per_item));
    const int forced = switches().slots_per_item;                        // experiment switch
    if (forced >= 1 && forced <= 64) per_item = forced;
    if (slots_per_item >= 1 && slots_per_item <= 64) per_item = slots_per_item;      // vsrd_render_config::adjoint_slots_per_item
    lay_out(p, N, per_item, static_cast<size_t>(p->front_waves) * 2, true);
    return true;
}

// vsrd_render_backward on residual fields in the split form.  The plan is the residual step's, with the chunk of rays sized to what the
// caller's workspace holds (at least min(num_rays, 64) rays, else the caller falls back to render_backward_kernel<K, true>).
bool plan_backward_split(int N, int num_distances, int num_rays, size_t budget_bytes, ResidualStepPlan* p) {
    p->rounds = rounds_for(num_distances - 1);
    if (p->rounds < 1 || p->rounds > 4) return false;
    p->pair = false;
    p->front_lds = static_cast<size_t>(backward_front_lds_floats(num_distances, N)) * sizeof(float) * kMaxWavesPerBlock;
    if (p->front_lds > kLdsDefault) return false;
    const size_t per_ray = static_cast<size_t>(N) * p->rounds * kSeedFloats * kWave * sizeof(float);
    long long chunk = static_cast<long long>(kSeedBudgetBytes / per_ray);
    if (chunk > num_rays) chunk = num_rays < 1 ? 1 : num_rays;
    for (;; chunk = chunk * 3 / 4) {                                       // the largest chunk whose whole layout fits the budget
        if (chunk < (num_rays < 64 ? num_rays : 64)) return false;
        const long long per_item = size_chunk(p, chunk, N);
        lay_out(p, N, per_item < 4 ? 4 : (per_item > 32 ? 32 : per_item), 4, false);
        if (p->total_bytes <= budget_bytes) return true;
        if (chunk <= 1) return false;
    }
}

// the regions of a planned workspace as pointers
struct SplitWorkspace {
    float* box_partials; float* loss_partials; float4* jets; float* box_extra; unsigned* counter; float* segment_sums; float* seeds; float* item_rows;
    unsigned char* masks; unsigned char* item_flags; unsigned* images;
    size_t clear_bytes;         // tile masks + the item counter's 16-byte slot (a multiple of 16 bytes: one fill kernel, not two)
};
SplitWorkspace split_workspace(void* workspace, const ResidualStepPlan& p) {
    float* base = static_cast<float*>(workspace);
    SplitWorkspace w;
    w.box_partials = base + p.box_partials;
    w.loss_partials = base + p.loss_partials;
    w.jets = reinterpret_cast<float4*>(base + p.jets);
    w.box_extra = base + p.box_extra;
    w.counter = reinterpret_cast<unsigned*>(base + p.counter);
    w.segment_sums = base + p.segment_sums;
    w.seeds = base + p.seeds;
    w.item_rows = base + p.item_rows;
    w.masks = reinterpret_cast<unsigned char*>(base + p.masks);
    w.item_flags = reinterpret_cast<unsigned char*>(base + p.item_flags);
    w.images = reinterpret_cast<unsigned*>(base + p.images);
    w.clear_bytes = (p.counter - p.masks + 4) * sizeof(float);
    return w;
}

// A chunk's tail, behind its front kernel: the MLP adjoint by instance over the chunk's seeds (images: its split-bf16 form, which reads
// the operand images the front kernel read), then the two deterministic reductions of its item rows into grad_mlp_weights and box_extra.
int32_t launch_adjoint_tail(const vsrd_field* field, const unsigned* images, uint32_t flags, const ResidualStepPlan& p, const SplitWorkspace& w, int rays,
                            bool accumulate, float* grad_mlp_weights, const Frames& frames, const FrameHeader* header, hipStream_t s) {
    const int N = field->num_instances;
    const long long used_slots = static_cast<long long>(rays) * p.rounds;
    if (images != nullptr) {
        if (vsrd_split_front::launch_adjoint(kMlpAdjointBlocks, field->instances, reinterpret_cast<const float*>(images), N, w.seeds, w.masks, p.slots_per_instance,
                                             used_slots, p.items_per_instance, p.slots_per_item, w.counter, w.item_rows, w.item_flags, frames.count, frames.stride, s) !=
            vsrd_split_front::kOk)
            return VSRD_E_LAUNCH;
    } else {
        const unsigned mlp_bits = (flags & VSRD_FLAG_MLP_WEIGHTS_CENTRED) ? kMlpCentredBit : 0u;
        const size_t adjoint_lds = (static_cast<size_t>(kMlpWbarFloats) + static_cast<size_t>(kMlpStashTiles) * kTileFloats) * sizeof(float);
        hipLaunchKernelGGL(residual_mlp_adjoint_kernel, dim3(kMlpAdjointBlocks, frames.count), dim3(kWave), adjoint_lds, s, field->instances, field->mlp_weights, N,
                           mlp_bits, w.seeds, w.masks, p.slots_per_instance, used_slots, p.items_per_instance, p.slots_per_item, w.counter, w.item_rows, w.item_flags,
                           frames.stride);
    }
    hipLaunchKernelGGL(reduce_item_rows_kernel, dim3(N, (kItemRowFloats + 255) / 256, kItemSegments * frames.count), dim3(256), 0, s, w.item_rows, w.item_flags,
                       p.items_per_instance, w.segment_sums, frames.stride, header);
    hipLaunchKernelGGL(reduce_item_segments_kernel, dim3(N, (kItemRowFloats + 255) / 256, frames.count), dim3(256), 0, s, w.segment_sums, grad_mlp_weights, w.box_extra,
                       accumulate ? 1 : 0, frames.stride, header);
    return launch_status();
}

int32_t render_backward_split(const vsrd_field* field, const vsrd_render_config* config, const float* origins, const float* directions,
                              const float* distances, int32_t num_distances, const float* grad_labels, const float* grad_gradients,
                              const float* grad_weights, void* workspace, size_t workspace_bytes, float* grad_instances, float* grad_mlp_weights,
                              void* stream, bool* taken) {
    const int N = field->num_instances;
    ResidualStepPlan p;
    *taken = plan_backward_split(N, num_distances, config->num_rays, workspace_bytes, &p);
    if (!*taken) return VSRD_OK;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int row = N * kGradStride;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    const SplitWorkspace w = split_workspace(workspace, p);
    const Frames one_frame = {1, 0};
    int chunk_index = 0;
    for (int first = 0; first < config->num_rays; first += p.chunk, ++chunk_index) {
        const int rays = std::min(p.chunk, config->num_rays - first);
        if (hipMemsetAsync(w.masks, 0, w.clear_bytes, s) != hipSuccess) return VSRD_E_LAUNCH;
        const bool known = for_rounds<1, 2, 4>(p.rounds, [&](auto k) {
            hipLaunchKernelGGL(render_backward_front_kernel<decltype(k)::value>, dim3(p.front_blocks), dim3(kBlockThreads), p.front_lds, s, f, field->instances,
                               field->mlp_weights, c, origins, directions, distances, num_distances, grad_labels, grad_gradients, grad_weights, w.box_partials, w.jets,
                               w.seeds, w.masks, p.slots_per_instance, first, rays, chunk_index > 0 ? 1 : 0);
        });
        if (!known) return VSRD_E_UNSUPPORTED;
        const int32_t status = launch_adjoint_tail(field, nullptr, config->flags, p, w, rays, chunk_index > 0, grad_mlp_weights, one_frame, nullptr, s);
        if (status != VSRD_OK) return status;
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(row), dim3(256), 0, s, w.box_partials, p.front_waves, row, grad_instances, w.box_extra);
    return launch_status();
}

// vsrd_field_eval_backward (grad_gradients = nullptr) and vsrd_field_eval_adjoint: one set of refusals, one launch geometry, one workspace
// layout; the normal's cotangent selects field_eval_backward_kernel<residual, true>, its absence the kernel of before.
int32_t field_eval_adjoint(const vsrd_field* field, const float* positions, int64_t num_points,
                           const float* grad_distances, const float* grad_labels, const float* grad_gradients, int32_t hard_union,
                           void* workspace, size_t workspace_bytes, float* grad_positions,
                           float* grad_instances, float* grad_mlp_weights, void* stream, const Frames& frames = {1, 0},
                           const FrameHeader* header = nullptr) {
    if (!valid_field(field) || !grad_instances || num_points < 0 || (!positions && num_points > 0)) return VSRD_E_INVALID_ARGUMENT;
    if (hard_union && grad_labels) return VSRD_E_INVALID_ARGUMENT;
    const bool residual = field->mlp_weights != nullptr;
    if (residual && !grad_mlp_weights) return VSRD_E_INVALID_ARGUMENT;
    const int N = field->num_instances;
    if (!workspace || workspace_bytes < vsrd_workspace_bytes(N, residual)) return VSRD_E_WORKSPACE;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int row = N * kGradStride, mlp_row = N * kMlpWeights;
    const bool batched = frames.stride != 0 || header != nullptr;     // the kFrames kernels (aux_kernels.h); the callers hand a batch points
    if (num_points == 0) {
        if (batched) return VSRD_E_UNSUPPORTED;
        if (residual && hipMemsetAsync(grad_mlp_weights, 0, mlp_row * sizeof(float), s) != hipSuccess) return VSRD_E_LAUNCH;
        return hipMemsetAsync(grad_instances, 0, row * sizeof(float), s) == hipSuccess ? VSRD_OK : VSRD_E_LAUNCH;
    }
    Geometry g;
    const size_t per_wave = (static_cast<size_t>(residual ? kMlpLdsFloats : 0) + row + 3) & ~static_cast<size_t>(3);
    if (!plan(static_cast<int>(std::min<int64_t>((num_points + kWave - 1) / kWave, 1 << 30)), per_wave, &g)) return VSRD_E_UNSUPPORTED;
    if (residual && g.threads > kResidualWaves * kWave) return VSRD_E_UNSUPPORTED;
    g.blocks = std::min(g.blocks, residual ? kMaxBlocksResidual : 2048);
    const OneKernelWorkspace w = one_kernel_workspace(workspace, N, residual);
    const FieldArgs f = field_args(field);
    for_bool(residual, [&](auto res) {
        constexpr bool kRes = decltype(res)::value;
        for_bool(grad_gradients != nullptr, [&](auto gamma) {
            constexpr bool kGamma = decltype(gamma)::value;
            if (batched)
                hipLaunchKernelGGL((field_eval_backward_kernel<kRes, kGamma, true>), dim3(g.blocks, frames.count), dim3(g.threads), g.lds_bytes, s, f,
                                   field->instances, field->mlp_weights, positions, static_cast<long long>(num_points), grad_distances, grad_labels, hard_union,
                                   grad_positions, w.partials, w.mlp_partials, grad_gradients, frames.stride, header);
            else
                hipLaunchKernelGGL((field_eval_backward_kernel<kRes, kGamma>), dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, f, field->instances,
                                   field->mlp_weights, positions, static_cast<long long>(num_points), grad_distances, grad_labels, hard_union, grad_positions,
                                   w.partials, w.mlp_partials, grad_gradients);
        });
    });
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    const int num_waves = g.blocks * (g.threads / kWave);
    // (a batch: the partial rows are the capacity's, rows n_f .. N-1 zeros.  The instance sums stop at the frame's own n_f -- the kernel's
    //  header rule is the [capacity][kGradStride] layout's; the MLP sums cover the capacity and land in a buffer of that size, of which the
    //  caller reads the leading n_f blocks)
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(row, frames.count), dim3(256), 0, s, w.partials, num_waves, row, grad_instances, nullptr, nullptr, 0, nullptr,
                       frames.stride, header);
    if (residual)
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(mlp_row, frames.count), dim3(256), 0, s, w.mlp_partials, num_waves, mlp_row, grad_mlp_weights, nullptr,
                           nullptr, 0, nullptr, frames.stride, nullptr);
    return launch_status();
}

// vsrd_field_eval and vsrd_sphere_trace behind their checks, over a batch of frames (aux_kernels.h: the kFrames kernels) or, with one frame
// and no header, as the launches of before.
int32_t launch_field_eval(const vsrd_field* field, const float* positions, int64_t num_points, float* distances, float* gradients, float* labels,
                          int32_t hard_union, const Frames& frames, const FrameHeader* header, hipStream_t s) {
    const int blocks = static_cast<int>(std::min<int64_t>((num_points + 255) / 256, 8192));
    const bool batched = frames.stride != 0 || header != nullptr;
    for_bool(field->mlp_weights != nullptr, [&](auto residual) {
        constexpr bool kRes = decltype(residual)::value;
        if (batched)
            hipLaunchKernelGGL((field_eval_kernel<kRes, true>), dim3(blocks, frames.count), dim3(256), 0, s, field_args(field), field->instances, field->mlp_weights,
                               positions, static_cast<long long>(num_points), distances, gradients, labels, hard_union, frames.stride, header);
        else
            hipLaunchKernelGGL(field_eval_kernel<kRes>, dim3(blocks), dim3(256), 0, s, field_args(field), field->instances, field->mlp_weights, positions,
                               static_cast<long long>(num_points), distances, gradients, labels, hard_union);
    });
    return launch_status();
}

int32_t launch_sphere_trace(const vsrd_field* field, const float* origins, int32_t origin_stride, const float* directions, const uint8_t* foreground,
                            int64_t num_rays, int32_t num_iterations, float convergence_criteria, float bounding_radius, int32_t initialise,
                            int32_t hard_union, float* positions, uint8_t* converged, const Frames& frames, const FrameHeader* header, hipStream_t s) {
    const int blocks = static_cast<int>(std::min<int64_t>((num_rays + 255) / 256, 16384));
    const bool batched = frames.stride != 0 || header != nullptr;
    for_bool(field->mlp_weights != nullptr, [&](auto residual) {
        constexpr bool kRes = decltype(residual)::value;
        if (batched)
            hipLaunchKernelGGL((sphere_trace_kernel<kRes, true>), dim3(blocks, frames.count), dim3(256), 0, s, field_args(field), field->instances,
                               field->mlp_weights, origins, origin_stride, directions, foreground, static_cast<long long>(num_rays), num_iterations,
                               convergence_criteria, bounding_radius, initialise, hard_union, positions, converged, frames.stride, header);
        else
            hipLaunchKernelGGL(sphere_trace_kernel<kRes>, dim3(blocks), dim3(256), 0, s, field_args(field), field->instances, field->mlp_weights, origins,
                               origin_stride, directions, foreground, static_cast<long long>(num_rays), num_iterations, convergence_criteria, bounding_radius,
                               initialise, hard_union, positions, converged);
    });
    return launch_status();
}

}  // namespace

extern "C" {

static_assert(sizeof(vsrd_frame_header) == sizeof(FrameHeader) && offsetof(vsrd_frame_header, num_views) == offsetof(FrameHeader, num_views) &&
                  offsetof(vsrd_frame_header, num_pixels) == offsetof(FrameHeader, num_pixels) && VSRD_FRAME_HEADER_HAS_VIEWS == kFrameHeaderHasViews,
              "wave.h: FrameHeader is vsrd_frame_header");
int32_t vsrd_abi_version(void) { return VSRD_ABI_VERSION; }

const char* vsrd_error_string(int32_t code) {
    switch (code) {
        case VSRD_OK: return "ok";
        case VSRD_E_INVALID_ARGUMENT: return "invalid argument";
        case VSRD_E_UNSUPPORTED: return "unsupported configuration";
        case VSRD_E_LAUNCH: return "HIP launch failed";
        case VSRD_E_WORKSPACE: return "workspace too small";
        default: return "unknown error";
    }
}

size_t vsrd_workspace_bytes(int32_t num_instances, int32_t residual) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES) return 0;
    return one_kernel_workspace(nullptr, num_instances, residual != 0).bytes;
}

int32_t vsrd_ray_directions(const float* inverse_projection, int32_t num_views, int32_t height, int32_t width,
                            float* directions, void* stream) {
    if (!inverse_projection || !directions || num_views < 1 || height < 1 || width < 1) return VSRD_E_INVALID_ARGUMENT;
    const size_t total = static_cast<size_t>(num_views) * height * width;
    const int blocks = static_cast<int>(std::min<size_t>((total + 255) / 256, 8192));
    hipLaunchKernelGGL(ray_directions_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       inverse_projection, num_views, height, width, directions);
    return launch_status();
}

int32_t vsrd_field_eval(const vsrd_field* field, const float* positions, int64_t num_points,
                        float* distances, float* gradients, float* labels, int32_t hard_union, void* stream) {
    if (!valid_field(field) || (!positions && num_points > 0) || num_points < 0) return VSRD_E_INVALID_ARGUMENT;
    if (hard_union && labels) return VSRD_E_INVALID_ARGUMENT;
    if (num_points == 0) return VSRD_OK;
    return launch_field_eval(field, positions, num_points, distances, gradients, labels, hard_union, {1, 0}, nullptr, static_cast<hipStream_t>(stream));
}

int32_t vsrd_field_eval_backward(const vsrd_field* field, const float* positions, int64_t num_points,
                                 const float* grad_distances, const float* grad_labels, int32_t hard_union,
                                 void* workspace, size_t workspace_bytes, float* grad_positions,
                                 float* grad_instances, float* grad_mlp_weights, void* stream) {
    return field_eval_adjoint(field, positions, num_points, grad_distances, grad_labels, nullptr, hard_union, workspace, workspace_bytes,
                              grad_positions, grad_instances, grad_mlp_weights, stream);
}

int32_t vsrd_field_eval_adjoint(const vsrd_field* field, const float* positions, int64_t num_points,
                                const float* grad_distances, const float* grad_labels, const float* grad_gradients,
                                int32_t hard_union, void* workspace, size_t workspace_bytes,
                                float* grad_positions, float* grad_instances, float* grad_mlp_weights, void* stream) {
    if (!grad_distances && !grad_labels && !grad_gradients) return VSRD_E_INVALID_ARGUMENT;
    return field_eval_adjoint(field, positions, num_points, grad_distances, grad_labels, grad_gradients, hard_union, workspace, workspace_bytes,
                              grad_positions, grad_instances, grad_mlp_weights, stream);
}

int32_t vsrd_sphere_trace(const vsrd_field* field, const float* origins, int32_t origin_stride, const float* directions,
                          const uint8_t* foreground, int64_t num_rays, int32_t num_iterations, float convergence_criteria,
                          float bounding_radius, int32_t initialise, int32_t hard_union,
                          float* positions, uint8_t* converged, void* stream) {
    if (!valid_field(field) || num_rays < 0 || num_iterations < 0 || (origin_stride != 0 && origin_stride != 3)) return VSRD_E_INVALID_ARGUMENT;
    if (num_rays == 0) return VSRD_OK;
    if (!origins || !directions || !positions || !converged) return VSRD_E_INVALID_ARGUMENT;
    return launch_sphere_trace(field, origins, origin_stride, directions, foreground, num_rays, num_iterations, convergence_criteria, bounding_radius,
                               initialise, hard_union, positions, converged, {1, 0}, nullptr, static_cast<hipStream_t>(stream));
}

int32_t vsrd_polygon_soft_masks(const float* polygons, const int32_t* counts, int32_t num_polygons, int32_t max_vertices,
                                int32_t height, int32_t width, const uint8_t* inside, float temperature,
                                float* distance_maps, float* soft_masks, void* stream) {
    if (num_polygons < 0 || max_vertices < 1 || height < 1 || width < 1 || temperature <= 0.0f) return VSRD_E_INVALID_ARGUMENT;
    if (num_polygons == 0) return VSRD_OK;
    if (!polygons || !counts || (!distance_maps && !soft_masks) || (soft_masks && !inside)) return VSRD_E_INVALID_ARGUMENT;
    const int pixels = height * width;
    const dim3 grid(static_cast<unsigned>(std::min((pixels + 255) / 256, 4096)), static_cast<unsigned>(num_polygons));
    hipLaunchKernelGGL(polygon_soft_mask_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), polygons, counts, num_polygons,
                       max_vertices, height, width, inside, temperature, distance_maps, soft_masks);
    return launch_status();
}

int32_t vsrd_frame_ingest_chunk(void) { return kIngestChunk; }

int32_t vsrd_frame_ingest(const int32_t* polygon_vertices, int32_t num_vertices, const int32_t* polygon_offsets, int32_t num_entries,
                          int32_t* entry_table, const uint8_t* inside, int32_t height, int32_t width, int32_t num_views, int32_t num_instances,
                          int32_t target_stride, float temperature, float* soft_masks, float* sampling_weights, float* gt_boxes,
                          uint8_t* visible, void* stream) {
    if (!polygon_vertices || !polygon_offsets || !entry_table || !inside || num_vertices < 1 || num_entries < 1) return VSRD_E_INVALID_ARGUMENT;
    if (height < 1 || width < 1 || num_views < 1 || num_views > kFrameMaxViews || num_instances < 1 || num_instances > VSRD_MAX_INSTANCES ||
        target_stride < num_instances || !(temperature > 0.0f))
        return VSRD_E_INVALID_ARGUMENT;
    const int64_t pixels = static_cast<int64_t>(height) * width;
    if (pixels * num_views * target_stride >= (int64_t{1} << 40) || pixels >= (int64_t{1} << 30)) return VSRD_E_UNSUPPORTED;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // the boxes first: they take the entries without a set bit out of the table the pixel pass reads
    hipLaunchKernelGGL(frame_ingest_boxes_kernel, dim3(num_instances, num_views), dim3(kIngestThreads), 0, s, entry_table, polygon_offsets, num_entries,
                       num_vertices, inside, height, width, num_instances, target_stride, gt_boxes, visible);
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    if (!soft_masks && !sampling_weights) return VSRD_OK;
    const int per_block = kIngestThreads * kIngestPixels;
    const dim3 grid(static_cast<unsigned>((pixels + per_block - 1) / per_block), static_cast<unsigned>(num_views));
    const bool vector = target_stride % 4 == 0 && reinterpret_cast<uintptr_t>(soft_masks) % 16 == 0;
    for_bool(vector, [&](auto wide) {
        hipLaunchKernelGGL(frame_ingest_pixels_kernel<decltype(wide)::value>, grid, dim3(kIngestThreads), 0, s, entry_table, polygon_offsets, polygon_vertices,
                           inside, height, width, num_instances, target_stride, temperature, soft_masks, sampling_weights);
    });
    return launch_status();
}

int32_t vsrd_sample_stratified(const vsrd_render_config* config, const float* u_coarse, float* distances, void* stream) {
    if (config != nullptr && config->num_frames > 1) return VSRD_E_UNSUPPORTED;      // (frame batches: the per-frame step entry points only)
    if (!valid_config(config)) return VSRD_E_INVALID_ARGUMENT;
    if (config->num_rays == 0) return VSRD_OK;
    if (!u_coarse || !distances) return VSRD_E_INVALID_ARGUMENT;
    const size_t total = static_cast<size_t>(config->num_rays) * config->num_samples;
    const int blocks = static_cast<int>(std::min<size_t>((total + 255) / 256, 8192));
    hipLaunchKernelGGL(sample_stratified_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       render_args(config), u_coarse, distances);
    return launch_status();
}

int32_t vsrd_sample_importance(const vsrd_render_config* config, const float* coarse_distances,
                               const float* coarse_weights, const float* u_fine, float* merged, float* fine, void* stream) {
    if (config != nullptr && config->num_frames > 1) return VSRD_E_UNSUPPORTED;      // (frame batches: the per-frame step entry points only)
    if (!valid_config(config)) return VSRD_E_INVALID_ARGUMENT;
    if (config->num_rays == 0) return VSRD_OK;
    if (!coarse_distances || !coarse_weights || !u_fine || (!merged && !fine)) return VSRD_E_INVALID_ARGUMENT;
    Geometry g;
    if (!plan(config->num_rays, wave_lds_floats(config->num_samples, 0), &g)) return VSRD_E_UNSUPPORTED;
    const RenderArgs c = render_args(config);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const bool known = for_rounds<1, 2, 4>(rounds_for(config->num_samples), [&](auto k) {
        hipLaunchKernelGGL(sample_importance_kernel<decltype(k)::value>, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, c, coarse_distances,
                           coarse_weights, u_fine, merged, fine);
    });
    if (!known) return VSRD_E_UNSUPPORTED;
    return launch_status();
}

int32_t vsrd_render_forward(const vsrd_field* field, const vsrd_render_config* config,
                            const float* origins, const float* directions,
                            const float* distances, int32_t num_distances,
                            float* labels, float* gradients, float* weights, void* stream) {
    if (config != nullptr && config->num_frames > 1) return VSRD_E_UNSUPPORTED;      // (frame batches: the per-frame step entry points only)
    if (!valid_field(field) || !valid_config(config) || num_distances < 2 || num_distances > 2 * VSRD_MAX_SAMPLES)
        return VSRD_E_INVALID_ARGUMENT;
    if (config->num_rays == 0) return VSRD_OK;   // empty batch: buffers may be null
    if (!origins || !directions || !distances || !labels) return VSRD_E_INVALID_ARGUMENT;
    const bool residual = field->mlp_weights != nullptr;
    Geometry g;
    if (!plan(config->num_rays, static_cast<size_t>(forward_lds_floats(num_distances, field->num_instances, residual)), &g)) return VSRD_E_UNSUPPORTED;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t status = VSRD_OK;
    auto launch = [&](auto k, auto res) {
        constexpr auto kernel = render_forward_kernel<decltype(k)::value, decltype(res)::value>;
        if ((status = opt_in_lds(kernel, g.lds_bytes)) != VSRD_OK) return;
        fit_to_residency(kernel, &g);
        hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, f, field->instances, field->mlp_weights, c, origins, directions, distances,
                           num_distances, labels, gradients, weights);
    };
    const int rounds = rounds_for(num_distances - 1);
    const bool known = residual ? for_rounds<1, 2, 4>(rounds, [&](auto k) { launch(k, std::true_type{}); })
                                : for_rounds<1, 2, 4, 8>(rounds, [&](auto k) { launch(k, std::false_type{}); });
    if (!known) return VSRD_E_UNSUPPORTED;
    if (status != VSRD_OK) return status;
    return launch_status();
}

int32_t vsrd_render_backward(const vsrd_field* field, const vsrd_render_config* config,
                             const float* origins, const float* directions,
                             const float* distances, int32_t num_distances,
                             const float* grad_labels, const float* grad_gradients, const float* grad_weights,
                             void* workspace, size_t workspace_bytes,
                             float* grad_instances, float* grad_mlp_weights, void* stream) {
    if (config != nullptr && config->num_frames > 1) return VSRD_E_UNSUPPORTED;      // (frame batches: the per-frame step entry points only)
    if (!valid_field(field) || !valid_config(config) || !grad_instances || !workspace || num_distances < 2 ||
        num_distances > 2 * VSRD_MAX_SAMPLES)
        return VSRD_E_INVALID_ARGUMENT;
    if (config->num_rays > 0 && (!origins || !directions || !distances || !grad_labels)) return VSRD_E_INVALID_ARGUMENT;
    const bool residual = field->mlp_weights != nullptr;
    if (residual && !grad_mlp_weights) return VSRD_E_INVALID_ARGUMENT;
    const int N = field->num_instances;
    if (workspace_bytes < vsrd_workspace_bytes(N, residual)) return VSRD_E_WORKSPACE;
    if (residual && config->num_rays > 0 && !(config->flags & VSRD_FLAG_RESIDUAL_SINGLE_KERNEL)) {
        // two kernels per chunk of rays (front part + MLP adjoint by instance) when the workspace holds a chunk's seeds
        bool taken = false;
        const int32_t status = render_backward_split(field, config, origins, directions, distances, num_distances, grad_labels, grad_gradients,
                                                     grad_weights, workspace, workspace_bytes, grad_instances, grad_mlp_weights, stream, &taken);
        if (taken) return status;
    }
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int row = N * kGradStride;
    const int mlp_row = N * kMlpWeights;
    if (config->num_rays == 0) {
        if (residual && hipMemsetAsync(grad_mlp_weights, 0, mlp_row * sizeof(float), s) != hipSuccess) return VSRD_E_LAUNCH;
        return hipMemsetAsync(grad_instances, 0, row * sizeof(float), s) == hipSuccess ? VSRD_OK : VSRD_E_LAUNCH;
    }
    Geometry g;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    // box-only fields, label adjoints only: the mappings of the fused step (quad_step.h), two kernels on one grid (backward_rows_kernel_body)
    // (allowed: a box-only field and no adjoints but the labels' -- the rows kernels carry neither the MLP nor per-sample adjoints)
    const RowsPlan r = plan_rows(N, num_distances, config->num_rays, config->flags, !residual && !grad_gradients && !grad_weights);
    if (r.rows) {
        if (!plan(static_cast<int>(r.num_groups), r.lds_floats, &g)) return VSRD_E_UNSUPPORTED;
        if (!cap_to_workspace(workspace_bytes, row, r.flag_bytes, &g)) return VSRD_E_WORKSPACE;
        const int num_waves = g.blocks * (g.threads / kWave);
        float* partials = static_cast<float*>(workspace);
        unsigned char* redo_flags = reinterpret_cast<unsigned char*>(partials + static_cast<size_t>(num_waves) * row);
        if (hipMemsetAsync(redo_flags, 0, 16, s) != hipSuccess) return VSRD_E_LAUNCH;
        for_bool(r.full, [&](auto full) {
            auto launch = [&](auto hot, auto rest) {
                launch_hot_then_rest(hot, rest, g, s, f, field->instances, c, origins, directions, distances, num_distances, grad_labels, partials, redo_flags);
            };
            if (r.quad) launch(render_backward_quad_kernel<true, decltype(full)::value>, render_backward_quad_kernel<false, false>);
            else launch(render_backward_pair_kernel<true, decltype(full)::value>, render_backward_pair_kernel<false, false>);
        });
        if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
        launch_reduce_rows(partials, num_waves, row, grad_instances, nullptr, 0, nullptr, workspace, workspace_bytes, s);
        return launch_status();
    }
    if (!plan(config->num_rays, static_cast<size_t>(backward_lds_floats(num_distances, N, residual)), &g)) return VSRD_E_UNSUPPORTED;
    if (residual && g.threads > kResidualWaves * kWave) return VSRD_E_UNSUPPORTED;      // cannot happen (LDS per wave), but the scratch is sized for it
    if (residual && g.blocks > kMaxBlocksResidual) g.blocks = kMaxBlocksResidual;
    const OneKernelWorkspace w = one_kernel_workspace(workspace, N, residual);
    bool known = false;
    for_bool(residual, [&](auto res) {
        known = for_rounds<1, 2, 4>(rounds_for(num_distances - 1), [&](auto k) {
            constexpr auto kernel = render_backward_kernel<decltype(k)::value, decltype(res)::value>;
            fit_to_residency(kernel, &g);
            if (residual && g.blocks > kMaxBlocksResidual) g.blocks = kMaxBlocksResidual;
            hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, f, field->instances, field->mlp_weights, c, origins, directions, distances,
                               num_distances, grad_labels, grad_gradients, grad_weights, w.partials, w.mlp_partials, w.jets, w.seeds);
        });
    });
    if (!known) return VSRD_E_UNSUPPORTED;
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    const int num_waves = g.blocks * (g.threads / kWave);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(row), dim3(256), 0, s, w.partials, num_waves, row, grad_instances);
    if (residual)
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(mlp_row), dim3(256), 0, s, w.mlp_partials, num_waves, mlp_row, grad_mlp_weights);
    return launch_status();
}

int32_t vsrd_render_hierarchical_forward(const vsrd_field* field, const vsrd_render_config* config,
                                         const float* origins, const float* directions,
                                         const float* u_coarse, const float* u_fine,
                                         float* labels, float* distances, float* gradients, float* weights, float* coarse_weights,
                                         float* u_coarse_out, float* u_fine_out, void* stream) {
    if (config != nullptr && config->num_frames > 1) return VSRD_E_UNSUPPORTED;      // (frame batches: the per-frame step entry points only)
    if (!valid_field(field) || !valid_config(config)) return VSRD_E_INVALID_ARGUMENT;
    if (config->num_rays == 0) return VSRD_OK;   // empty batch: buffers may be null
    if (!origins || !directions || !labels) return VSRD_E_INVALID_ARGUMENT;
    const bool residual = field->mlp_weights != nullptr;
    if ((config->flags & VSRD_FLAG_SKIP_EXACT_MISSES) && (gradients || weights)) return VSRD_E_INVALID_ARGUMENT;
    const int S = config->num_samples;
    Geometry g;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // labels, distances, pass 1's weights and the uniforms only (no per-sample gradients / weights of pass 2), box-only field: the forward
    // in the mappings of the fused step (quad_step.h), two kernels on one grid (hierarchical_rows_kernel_body)
    // (allowed: a box-only field and no per-sample outputs of pass 2, which the rows kernels do not write)
    const RowsPlan r = plan_rows(field->num_instances, 2 * S, config->num_rays, config->flags, !residual && !gradients && !weights);
    if (r.rows) {
        if (!plan(static_cast<int>(r.num_groups), r.lds_floats, &g)) return VSRD_E_UNSUPPORTED;
        for_bool(r.full, [&](auto full) {
            auto launch = [&](auto hot, auto rest) {
                launch_hot_then_rest(hot, rest, g, s, f, field->instances, c, origins, directions, u_coarse, u_fine, labels, distances, coarse_weights, u_coarse_out, u_fine_out);
            };
            if (r.quad) launch(render_hierarchical_quad_kernel<true, decltype(full)::value>, render_hierarchical_quad_kernel<false, false>);
            else launch(render_hierarchical_pair_kernel<true, decltype(full)::value>, render_hierarchical_pair_kernel<false, false>);
        });
        return launch_status();
    }
    if (!plan(config->num_rays, static_cast<size_t>(hierarchical_lds_floats(S, field->num_instances, residual)), &g)) return VSRD_E_UNSUPPORTED;
    int32_t status = VSRD_OK;
    auto launch = [&](auto k, auto res) {
        constexpr auto kernel = render_hierarchical_kernel<decltype(k)::value, decltype(res)::value>;
        if ((status = opt_in_lds(kernel, g.lds_bytes)) != VSRD_OK) return;
        fit_to_residency(kernel, &g);
        hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, f, field->instances, field->mlp_weights, c, origins, directions, u_coarse, u_fine,
                           labels, distances, gradients, weights, coarse_weights, u_coarse_out, u_fine_out);
    };
    const int rounds = rounds_for(2 * S - 1);
    const bool known = residual ? for_rounds<1, 2, 4>(rounds, [&](auto k) { launch(k, std::true_type{}); })
                                : for_rounds<1, 2, 4, 8>(rounds, [&](auto k) { launch(k, std::false_type{}); });
    if (!known) return VSRD_E_UNSUPPORTED;
    if (status != VSRD_OK) return status;
    return launch_status();
}

int32_t vsrd_project_boxes_forward(const float* world_corners, const float* extrinsics, const float* intrinsics,
                                   const int32_t* edges, int32_t num_edges, int32_t num_views, int32_t num_boxes,
                                   int32_t height, int32_t width, float epsilon,
                                   float* boxes_2d, float* camera_corners, int32_t* selection, void* stream) {
    if (num_views < 0 || num_boxes < 0 || num_edges < 1 || num_edges > kMaxEdges) return VSRD_E_INVALID_ARGUMENT;
    if (num_views == 0 || num_boxes == 0) return VSRD_OK;
    if (!world_corners || !extrinsics || !intrinsics || !edges || !boxes_2d || !selection) return VSRD_E_INVALID_ARGUMENT;
    const int total = num_views * num_boxes;
    hipLaunchKernelGGL(project_boxes_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       world_corners, extrinsics, intrinsics, edges, num_edges, num_views, num_boxes,
                       static_cast<float>(height), static_cast<float>(width), epsilon, boxes_2d, camera_corners, selection);
    return launch_status();
}

int32_t vsrd_project_boxes_backward(const float* world_corners, const float* extrinsics, const float* intrinsics,
                                    const int32_t* edges, int32_t num_edges, int32_t num_views, int32_t num_boxes, float epsilon,
                                    const float* grad_boxes_2d, const int32_t* selection, float* grad_world_per_view, void* stream) {
    if (num_views < 0 || num_boxes < 0 || num_edges < 1 || num_edges > kMaxEdges) return VSRD_E_INVALID_ARGUMENT;
    if (num_views == 0 || num_boxes == 0) return VSRD_OK;
    if (!world_corners || !extrinsics || !intrinsics || !edges || !grad_boxes_2d || !selection || !grad_world_per_view)
        return VSRD_E_INVALID_ARGUMENT;
    const int total = num_views * num_boxes;
    hipLaunchKernelGGL(project_boxes_backward_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       world_corners, extrinsics, intrinsics, edges, num_views, num_boxes, epsilon, grad_boxes_2d, selection,
                       grad_world_per_view);
    return launch_status();
}

namespace {
constexpr int kSplitBlocks = 1024;                       // render_silhouette_split_kernel: x 2 waves = two waves on each of the 1024 SIMDs
}  // namespace

int32_t vsrd_render_silhouette_step(const vsrd_field* field, const vsrd_render_config* config,
                                    const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                    const float* targets, const float* instance_weights, float loss_scale,
                                    void* workspace, size_t workspace_bytes,
                                    float* loss, float* grad_instances, float* labels, void* stream) {
    return vsrd_render_silhouette_step_with_header(field, config, origins, directions, u_coarse, u_fine, targets, instance_weights, loss_scale, workspace,
                                                   workspace_bytes, loss, grad_instances, labels, nullptr, stream);
}

int32_t vsrd_render_silhouette_step_with_header(const vsrd_field* field, const vsrd_render_config* config,
                                                const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                                const float* targets, const float* instance_weights, float loss_scale,
                                                void* workspace, size_t workspace_bytes,
                                                float* loss, float* grad_instances, float* labels, const vsrd_frame_header* frame_header, void* stream) {
    if (!valid_field(field) || !valid_config(config, true, true) || !workspace || !loss || !grad_instances) return VSRD_E_INVALID_ARGUMENT;
    if (field->mlp_weights != nullptr) return VSRD_E_UNSUPPORTED;            // box-only fast path
    const int N = field->num_instances;
    if (workspace_bytes < vsrd_workspace_bytes(N, 0)) return VSRD_E_WORKSPACE;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int row = N * kGradStride;
    Frames frames;
    frames_of(config->num_frames, config->frame_stride, &frames);           // (validated by valid_config)
    if ((frames.count > 1 || frame_header) && (config->num_rays == 0 || wants_samples(config))) return VSRD_E_UNSUPPORTED;
    const FrameHeader* header = reinterpret_cast<const FrameHeader*>(frame_header);
    if (config->num_rays == 0) {
        if (hipMemsetAsync(loss, 0, sizeof(float), s) != hipSuccess) return VSRD_E_LAUNCH;
        return hipMemsetAsync(grad_instances, 0, row * sizeof(float), s) == hipSuccess ? VSRD_OK : VSRD_E_LAUNCH;
    }
    if (!origins || !directions || !targets) return VSRD_E_INVALID_ARGUMENT;
    const int S = config->num_samples;
    const int rounds = rounds_for(2 * S - 1);
    if (rounds < 1 || rounds > 4) return VSRD_E_UNSUPPORTED;
    // dense launches of the benchmark shapes: four neighbouring rays per wave (quad_step.h).  Gathered rays (the reference's 1000
    // importance-sampled rays per step) are neither neighbours nor enough to fill the chip four to a wave.
    const bool force_split = (config->flags & VSRD_FLAG_STEP_SPLIT_RAY) && !(config->flags & VSRD_FLAG_STEP_WAVE_PER_RAY);
    // (dense = rays AND targets read row by row: the multi-ray kernels know neither ray_indices nor the target column map)
    // (allowed: a dense launch that was not asked to split its rays)
    const RowsPlan r = plan_rows(N, 2 * S, config->num_rays, config->flags,
                                 config->ray_indices == nullptr && config->target_columns == nullptr && !(config->flags & VSRD_FLAG_STEP_SPLIT_RAY));
    // ... and for more instances or samples than a quad takes (BASELINE config 5: N = 64, S = 128) two rays per wave, 32 lanes each (plan_rows)
    // ... and for launches too small to put two waves on every SIMD one ray per wave (the reference's 1000 sampled rays per step: 1000
    // waves on 1024 SIMDs, pure latency), a ray split over the two waves of a workgroup (render_silhouette_split_kernel)
    // (a step that writes its samples out -- vsrd_render_config::out_* -- keeps one ray per wave: the split form has no such outputs)
    const bool split = !r.rows && !(config->flags & VSRD_FLAG_STEP_WAVE_PER_RAY) && !wants_samples(config) && (rounds == 2 || rounds == 4) &&
                       (force_split || config->num_rays <= switches().split_max_rays) &&
                       static_cast<size_t>(split_lds_floats(S, N)) * sizeof(float) <= kLdsLimit / 2;
    if (split) {
        const int blocks = config->num_rays < kSplitBlocks ? config->num_rays : kSplitBlocks;
        const int num_waves = blocks * kPairWaves;
        if (static_cast<size_t>(num_waves) * (row + 1) * sizeof(float) > workspace_bytes) return VSRD_E_WORKSPACE;
        if (frames.count > 1 && static_cast<long long>(workspace_bytes) > frames.stride) return VSRD_E_INVALID_ARGUMENT;      // (the frames' workspaces would overlap)
        const size_t lds_bytes = static_cast<size_t>(split_lds_floats(S, N)) * sizeof(float);
        const FieldArgs f = field_args(field);
        RenderArgs c = render_args(config);
        c.sh.inv_t = f.inv_t;
        float* partials = static_cast<float*>(workspace);
        float* loss_partials = partials + static_cast<size_t>(num_waves) * row;
        int32_t status = VSRD_OK;
        for_rounds<2, 4>(rounds, [&](auto k) {
            for_bool(frames.count > 1 || header, [&](auto batch) {
                constexpr auto kernel = render_silhouette_split_kernel<decltype(k)::value, decltype(batch)::value>;
                if ((status = opt_in_lds(kernel, lds_bytes)) != VSRD_OK) return;
                hipLaunchKernelGGL(kernel, dim3(blocks, frames.count), dim3(kPairWaves * kWave), lds_bytes, s, f, field->instances, c, origins, directions, u_coarse,
                                   u_fine, targets, instance_weights, loss_scale, labels, partials, loss_partials, header);
            });
        });
        if (status != VSRD_OK) return status;
        if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(row + 1, frames.count), dim3(256), 0, s, partials, num_waves, row, grad_instances, nullptr, loss_partials, 1, loss,
                           frames.stride, header);
        return launch_status();
    }
    if (frames.count > 1 || header) return VSRD_E_UNSUPPORTED;     // a batch of frames runs in the split-ray form only (gathered launches of at most 2048 rays per frame)
    Geometry g;
    if (!plan(r.rows ? static_cast<int>(r.num_groups) : config->num_rays, r.rows ? r.lds_floats : static_cast<size_t>(wave_lds_floats(S, N)) + N + row, &g))
        return VSRD_E_UNSUPPORTED;
    // one gradient row and one loss partial per wave, and behind them (multi-ray mappings) the groups' flags
    if (!cap_to_workspace(vsrd_workspace_bytes(N, 0), row + 1, r.flag_bytes, &g)) return VSRD_E_WORKSPACE;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    const int num_waves = g.blocks * (g.threads / kWave);
    float* partials = static_cast<float*>(workspace);
    float* loss_partials = partials + static_cast<size_t>(num_waves) * row;
    unsigned char* redo_flags = reinterpret_cast<unsigned char*>(loss_partials + num_waves);
    int32_t status = VSRD_OK;
    bool known = true;
    if (r.rows) {
        // (exactly the launches that fill their shape get a <4, true, true> kernel: S = 4 x lanes)
        auto launch = [&](auto hot, auto rest) {
            if ((status = opt_in_lds(hot, g.lds_bytes)) != VSRD_OK || (status = opt_in_lds(rest, g.lds_bytes)) != VSRD_OK) return;
            if (hipMemsetAsync(redo_flags, 0, 16, s) != hipSuccess) { status = VSRD_E_LAUNCH; return; }
            launch_hot_then_rest(hot, rest, g, s, f, field->instances, c, origins, directions, u_coarse, u_fine, targets, instance_weights, loss_scale, labels, partials,
                                 loss_partials, redo_flags);
        };
        // (... and of those the launches with VSRD_FLAG_YAW_GRADIENTS a hot kernel that has the flag compiled in: quad_step.h, quad_phase_b.
        //  The hot kernel runs only fields whose rotations are all about y, so the flag alone decides)
        const bool yaw_only = (config->flags & VSRD_FLAG_YAW_GRADIENTS) != 0u;
        if (r.quad && r.full) for_bool(yaw_only, [&](auto y) {
            launch(render_silhouette_quad_kernel<4, true, true, decltype(y)::value>, render_silhouette_quad_kernel<4, false, false>); });
        else if (r.full) for_bool(yaw_only, [&](auto y) {
            launch(render_silhouette_pair_kernel<4, true, true, decltype(y)::value>, render_silhouette_pair_kernel<4, false, false>); });
        else if (r.quad) known = for_rounds<1, 2, 4>(r.rounds, [&](auto k) {
            launch(render_silhouette_quad_kernel<decltype(k)::value, true, false>, render_silhouette_quad_kernel<decltype(k)::value, false, false>); });
        else known = for_rounds<2, 4>(r.rounds, [&](auto k) {
            launch(render_silhouette_pair_kernel<decltype(k)::value, true, false>, render_silhouette_pair_kernel<decltype(k)::value, false, false>); });
    } else {
        known = for_rounds<1, 2, 4>(rounds, [&](auto k) {
            constexpr auto kernel = render_silhouette_kernel<decltype(k)::value>;
            if ((status = opt_in_lds(kernel, g.lds_bytes)) != VSRD_OK) return;
            hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, f, field->instances, c, origins, directions, u_coarse, u_fine, targets,
                               instance_weights, loss_scale, labels, partials, loss_partials);
        });
    }
    if (!known) return VSRD_E_UNSUPPORTED;
    if (status != VSRD_OK) return status;
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    launch_reduce_rows(partials, num_waves, row, grad_instances, loss_partials, 1, loss, workspace, vsrd_workspace_bytes(N, 0), s);
    return launch_status();
}

static int32_t residual_step_single_kernel(const vsrd_field* field, const vsrd_render_config* config,
                                  const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                  const float* targets, const float* instance_weights, float loss_scale, float eikonal_ratio,
                                  void* workspace, size_t workspace_bytes,
                                  float* losses, float* grad_instances, float* grad_mlp_weights, float* labels, void* stream) {
    if (!valid_field(field) || !valid_config(config, true) || !workspace || !losses || !grad_instances || !grad_mlp_weights) return VSRD_E_INVALID_ARGUMENT;
    if (field->mlp_weights == nullptr) return VSRD_E_INVALID_ARGUMENT;       // box-only fields: vsrd_render_silhouette_step
    const int N = field->num_instances;
    if (workspace_bytes < vsrd_workspace_bytes(N, 1)) return VSRD_E_WORKSPACE;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int row = N * kGradStride, mlp_row = N * kMlpWeights;
    if (config->num_rays == 0) {
        if (hipMemsetAsync(losses, 0, 2 * sizeof(float), s) != hipSuccess) return VSRD_E_LAUNCH;
        if (hipMemsetAsync(grad_mlp_weights, 0, mlp_row * sizeof(float), s) != hipSuccess) return VSRD_E_LAUNCH;
        return hipMemsetAsync(grad_instances, 0, row * sizeof(float), s) == hipSuccess ? VSRD_OK : VSRD_E_LAUNCH;
    }
    if (!origins || !directions || !targets) return VSRD_E_INVALID_ARGUMENT;
    const int S = config->num_samples;
    const int num_points = 2 * S - 1;
    const int rounds = rounds_for(num_points);
    Geometry g;
    if (!plan(config->num_rays, static_cast<size_t>(residual_step_lds_floats(S, N)), &g)) return VSRD_E_UNSUPPORTED;
    if (g.threads > kResidualWaves * kWave) return VSRD_E_UNSUPPORTED;
    if (g.blocks > kMaxBlocksResidual) g.blocks = kMaxBlocksResidual;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    const int num_waves = g.blocks * (g.threads / kWave);
    const OneKernelWorkspace w = one_kernel_workspace(workspace, N, true);
    float* loss_partials = w.partials + static_cast<size_t>(num_waves) * row;           // inside the (much larger) box-partial region
    // d/dg of  eikonal_ratio * mean over [R, 2S-1] of (|g| - 1)^2 ;  the reported eikonal term is the plain mean
    const float eikonal_norm = 1.0f / (static_cast<float>(config->num_rays) * static_cast<float>(num_points));
    const float eikonal_scale = eikonal_ratio * eikonal_norm;
    int32_t status = VSRD_OK;
    const bool known = for_rounds<1, 2, 4>(rounds, [&](auto k) {
        constexpr auto kernel = render_residual_step_kernel<decltype(k)::value>;
        if ((status = opt_in_lds(kernel, g.lds_bytes)) != VSRD_OK) return;
        hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, s, f, field->instances, field->mlp_weights, c, origins, directions, u_coarse, u_fine,
                           targets, instance_weights, loss_scale, eikonal_scale, eikonal_norm, labels, w.partials, w.mlp_partials, w.jets, w.seeds, loss_partials);
    });
    if (!known) return VSRD_E_UNSUPPORTED;
    if (status != VSRD_OK) return status;
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(row), dim3(256), 0, s, w.partials, num_waves, row, grad_instances);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(mlp_row), dim3(256), 0, s, w.mlp_partials, num_waves, mlp_row, grad_mlp_weights);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(2), dim3(256), 0, s, loss_partials, num_waves, 2, losses);
    return launch_status();
}

size_t vsrd_render_backward_workspace_bytes(int32_t num_instances, int32_t residual, int32_t num_distances, int32_t num_rays) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES || num_distances < 2 || num_distances > 2 * VSRD_MAX_SAMPLES || num_rays < 0) return 0;
    size_t need = vsrd_workspace_bytes(num_instances, residual);
    ResidualStepPlan p;
    if (residual && num_rays > 0 && plan_backward_split(num_instances, num_distances, num_rays, ~size_t(0), &p) && p.total_bytes > need) need = p.total_bytes;
    return need;
}

size_t vsrd_residual_step_workspace_bytes(int32_t num_instances, int32_t num_samples, int32_t num_rays) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES || num_samples < 2 || num_samples > VSRD_MAX_SAMPLES || num_rays < 0) return 0;
    ResidualStepPlan p;
    size_t need = vsrd_workspace_bytes(num_instances, 1);                 // (VSRD_FLAG_RESIDUAL_SINGLE_KERNEL and shapes the split form does not take)
    for (int allow_pair = 0; allow_pair < 2; ++allow_pair)                // (either front kernel: VSRD_FLAG_RESIDUAL_WAVE_PER_RAY)
        if (plan_residual_step(num_instances, num_samples, num_rays, allow_pair != 0, &p) && p.total_bytes > need) need = p.total_bytes;
    return need;
}

int32_t vsrd_render_residual_step(const vsrd_field* field, const vsrd_render_config* config,
                                  const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                  const float* targets, const float* instance_weights, float loss_scale, float eikonal_ratio,
                                  void* workspace, size_t workspace_bytes,
                                  float* losses, float* grad_instances, float* grad_mlp_weights, float* labels, void* stream) {
    return vsrd_render_residual_step_with_header(field, config, origins, directions, u_coarse, u_fine, targets, instance_weights, loss_scale, eikonal_ratio,
                                                 workspace, workspace_bytes, losses, grad_instances, grad_mlp_weights, labels, nullptr, stream);
}

int32_t vsrd_render_residual_step_with_header(const vsrd_field* field, const vsrd_render_config* config,
                                              const float* origins, const float* directions, const float* u_coarse, const float* u_fine,
                                              const float* targets, const float* instance_weights, float loss_scale, float eikonal_ratio,
                                              void* workspace, size_t workspace_bytes,
                                              float* losses, float* grad_instances, float* grad_mlp_weights, float* labels,
                                              const vsrd_frame_header* frame_header, void* stream) {
    if (!valid_field(field) || !valid_config(config, true, true) || !workspace || !losses || !grad_instances || !grad_mlp_weights) return VSRD_E_INVALID_ARGUMENT;
    if (field->mlp_weights == nullptr) return VSRD_E_INVALID_ARGUMENT;       // box-only fields: vsrd_render_silhouette_step
    const int N = field->num_instances, S = config->num_samples;
    ResidualStepPlan p;
    // (a step that writes its samples out -- vsrd_render_config::out_* -- keeps one ray per wave: the split-ray and the one-kernel forms have no such outputs)
    const bool allow_pair = !(config->flags & VSRD_FLAG_RESIDUAL_WAVE_PER_RAY) && !wants_samples(config);
    if (wants_samples(config) && (config->flags & VSRD_FLAG_RESIDUAL_SINGLE_KERNEL)) return VSRD_E_UNSUPPORTED;
    Frames frames;
    frames_of(config->num_frames, config->frame_stride, &frames);           // (validated by valid_config)
    if (config->adjoint_slots_per_item < 0 || config->adjoint_slots_per_item > 64) return VSRD_E_INVALID_ARGUMENT;
    const bool one_kernel = (config->flags & VSRD_FLAG_RESIDUAL_SINGLE_KERNEL) || config->num_rays == 0 ||
                            !plan_residual_step(N, S, config->num_rays, allow_pair, &p, config->adjoint_slots_per_item);
    // a batch of frames: the two-kernel form with every frame's rays in ONE chunk (each frame its own seeds, item counter and rows, frame_stride apart)
    if (frames.count > 1 && (one_kernel || p.chunk < config->num_rays || static_cast<long long>(p.total_bytes) > frames.stride)) return VSRD_E_UNSUPPORTED;
    // a per-frame header (mixed batches): the forms that batch -- two kernels, the ray split over a pair of waves, one chunk, no sample outputs
    const FrameHeader* header = reinterpret_cast<const FrameHeader*>(frame_header);
    if (header && (one_kernel || !p.pair || p.chunk < config->num_rays || wants_samples(config))) return VSRD_E_UNSUPPORTED;
    if (one_kernel && wants_samples(config)) return VSRD_E_UNSUPPORTED;
    if (one_kernel)
        return residual_step_single_kernel(field, config, origins, directions, u_coarse, u_fine, targets, instance_weights, loss_scale, eikonal_ratio,
                                           workspace, workspace_bytes, losses, grad_instances, grad_mlp_weights, labels, stream);
    if (workspace_bytes < p.total_bytes) return VSRD_E_WORKSPACE;
    if (!origins || !directions || !targets) return VSRD_E_INVALID_ARGUMENT;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int row = N * kGradStride;
    const int num_points = 2 * S - 1;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    const SplitWorkspace w = split_workspace(workspace, p);
    const float eikonal_norm = 1.0f / (static_cast<float>(config->num_rays) * static_cast<float>(num_points));
    const float eikonal_scale = eikonal_ratio * eikonal_norm;
    // VSRD_FLAG_MLP_SPLIT_BF16: the front kernels of the OTHER translation unit (split_front.hip), which read the instances' split-bf16
    // operand images instead of their weights
    const bool split = (config->flags & VSRD_FLAG_MLP_SPLIT_BF16) != 0u;
    if (split && vsrd_split_front::pack_images(field->mlp_weights, N, (config->flags & VSRD_FLAG_MLP_WEIGHTS_CENTRED) ? 1 : 0, w.images, frames.count, frames.stride,
                                               header, s) != vsrd_split_front::kOk)
        return VSRD_E_LAUNCH;
    const float* front_weights = split ? reinterpret_cast<const float*>(w.images) : field->mlp_weights;
    int chunk_index = 0;
    for (int first = 0; first < config->num_rays; first += p.chunk, ++chunk_index) {
        const int rays = std::min(p.chunk, config->num_rays - first);
        if (!clear_frames(w.masks, w.clear_bytes, frames, s)) return VSRD_E_LAUNCH;
        // the front kernel: one dispatch (launch.h), this unit's copy for the fp32 products and split_front.hip's for the split-bf16 ones
        const vsrd_split_front::FrontLaunch launch = {&f, sizeof f, &c, sizeof c, field->instances, front_weights, origins, directions, u_coarse, u_fine, targets,
                                                      instance_weights, loss_scale, eikonal_scale, eikonal_norm, labels, w.box_partials, w.jets, w.loss_partials, w.seeds,
                                                      w.masks, p.slots_per_instance, first, rays, chunk_index > 0 ? 1 : 0, p.pair, p.rounds, p.front_blocks, p.front_lds,
                                                      wants_samples(config), frames.count, frame_header};
        const int code = split ? vsrd_split_front::launch_front(launch, s, debug()) : vsrd::launch_front(launch, s, debug());
        if (code != vsrd_split_front::kOk) return code == vsrd_split_front::kUnsupported ? VSRD_E_UNSUPPORTED : VSRD_E_LAUNCH;
        const int32_t status = launch_adjoint_tail(field, split ? w.images : nullptr, config->flags, p, w, rays, chunk_index > 0, grad_mlp_weights, frames, header, s);
        if (status != VSRD_OK) return status;
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(row + 2, frames.count), dim3(256), 0, s, w.box_partials, p.front_waves, row, grad_instances, w.box_extra, w.loss_partials, 2,
                       losses, frames.stride, header);
    return launch_status();
}

size_t vsrd_frame_scratch_bytes(int32_t num_views, int32_t num_boxes) {
    if (num_views < 1 || num_views > kFrameMaxViews || num_boxes < 1 || num_boxes > kFrameMaxBoxes) return 0;
    return frame_scratch_floats(num_views, num_boxes) * sizeof(float);
}

namespace {
// What every frame kernel reads of a vsrd_frame_config -- the sizes, the image, the projection's guard, the decode's ranges and the batch stride --
// with the frame header: the ONE reader of those fields.  It refuses what every entry point refuses (the box count, the batch fields); the
// view and step counts are checked by the entry points that read them.
bool frame_shape(const vsrd_frame_config* c, const vsrd_frame_header* frame_header, FrameStepArgs* a, Frames* frames) {
    if (!c || c->num_boxes < 1 || c->num_boxes > kFrameMaxBoxes || !frames_of(c->num_frames, c->frame_stride, frames)) return false;
    *a = FrameStepArgs{};
    a->num_boxes = c->num_boxes; a->num_views = c->num_views;
    a->height = c->height; a->width = c->width; a->epsilon = c->epsilon;
    for (int j = 0; j < 3; ++j) {
        a->location_lo[j] = c->location_lo[j]; a->location_hi[j] = c->location_hi[j];
        a->dimension_lo[j] = c->dimension_lo[j]; a->dimension_hi[j] = c->dimension_hi[j];
    }
    a->frame_stride = frames->stride;
    a->header = reinterpret_cast<const FrameHeader*>(frame_header);
    return true;
}
bool valid_views(const vsrd_frame_config* c) { return c->num_views >= 1 && c->num_views <= kFrameMaxViews; }
// frame_shape and what the prologues and the epilogue alone read: the steps, the schedules, the loss weights and Adam's constants
bool frame_args(const vsrd_frame_config* c, const vsrd_frame_header* frame_header, FrameStepArgs* a, Frames* frames) {
    if (!frame_shape(c, frame_header, a, frames) || !valid_views(c) || c->num_steps < 1) return false;
    a->num_steps = c->num_steps;
    a->max_temperature = c->max_temperature; a->min_temperature = c->min_temperature; a->max_std = c->max_std; a->min_std = c->min_std;
    a->weight_iou = c->weight_iou; a->weight_l1 = c->weight_l1; a->weight_silhouette = c->weight_silhouette;
    a->beta1 = c->beta1; a->beta2 = c->beta2; a->adam_epsilon = c->adam_epsilon; a->lr_gamma = c->lr_gamma;
    return true;
}
// the buffers of a frame's prologue, none of which may be null (the scratch apart: its size is the caller's next check)
bool frame_buffers(const float* raw_locations, const float* raw_dimensions, const float* raw_orientations, const float* extrinsics, const float* intrinsics,
                   const float* gt_boxes, const uint8_t* visible, const int64_t* step, void* scratch, float* instances, int64_t* pd_indices, int64_t* gt_indices,
                   int32_t* target_columns, float* instance_weights, float* schedule, float* projection_losses, float* grad_raw, FrameBuffers* b) {
    if (!raw_locations || !raw_dimensions || !raw_orientations || !extrinsics || !intrinsics || !gt_boxes || !visible || !step || !instances ||
        !pd_indices || !gt_indices || !target_columns || !instance_weights || !schedule || !projection_losses || !grad_raw)
        return false;
    b->raw_locations = raw_locations; b->raw_dimensions = raw_dimensions; b->raw_orientations = raw_orientations;
    b->extrinsics = extrinsics; b->intrinsics = intrinsics; b->gt_boxes = gt_boxes; b->visible = visible;
    b->step = reinterpret_cast<const long long*>(step);
    b->scratch = static_cast<float*>(scratch);
    b->instances = instances;
    b->pd_indices = reinterpret_cast<long long*>(pd_indices); b->gt_indices = reinterpret_cast<long long*>(gt_indices);
    b->target_map = target_columns; b->instance_weights = instance_weights; b->schedule = schedule; b->losses = projection_losses; b->grad_raw = grad_raw;
    return true;
}
bool valid_adam(const vsrd_adam_tensors& t) { return t.parameter && t.exp_avg && t.exp_avg_sq && t.step && t.learning_rate; }
AdamTensors adam_tensors(const vsrd_adam_tensors& t) { return AdamTensors{t.parameter, t.exp_avg, t.exp_avg_sq, t.step, t.learning_rate}; }
}  // namespace

int32_t vsrd_frame_prologue(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                            const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                            const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                            float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                            float* schedule, float* projection_losses, float* grad_raw, void* stream) {
    return vsrd_frame_prologue_with_header(config, raw_locations, raw_dimensions, raw_orientations, extrinsics, intrinsics, gt_boxes, visible, step, scratch,
                                           scratch_bytes, instances, pd_indices, gt_indices, target_columns, instance_weights, schedule, projection_losses,
                                           grad_raw, nullptr, stream);
}

int32_t vsrd_frame_prologue_with_header(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                                        const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                                        const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                                        float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                                        float* schedule, float* projection_losses, float* grad_raw, const vsrd_frame_header* frame_header, void* stream) {
    FrameStepArgs a;
    Frames frames;
    if (!frame_args(config, frame_header, &a, &frames)) return VSRD_E_INVALID_ARGUMENT;
    FrameBuffers b;
    if (!frame_buffers(raw_locations, raw_dimensions, raw_orientations, extrinsics, intrinsics, gt_boxes, visible, step, scratch, instances, pd_indices, gt_indices,
                       target_columns, instance_weights, schedule, projection_losses, grad_raw, &b))
        return VSRD_E_INVALID_ARGUMENT;
    if (!scratch || scratch_bytes < vsrd_frame_scratch_bytes(a.num_views, a.num_boxes)) return VSRD_E_WORKSPACE;
    hipLaunchKernelGGL(frame_prologue_kernel, dim3(1, frames.count), dim3(kFrameThreads), 0, static_cast<hipStream_t>(stream), a, b);
    return launch_status();
}

int32_t vsrd_frame_prologue_sample(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                                   const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                                   const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                                   float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                                   float* schedule, float* projection_losses, float* grad_raw,
                                   void* ray_table, int64_t count, int32_t num_rays, uint64_t seed, const int64_t* remap, int64_t* ray_indices, void* stream) {
    return vsrd_frame_prologue_sample_with_header(config, raw_locations, raw_dimensions, raw_orientations, extrinsics, intrinsics, gt_boxes, visible, step,
                                                  scratch, scratch_bytes, instances, pd_indices, gt_indices, target_columns, instance_weights, schedule,
                                                  projection_losses, grad_raw, ray_table, count, num_rays, seed, remap, ray_indices, nullptr, stream);
}

int32_t vsrd_frame_prologue_sample_with_header(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions,
                                               const float* raw_orientations, const float* extrinsics, const float* intrinsics, const float* gt_boxes,
                                               const uint8_t* visible, const int64_t* step, void* scratch, size_t scratch_bytes,
                                               float* instances, int64_t* pd_indices, int64_t* gt_indices, int32_t* target_columns, float* instance_weights,
                                               float* schedule, float* projection_losses, float* grad_raw,
                                               void* ray_table, int64_t count, int32_t num_rays, uint64_t seed, const int64_t* remap, int64_t* ray_indices,
                                               const vsrd_frame_header* frame_header, void* stream) {
    FrameStepArgs a;
    Frames frames;
    if (!frame_args(config, frame_header, &a, &frames)) return VSRD_E_INVALID_ARGUMENT;
    FrameBuffers b;
    if (!frame_buffers(raw_locations, raw_dimensions, raw_orientations, extrinsics, intrinsics, gt_boxes, visible, step, scratch, instances, pd_indices, gt_indices,
                       target_columns, instance_weights, schedule, projection_losses, grad_raw, &b))
        return VSRD_E_INVALID_ARGUMENT;
    if (!ray_table || !ray_indices || count < 1 || count >= 0xffffffffll || num_rays < 1 || num_rays > kSampleMax) return VSRD_E_INVALID_ARGUMENT;
    if (!scratch || scratch_bytes < vsrd_frame_scratch_bytes(a.num_views, a.num_boxes)) return VSRD_E_WORKSPACE;
    // (a refused LDS opt-in is "this device / build cannot run the combined launch" -- VSRD_E_UNSUPPORTED, on which the caller falls back to
    //  vsrd_frame_prologue + vsrd_sample_rays_table -- and not a failed launch, which must not be mistaken for it)
    if (opt_in_lds(frame_prologue_sample_kernel, kTableLdsBytes) != VSRD_OK) return VSRD_E_UNSUPPORTED;
    hipLaunchKernelGGL(frame_prologue_sample_kernel, dim3(2, frames.count), dim3(kTableThreads), kTableLdsBytes, static_cast<hipStream_t>(stream), a, b,
                       static_cast<RayTableHeader*>(ray_table), static_cast<long long>(count), num_rays, seed, reinterpret_cast<const unsigned long long*>(step),
                       reinterpret_cast<const long long*>(remap), reinterpret_cast<long long*>(ray_indices));
    return launch_status();
}

int32_t vsrd_frame_epilogue(const vsrd_frame_config* config, const float* grad_instances, const float* grad_raw_projection,
                            const float* projection_losses, const float* render_losses, float eikonal_ratio,
                            const vsrd_adam_tensors* locations, const vsrd_adam_tensors* dimensions, const vsrd_adam_tensors* orientations,
                            float* other_learning_rate_0, float* other_learning_rate_1, int64_t* step,
                            float* record, float* raw_gradients, void* stream) {
    return vsrd_frame_epilogue_with_header(config, grad_instances, grad_raw_projection, projection_losses, render_losses, eikonal_ratio, locations, dimensions,
                                           orientations, other_learning_rate_0, other_learning_rate_1, step, record, raw_gradients, nullptr, stream);
}

int32_t vsrd_frame_epilogue_with_header(const vsrd_frame_config* config, const float* grad_instances, const float* grad_raw_projection,
                                        const float* projection_losses, const float* render_losses, float eikonal_ratio,
                                        const vsrd_adam_tensors* locations, const vsrd_adam_tensors* dimensions, const vsrd_adam_tensors* orientations,
                                        float* other_learning_rate_0, float* other_learning_rate_1, int64_t* step,
                                        float* record, float* raw_gradients, const vsrd_frame_header* frame_header, void* stream) {
    FrameStepArgs a;
    Frames frames;
    if (!frame_args(config, frame_header, &a, &frames)) return VSRD_E_INVALID_ARGUMENT;
    if (!grad_instances || !grad_raw_projection || !projection_losses || !render_losses || !locations || !dimensions || !orientations || !step || !record)
        return VSRD_E_INVALID_ARGUMENT;
    if (!valid_adam(*locations) || !valid_adam(*dimensions) || !valid_adam(*orientations)) return VSRD_E_INVALID_ARGUMENT;
    EpilogueBuffers e;
    e.grad_instances = grad_instances; e.grad_raw_projection = grad_raw_projection; e.projection_losses = projection_losses;
    e.render_losses = render_losses; e.eikonal_ratio = eikonal_ratio;
    e.locations = adam_tensors(*locations); e.dimensions = adam_tensors(*dimensions); e.orientations = adam_tensors(*orientations);
    e.other_learning_rates[0] = other_learning_rate_0; e.other_learning_rates[1] = other_learning_rate_1;
    e.step = reinterpret_cast<long long*>(step); e.record = record; e.raw_gradients = raw_gradients;
    hipLaunchKernelGGL(frame_epilogue_kernel, dim3(1, frames.count), dim3(kFrameMaxBoxes), 0, static_cast<hipStream_t>(stream), a, e);
    return launch_status();
}

int32_t vsrd_frame_labels(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                          const float* extrinsics, const float* intrinsics, const float* gt_boxes, const uint8_t* visible,
                          float* camera_corners, float* boxes_2d, float* mean_iou, int64_t* matched_gt, float* confidences,
                          const vsrd_frame_header* frame_header, void* stream) {
    FrameStepArgs a;                       // (the schedules, loss weights and Adam's constants are not read: num_steps is not checked)
    Frames frames;
    if (!frame_shape(config, frame_header, &a, &frames) || !valid_views(config)) return VSRD_E_INVALID_ARGUMENT;
    if (!raw_locations || !raw_dimensions || !raw_orientations || !extrinsics || !intrinsics || !gt_boxes || !visible) return VSRD_E_INVALID_ARGUMENT;
    LabelBuffers b;
    b.raw_locations = raw_locations; b.raw_dimensions = raw_dimensions; b.raw_orientations = raw_orientations;
    b.extrinsics = extrinsics; b.intrinsics = intrinsics; b.gt_boxes = gt_boxes; b.visible = visible;
    b.camera_corners = camera_corners; b.boxes_2d = boxes_2d; b.mean_iou = mean_iou;
    b.matched_gt = reinterpret_cast<long long*>(matched_gt); b.confidences = confidences;
    hipLaunchKernelGGL(frame_labels_kernel, dim3(frames.count), dim3(kFrameThreads), 0, static_cast<hipStream_t>(stream), a, b);
    return launch_status();
}

int32_t vsrd_frame_group_labels(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                                int32_t num_label_views, const int32_t* label_view_count, const float* label_extrinsics, const float* label_intrinsics,
                                const float* label_gt_boxes, const uint8_t* label_visible, float* camera_corners, float* boxes_2d, float* mean_iou,
                                int64_t* matched_gt, float* confidences, const vsrd_frame_header* frame_header, void* stream) {
    static_assert(kGroupMaxViews == VSRD_MAX_LABEL_VIEWS, "frame_group_labels.h and the ABI agree on the label-view capacity");
    FrameStepArgs a;                       // (num_views is not read, and not checked: the label views are the call's own)
    Frames frames;
    if (!frame_shape(config, frame_header, &a, &frames) || num_label_views < 1 || num_label_views > kGroupMaxViews) return VSRD_E_INVALID_ARGUMENT;
    if (!raw_locations || !raw_dimensions || !raw_orientations || !label_extrinsics || !label_intrinsics || !label_gt_boxes || !label_visible ||
        !boxes_2d || !mean_iou)
        return VSRD_E_INVALID_ARGUMENT;
    GroupLabelBuffers b;
    b.raw_locations = raw_locations; b.raw_dimensions = raw_dimensions; b.raw_orientations = raw_orientations;
    b.view_count = label_view_count; b.extrinsics = label_extrinsics; b.intrinsics = label_intrinsics; b.gt_boxes = label_gt_boxes; b.visible = label_visible;
    b.camera_corners = camera_corners; b.boxes_2d = boxes_2d; b.mean_iou = mean_iou;
    b.matched_gt = reinterpret_cast<long long*>(matched_gt); b.confidences = confidences;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = num_label_views, N = config->num_boxes;
    hipLaunchKernelGGL(frame_group_project_kernel, dim3((L + kGroupWaves - 1) / kGroupWaves, frames.count), dim3(kGroupThreads), 0, s, a, b, L);
    hipLaunchKernelGGL(frame_group_mean_iou_kernel, dim3((N + kGroupWaves - 1) / kGroupWaves, frames.count), dim3(kGroupThreads), 0, s, a, b, L);
    if (matched_gt || confidences) hipLaunchKernelGGL(frame_group_assign_kernel, dim3(frames.count), dim3(kWave), 0, s, a, b);
    return launch_status();
}

int32_t vsrd_frame_masks(const vsrd_field* field, const vsrd_render_config* config, const vsrd_frame_masks_config* masks,
                         const float* camera_positions, const float* ray_directions, const float* u_coarse, const float* u_fine,
                         const float* targets, const int32_t* target_columns, uint8_t* mask_bits, float* soft, int32_t* counts,
                         const vsrd_frame_header* frame_header, void* stream) {
    if (!valid_field(field) || !config || !masks || !camera_positions || !ray_directions || !mask_bits) return VSRD_E_INVALID_ARGUMENT;
    vsrd_render_config own = *config;
    own.num_rays = 0;                                            // (ignored: the ray count is H W)
    if (!valid_config(&own)) return VSRD_E_INVALID_ARGUMENT;     // (rejects ray_indices, target_columns and out_* inside the config)
    const int32_t image = image_view_status(masks->num_views, masks->view, masks->height, masks->width, masks->num_iterations);
    if (image == VSRD_E_INVALID_ARGUMENT) return VSRD_E_INVALID_ARGUMENT;
    if ((targets != nullptr) != (counts != nullptr)) return VSRD_E_INVALID_ARGUMENT;
    const int N = field->num_instances, S = config->num_samples;
    if (targets != nullptr && masks->target_stride < (target_columns ? 1 : N)) return VSRD_E_INVALID_ARGUMENT;
    const bool residual = field->mlp_weights != nullptr;
    const int rounds = rounds_for(2 * S - 1);
    if (rounds == 0 || (residual && rounds > 4)) return VSRD_E_INVALID_ARGUMENT;
    if (image != VSRD_OK) return image;
    Frames frames;
    if (!frames_of(config->num_frames, config->frame_stride, &frames)) return VSRD_E_INVALID_ARGUMENT;
    static_assert(kRunPixels == kWave, "a run is one wave's pixels");
    Geometry g;
    if (!plan(image_runs(masks->height, masks->width), static_cast<size_t>(hierarchical_lds_floats(S, N, residual)), &g)) return VSRD_E_UNSUPPORTED;
    const FieldArgs f = field_args(field);
    RenderArgs c = render_args(config);
    c.sh.inv_t = f.inv_t;
    c.frame_stride = frames.stride;
    MaskArgs m;
    m.view = masks->view; m.height = masks->height; m.width = masks->width; m.num_iterations = masks->num_iterations;
    m.criteria = masks->convergence_criteria; m.bounding_radius = masks->bounding_radius; m.threshold = masks->threshold;
    m.target_stride = masks->target_stride;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const FrameHeader* header = reinterpret_cast<const FrameHeader*>(frame_header);
    int32_t status = VSRD_OK;
    auto launch = [&](auto k, auto res) {
        constexpr auto kernel = frame_masks_kernel<decltype(k)::value, decltype(res)::value>;
        if ((status = opt_in_lds(kernel, g.lds_bytes)) != VSRD_OK) return;
        if (counts != nullptr) hipLaunchKernelGGL(frame_masks_clear_kernel, dim3(frames.count), dim3(256), 0, s, counts, N, frames.stride, header);
        hipLaunchKernelGGL(kernel, dim3(g.blocks, frames.count), dim3(g.threads), g.lds_bytes, s, f, field->instances, field->mlp_weights, c, m, camera_positions,
                           ray_directions, u_coarse, u_fine, targets, target_columns, mask_bits, soft, counts, header);
    };
    if (residual) for_rounds<1, 2, 4>(rounds, [&](auto k) { launch(k, std::true_type{}); });
    else for_rounds<1, 2, 4, 8>(rounds, [&](auto k) { launch(k, std::false_type{}); });
    if (status != VSRD_OK) return status;
    return launch_status();
}

int32_t vsrd_frame_metrics(const vsrd_frame_config* config, const float* raw_locations, const float* raw_dimensions, const float* raw_orientations,
                           const float* gt_boxes_3d, const float* rectification, const int64_t* pd_indices, const int64_t* gt_indices,
                           float* corners, float* ious, float* summary, const vsrd_frame_header* frame_header, void* stream) {
    FrameStepArgs a;                       // (of it the kernel reads the box count, the decode's ranges and the batch fields: nothing else is checked)
    Frames frames;
    if (!frame_shape(config, frame_header, &a, &frames)) return VSRD_E_INVALID_ARGUMENT;
    if (!raw_locations || !raw_dimensions || !raw_orientations || !gt_boxes_3d || !ious || !summary) return VSRD_E_INVALID_ARGUMENT;
    if ((pd_indices != nullptr) != (gt_indices != nullptr)) return VSRD_E_INVALID_ARGUMENT;
    MetricBuffers b;
    b.raw_locations = raw_locations; b.raw_dimensions = raw_dimensions; b.raw_orientations = raw_orientations;
    b.gt_boxes_3d = gt_boxes_3d; b.rectification = rectification;
    b.pd_indices = reinterpret_cast<const long long*>(pd_indices); b.gt_indices = reinterpret_cast<const long long*>(gt_indices);
    b.corners = corners; b.ious = ious; b.summary = summary;
    hipLaunchKernelGGL(frame_metrics_kernel, dim3(frames.count), dim3(kWave), 0, static_cast<hipStream_t>(stream), a, b);
    return launch_status();
}

int32_t vsrd_frame_log(const vsrd_frame_log_config* log, void* stream) {
    static_assert(kLogScalars == VSRD_LOG_SCALARS && kLogMaxSegments == VSRD_LOG_MAX_SEGMENTS, "frame_log.h and the ABI agree on the row and the table");
    static_assert(sizeof(LogSegment) == sizeof(vsrd_log_segment), "frame_log.h and the ABI agree on a table entry");
    Frames frames;
    if (!log || log->scalar_interval < 0 || log->checkpoint_interval < 0 || log->history_capacity < 0 || log->snapshot_capacity < 0 ||
        !frames_of(log->num_frames, log->frame_stride, &frames))
        return VSRD_E_INVALID_ARGUMENT;
    if (!log->step || !log->counters) return VSRD_E_INVALID_ARGUMENT;
    if (log->scalar_interval > 0 && (!log->record || !log->learning_rates || !log->schedule || !log->history)) return VSRD_E_INVALID_ARGUMENT;
    if (log->checkpoint_interval > 0 &&
        (!log->segments || !log->snapshots || !log->snapshot_steps || log->num_segments < 0 || log->num_segments > kLogMaxSegments ||
         log->snapshot_floats < 0 || (log->snapshot_floats & 3) != 0 || (reinterpret_cast<uintptr_t>(log->snapshots) & 15) != 0))
        return VSRD_E_INVALID_ARGUMENT;
    if (log->scalar_interval == 0 && log->checkpoint_interval == 0) return VSRD_OK;
    LogArgs a;
    a.scalar_interval = log->scalar_interval; a.checkpoint_interval = log->checkpoint_interval;
    a.history_capacity = log->history_capacity; a.snapshot_capacity = log->snapshot_capacity;
    a.snapshot_floats = log->snapshot_floats; a.num_segments = log->num_segments; a.frame_stride = frames.stride;
    a.step = reinterpret_cast<const long long*>(log->step);
    a.record = reinterpret_cast<const unsigned*>(log->record);
    a.learning_rates = static_cast<const unsigned* const*>(log->learning_rates);
    a.schedule = reinterpret_cast<const unsigned*>(log->schedule); a.summary = reinterpret_cast<const unsigned*>(log->summary);
    a.segments = reinterpret_cast<const LogSegment*>(log->segments);
    a.history = reinterpret_cast<unsigned*>(log->history); a.snapshots = reinterpret_cast<unsigned*>(log->snapshots);
    a.snapshot_steps = log->snapshot_steps; a.counters = log->counters;
    // one block without snapshots; with them a block per 256 16-byte accesses of a slot, at most kLogMaxBlocks per frame (grid-stride beyond)
    long long blocks = 1;
    if (log->checkpoint_interval > 0) blocks = (log->snapshot_floats / 4 + kLogThreads - 1) / kLogThreads;
    blocks = blocks < 1 ? 1 : (blocks > kLogMaxBlocks ? kLogMaxBlocks : blocks);
    hipLaunchKernelGGL(frame_log_kernel, dim3(static_cast<unsigned>(blocks), frames.count), dim3(kLogThreads), 0, static_cast<hipStream_t>(stream), a);
    return launch_status();
}

namespace {
bool valid_patch_shape(int V, int R, int P) {
    return V >= 1 && V <= kPatchMaxViews && R >= 1 && R <= kPatchMaxRays && P >= 1 && P <= kPatchMaxPixels;
}

// What the patch calls and vsrd_frame_photometric refuse of a patch config (each side within the pixel limit before their product is formed).
bool valid_patch_config(const vsrd_patch_correlation_config* c) {
    if (!c || c->patch_width < 1 || c->patch_height < 1 || c->patch_width > kPatchMaxPixels || c->patch_height > kPatchMaxPixels) return false;
    const int V = c->num_views;
    return valid_patch_shape(V, c->num_rays, c->patch_width * c->patch_height) && c->top_k >= 1 && c->top_k <= V && c->target_view >= 0 &&
           c->target_view < V && c->height >= 2 && c->width >= 2 && static_cast<int64_t>(c->height) * c->width < (int64_t{1} << 30);
}

// The patch calls' workspace (patch_correlation.h: PatchArgs; `bytes`: vsrd_patch_correlation_workspace_bytes): the views' constants
// [V,12] + K_t^-1 [9] (padded to 12), then the rays' (sum, count) [R,2].
struct PatchWorkspace {
    float* constants; float* ray_stats;
    size_t bytes;
};
PatchWorkspace patch_workspace(void* workspace, int V, int R) {
    Carver c{static_cast<float*>(workspace)};
    PatchWorkspace w;
    w.constants = c.take(static_cast<size_t>(V + 1) * kPatchViewFloats);
    w.ray_stats = c.take(static_cast<size_t>(R) * 2);
    w.bytes = c.at * sizeof(float);
    return w;
}

// The checks the two calls share, in this order: the shape, the pointers, the workspace.
int32_t patch_args(const vsrd_patch_correlation_config* config, const float* gray, const float* intrinsics, const float* extrinsics, const int32_t* pixels,
                   const float* positions, const float* normals, const uint8_t* converged, void* workspace, size_t workspace_bytes, PatchArgs* a) {
    static_assert(kPatchMaxViews == VSRD_PATCH_MAX_VIEWS && kPatchMaxPixels == VSRD_PATCH_MAX_PIXELS && kPatchMaxRays == VSRD_PATCH_MAX_RAYS,
                  "patch_correlation.h and the ABI agree on the limits");
    if (!valid_patch_config(config)) return VSRD_E_INVALID_ARGUMENT;
    if (!gray || !intrinsics || !extrinsics || !pixels || !positions || !normals || !converged) return VSRD_E_INVALID_ARGUMENT;
    const PatchWorkspace w = patch_workspace(workspace, config->num_views, config->num_rays);
    if (!workspace || workspace_bytes < w.bytes) return VSRD_E_WORKSPACE;
    a->num_views = config->num_views; a->num_rays = config->num_rays; a->height = config->height; a->width = config->width;
    a->patch_width = config->patch_width; a->patch_height = config->patch_height; a->top_k = config->top_k; a->target_view = config->target_view;
    a->sample_epsilon = config->sample_epsilon; a->correlation_epsilon = config->correlation_epsilon;
    a->gray = gray; a->intrinsics = intrinsics; a->extrinsics = extrinsics; a->pixels = pixels; a->positions = positions; a->normals = normals;
    a->converged = converged;
    a->constants = w.constants; a->ray_stats = w.ray_stats;
    a->view_capacity = config->num_views; a->frame_stride = 0; a->header = nullptr;
    return VSRD_OK;
}

// The launches of the two patch calls behind their checks, over a batch of frames (patch_correlation.h: the kFrames kernels, the frame
// along blockIdx.y) or, with one frame and no header, as the launches of before.
int32_t launch_patch_forward(PatchArgs a, float* loss, float* stats, float* patches, float* coefficients, int32_t* selected, const Frames& frames,
                             const FrameHeader* header, hipStream_t s) {
    a.frame_stride = frames.stride; a.header = header;
    for_bool(frames.stride != 0 || header != nullptr, [&](auto batched) {
        constexpr bool kFrames = decltype(batched)::value;
        const unsigned count = kFrames ? frames.count : 1;
        hipLaunchKernelGGL(patch_constants_kernel<kFrames>, dim3(1, count), dim3(kWave), 0, s, a);
        hipLaunchKernelGGL(patch_correlation_forward_kernel<kFrames>, dim3(a.num_rays, count), dim3(kPatchThreads), 0, s, a, patches, coefficients, selected);
        hipLaunchKernelGGL(patch_loss_kernel<kFrames>, dim3(1, count), dim3(kWave), 0, s, a, loss, stats);
    });
    return launch_status();
}

int32_t launch_patch_backward(PatchArgs a, const float* stats, const float* grad_loss, float* grad_positions, float* grad_normals, const Frames& frames,
                              const FrameHeader* header, hipStream_t s) {
    a.frame_stride = frames.stride; a.header = header;
    for_bool(frames.stride != 0 || header != nullptr, [&](auto batched) {
        constexpr bool kFrames = decltype(batched)::value;
        const unsigned count = kFrames ? frames.count : 1;
        hipLaunchKernelGGL(patch_constants_kernel<kFrames>, dim3(1, count), dim3(kWave), 0, s, a);
        hipLaunchKernelGGL(patch_correlation_backward_kernel<kFrames>, dim3(a.num_rays, count), dim3(kPatchThreads), 0, s, a, stats, grad_loss, grad_positions,
                           grad_normals);
    });
    return launch_status();
}
}  // namespace

int32_t vsrd_grayscale_images(const float* images, int32_t num_views, int32_t height, int32_t width, float* gray, void* stream) {
    if (!images || !gray || num_views < 1 || num_views > 65535 || height < 1 || width < 1) return VSRD_E_INVALID_ARGUMENT;
    const long long plane = static_cast<long long>(height) * width;
    if (plane >= (1ll << 30)) return VSRD_E_UNSUPPORTED;
    long long blocks = (plane / 4 + 255) / 256;                  // a thread per 16 bytes of a plane, grid-stride beyond 1024 blocks
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    hipLaunchKernelGGL(patch_gray_kernel, dim3(static_cast<unsigned>(blocks), num_views), dim3(256), 0, static_cast<hipStream_t>(stream), images, gray, plane);
    return launch_status();
}

size_t vsrd_patch_correlation_workspace_bytes(int32_t num_views, int32_t num_rays, int32_t patch_pixels) {
    return valid_patch_shape(num_views, num_rays, patch_pixels) ? patch_workspace(nullptr, num_views, num_rays).bytes : 0;
}

int32_t vsrd_patch_correlation_forward(const vsrd_patch_correlation_config* config, const float* gray, const float* intrinsics, const float* extrinsics,
                                       const int32_t* pixels, const float* positions, const float* normals, const uint8_t* converged,
                                       void* workspace, size_t workspace_bytes, float* loss, float* stats,
                                       float* patches, float* coefficients, int32_t* selected, void* stream) {
    PatchArgs a;
    const int32_t status = patch_args(config, gray, intrinsics, extrinsics, pixels, positions, normals, converged, workspace, workspace_bytes, &a);
    if (status != VSRD_OK) return status;
    if (!loss || !stats) return VSRD_E_INVALID_ARGUMENT;
    return launch_patch_forward(a, loss, stats, patches, coefficients, selected, {1, 0}, nullptr, static_cast<hipStream_t>(stream));
}

int32_t vsrd_patch_correlation_backward(const vsrd_patch_correlation_config* config, const float* gray, const float* intrinsics, const float* extrinsics,
                                        const int32_t* pixels, const float* positions, const float* normals, const uint8_t* converged,
                                        void* workspace, size_t workspace_bytes, const float* stats, const float* grad_loss,
                                        float* grad_positions, float* grad_normals, void* stream) {
    PatchArgs a;
    const int32_t status = patch_args(config, gray, intrinsics, extrinsics, pixels, positions, normals, converged, workspace, workspace_bytes, &a);
    if (status != VSRD_OK) return status;
    if (!stats || !grad_loss || !grad_positions || !grad_normals) return VSRD_E_INVALID_ARGUMENT;
    return launch_patch_backward(a, stats, grad_loss, grad_positions, grad_normals, {1, 0}, nullptr, static_cast<hipStream_t>(stream));
}

namespace {
// The workspace of vsrd_frame_photometric, in floats: the per-ray arrays (each padded to a multiple of 4 rays), the four parameter-gradient
// blocks of the two field adjoints, the patch correlation's workspace, then -- 256-byte aligned -- the field adjoints' own workspace.
struct PhotometricWorkspace {
    float *directions, *p0, *d0, *g0, *slopes, *p1, *g1, *lengths, *normals, *grad_p1, *grad_normals, *gamma, *grad_x, *grad_d0, *one;
    int* pixels;
    unsigned char* converged;
    float *first_instances, *second_instances, *first_mlp, *second_mlp;
    float* patch;
    size_t patch_bytes;
    void* field;
    size_t field_bytes;
    size_t total_bytes;
};
size_t padded4(size_t n) { return (n + 3) & ~static_cast<size_t>(3); }
PhotometricWorkspace photometric_workspace(void* workspace, int N, bool residual, int V, int R) {
    PhotometricWorkspace w;
    Carver c{static_cast<float*>(workspace)};
    const size_t rays = padded4(static_cast<size_t>(R));
    auto take = [&](size_t floats) { return c.take(padded4(floats)); };
    w.directions = take(3 * rays); w.p0 = take(3 * rays); w.d0 = take(rays); w.g0 = take(3 * rays); w.slopes = take(rays);
    w.p1 = take(3 * rays); w.g1 = take(3 * rays); w.lengths = take(rays); w.normals = take(3 * rays);
    w.grad_p1 = take(3 * rays); w.grad_normals = take(3 * rays); w.gamma = take(3 * rays); w.grad_x = take(3 * rays); w.grad_d0 = take(rays);
    w.one = take(4);
    w.pixels = reinterpret_cast<int*>(take(2 * rays));
    w.converged = reinterpret_cast<unsigned char*>(take(rays / 4));
    w.first_instances = take(static_cast<size_t>(N) * kGradStride); w.second_instances = take(static_cast<size_t>(N) * kGradStride);
    w.first_mlp = take(residual ? static_cast<size_t>(N) * kMlpWeights : 0); w.second_mlp = take(residual ? static_cast<size_t>(N) * kMlpWeights : 0);
    w.patch_bytes = patch_workspace(nullptr, V, R).bytes;
    w.patch = take(w.patch_bytes / sizeof(float));
    c.at = (c.at + 63) & ~static_cast<size_t>(63);
    w.field_bytes = vsrd_workspace_bytes(N, residual);
    w.field = c.take(w.field_bytes / sizeof(float));
    w.total_bytes = c.at * sizeof(float);
    return w;
}
}  // namespace

size_t vsrd_frame_photometric_workspace_bytes(int32_t num_instances, int32_t residual, int32_t num_views, int32_t num_rays, int32_t patch_pixels) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES || num_rays > kPhotometricMaxRays || !valid_patch_shape(num_views, num_rays, patch_pixels)) return 0;
    return photometric_workspace(nullptr, num_instances, residual != 0, num_views, num_rays).total_bytes;
}

namespace {
// vsrd_frame_photometric and its _with_header twin: one set of refusals, one sequence of launches.  `batches` false (the first symbol):
// num_frames >= 2 is VSRD_E_UNSUPPORTED.  With one frame and no header every launch is the one-frame launch of before.
int32_t frame_photometric(const vsrd_frame_photometric_config* config, const vsrd_patch_correlation_config* patch, const vsrd_field* field,
                          const float* camera_position, const float* ray_directions, const float* gray, const float* intrinsics,
                          const float* extrinsics, const int64_t* ray_indices, void* workspace, size_t workspace_bytes,
                          float* loss, float* stats, float* photometric_grad_instances, float* photometric_grad_mlp,
                          float* grad_instances, float* grad_mlp, float* positions, float* normals, uint8_t* converged,
                          const FrameHeader* header, bool batches, void* stream) {
    static_assert(kPhotometricMaxRays == VSRD_PHOTOMETRIC_MAX_RAYS, "frame_photometric.h and the ABI agree on the limit");
    Frames frames;
    if (!config || !frames_of(config->num_frames, config->frame_stride, &frames)) return VSRD_E_INVALID_ARGUMENT;
    if (frames.count > 1 && !batches) return VSRD_E_UNSUPPORTED;
    if (!patch || !valid_field(field) || config->num_iterations < 0) return VSRD_E_INVALID_ARGUMENT;
    const int N = field->num_instances, V = patch->num_views, R = patch->num_rays;
    const bool residual = field->mlp_weights != nullptr;
    if (R > kPhotometricMaxRays || !valid_patch_config(patch)) return VSRD_E_INVALID_ARGUMENT;
    if (!camera_position || !ray_directions || !gray || !intrinsics || !extrinsics || !ray_indices || !loss || !stats || !photometric_grad_instances ||
        !grad_instances || (residual && (!photometric_grad_mlp || !grad_mlp)))
        return VSRD_E_INVALID_ARGUMENT;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return workspace ? VSRD_E_INVALID_ARGUMENT : VSRD_E_WORKSPACE;
    PhotometricWorkspace w = photometric_workspace(workspace, N, residual, V, R);
    if (workspace_bytes < w.total_bytes) return VSRD_E_WORKSPACE;
    if (positions) w.p1 = positions;
    if (normals) w.normals = normals;
    if (converged) w.converged = converged;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((R + kPhotometricThreads - 1) / kPhotometricThreads, frames.count), block(kPhotometricThreads);
    PatchArgs a;
    int32_t status = patch_args(patch, gray, intrinsics, extrinsics, w.pixels, w.p1, w.normals, w.converged, w.patch, w.patch_bytes, &a);
    if (status != VSRD_OK) return status;
    hipLaunchKernelGGL(photometric_gather_kernel, grid, block, 0, s, R, patch->width, reinterpret_cast<const long long*>(ray_indices), ray_directions,
                       w.directions, w.pixels, w.one, frames.stride);
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    status = launch_sphere_trace(field, camera_position, 0, w.directions, nullptr, R, config->num_iterations, config->convergence_criteria,
                                 config->bounding_radius, 0, 1, w.p0, w.converged, frames, header, s);
    if (status != VSRD_OK) return status;
    status = launch_field_eval(field, w.p0, R, w.d0, w.g0, nullptr, 1, frames, header, s);
    if (status != VSRD_OK) return status;
    hipLaunchKernelGGL(photometric_newton_kernel, grid, block, 0, s, R, w.p0, w.converged, w.d0, w.g0, w.directions, w.p1, w.slopes, frames.stride);
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    status = launch_field_eval(field, w.p1, R, nullptr, w.g1, nullptr, 1, frames, header, s);
    if (status != VSRD_OK) return status;
    hipLaunchKernelGGL(photometric_normalise_kernel, grid, block, 0, s, R, w.g1, w.normals, w.lengths, frames.stride);
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    status = launch_patch_forward(a, loss, stats, nullptr, nullptr, nullptr, frames, header, s);
    if (status != VSRD_OK) return status;
    status = launch_patch_backward(a, stats, w.one, w.grad_p1, w.grad_normals, frames, header, s);
    if (status != VSRD_OK) return status;
    hipLaunchKernelGGL(photometric_normal_adjoint_kernel, grid, block, 0, s, R, w.converged, w.normals, w.lengths, w.grad_normals, w.gamma, frames.stride);
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    status = field_eval_adjoint(field, w.p1, R, nullptr, nullptr, w.gamma, 1, w.field, w.field_bytes, w.grad_x, w.first_instances,
                                residual ? w.first_mlp : nullptr, stream, frames, header);
    if (status != VSRD_OK) return status;
    hipLaunchKernelGGL(photometric_newton_adjoint_kernel, grid, block, 0, s, R, w.converged, w.grad_p1, w.grad_x, w.directions, w.slopes, w.grad_d0,
                       frames.stride);
    if (launch_status() != VSRD_OK) return VSRD_E_LAUNCH;
    status = field_eval_adjoint(field, w.p0, R, w.grad_d0, nullptr, nullptr, 1, w.field, w.field_bytes, nullptr, w.second_instances,
                                residual ? w.second_mlp : nullptr, stream, frames, header);
    if (status != VSRD_OK) return status;
    const int count_instances = N * kGradStride, count_mlp = residual ? N * kMlpWeights : 0;
    const int blocks = std::min((count_instances + count_mlp + kPhotometricThreads - 1) / kPhotometricThreads, 1024);
    hipLaunchKernelGGL(photometric_accumulate_kernel, dim3(blocks, frames.count), block, 0, s, stats, config->scale, count_instances, count_mlp, w.first_instances,
                       w.second_instances, w.first_mlp, w.second_mlp, photometric_grad_instances, photometric_grad_mlp, grad_instances, grad_mlp, N,
                       frames.stride, header);
    return launch_status();
}
}  // namespace

int32_t vsrd_frame_photometric(const vsrd_frame_photometric_config* config, const vsrd_patch_correlation_config* patch, const vsrd_field* field,
                               const float* camera_position, const float* ray_directions, const float* gray, const float* intrinsics,
                               const float* extrinsics, const int64_t* ray_indices, void* workspace, size_t workspace_bytes,
                               float* loss, float* stats, float* photometric_grad_instances, float* photometric_grad_mlp,
                               float* grad_instances, float* grad_mlp, float* positions, float* normals, uint8_t* converged, void* stream) {
    return frame_photometric(config, patch, field, camera_position, ray_directions, gray, intrinsics, extrinsics, ray_indices, workspace, workspace_bytes,
                             loss, stats, photometric_grad_instances, photometric_grad_mlp, grad_instances, grad_mlp, positions, normals, converged,
                             nullptr, false, stream);
}

int32_t vsrd_frame_photometric_with_header(const vsrd_frame_photometric_config* config, const vsrd_patch_correlation_config* patch, const vsrd_field* field,
                                           const float* camera_position, const float* ray_directions, const float* gray, const float* intrinsics,
                                           const float* extrinsics, const int64_t* ray_indices, void* workspace, size_t workspace_bytes,
                                           float* loss, float* stats, float* photometric_grad_instances, float* photometric_grad_mlp,
                                           float* grad_instances, float* grad_mlp, float* positions, float* normals, uint8_t* converged,
                                           const vsrd_frame_header* frame_header, void* stream) {
    return frame_photometric(config, patch, field, camera_position, ray_directions, gray, intrinsics, extrinsics, ray_indices, workspace, workspace_bytes,
                             loss, stats, photometric_grad_instances, photometric_grad_mlp, grad_instances, grad_mlp, positions, normals, converged,
                             reinterpret_cast<const FrameHeader*>(frame_header), true, stream);
}

int32_t vsrd_frame_photometric_finish(const float* loss, const float* stats, float weight, float* record, void* stream) {
    if (!loss || !stats || !record) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(photometric_finish_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), loss, stats, weight, record, 0ll);
    return launch_status();
}

int32_t vsrd_frame_photometric_finish_with_header(const float* loss, const float* stats, float weight, float* record, int32_t num_frames,
                                                  int64_t frame_stride, void* stream) {
    Frames frames;
    if (!loss || !stats || !record || !frames_of(num_frames, frame_stride, &frames)) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(photometric_finish_kernel, dim3(1, frames.count), dim3(kWave), 0, static_cast<hipStream_t>(stream), loss, stats, weight, record,
                       frames.stride);
    return launch_status();
}

// (vsrd_box_decode_forward / _backward: box_decode.hip, a translation unit of its own for its floating-point contraction mode)

namespace {
struct HyperPlan {
    size_t activations;        // float offset of z[l] = activations + l * N * 256, l < 4
    size_t inv_norm;           // 4 x 256 + 1632
    size_t gz;                 // 5 x N x 256: the output adjoints of the four hidden linears, then the embeddings' gradient
    size_t partials;           // final_blocks x N x 256
    size_t norm_partials;      // 4 x N x 2 x 256
    size_t total;
    int final_blocks;
};
static HyperPlan plan_hypernetwork(int num_instances) {
    const size_t slab = static_cast<size_t>(num_instances) * kHyperWidth;
    HyperPlan p;
    p.final_blocks = (kMlpWeights + kHyperWaves - 1) / kHyperWaves;
    p.activations = 0;
    p.inv_norm = p.activations + (VSRD_HYPER_LAYERS - 1) * slab;
    p.gz = p.inv_norm + (VSRD_HYPER_LAYERS - 1) * kHyperWidth + kMlpWbarFloats;
    p.partials = p.gz + (VSRD_HYPER_LAYERS) * slab;
    p.norm_partials = p.partials + static_cast<size_t>(p.final_blocks) * slab;
    p.total = p.norm_partials + (VSRD_HYPER_LAYERS - 1) * 2 * slab;
    return p;
}
static bool valid_hypernetwork(const vsrd_hypernetwork* net) {
    if (!net || net->num_instances < 1 || net->num_instances > VSRD_MAX_INSTANCES || net->num_outputs != kMlpWeights) return false;
    if (!valid_adam(net->embeddings)) return false;
    for (int l = 0; l < VSRD_HYPER_LAYERS; ++l) {
        if (!valid_adam(net->weight_v[l]) || !valid_adam(net->weight_g[l]) || !valid_adam(net->bias[l])) return false;
        if (l + 1 < VSRD_HYPER_LAYERS && (!valid_adam(net->norm_weight[l]) || !valid_adam(net->norm_bias[l]))) return false;
    }
    return true;
}
}  // namespace

size_t vsrd_hypernetwork_workspace_bytes(int32_t num_instances) {
    if (num_instances < 1 || num_instances > VSRD_MAX_INSTANCES) return 0;
    return plan_hypernetwork(num_instances).total * sizeof(float);
}

int32_t vsrd_hypernetwork_forward(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                  float* mlp_weights, float* centred, void* stream) {
    return vsrd_hypernetwork_forward_with_header(net, workspace, workspace_bytes, mlp_weights, centred, nullptr, stream);
}

int32_t vsrd_hypernetwork_forward_with_header(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                              float* mlp_weights, float* centred, const vsrd_frame_header* frame_header, void* stream) {
    if (!valid_hypernetwork(net) || !mlp_weights) return VSRD_E_INVALID_ARGUMENT;
    const FrameHeader* header = reinterpret_cast<const FrameHeader*>(frame_header);
    Frames frames;
    if (!frames_of(net->num_frames, net->frame_stride, &frames)) return VSRD_E_INVALID_ARGUMENT;
    const int N = net->num_instances;
    const HyperPlan p = plan_hypernetwork(N);
    if (!workspace || workspace_bytes < p.total * sizeof(float)) return VSRD_E_WORKSPACE;
    float* ws = static_cast<float*>(workspace);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t slab = static_cast<size_t>(N) * kHyperWidth, lds = slab * sizeof(float);
    if (opt_in_lds(hyper_linear_forward_kernel, lds) != VSRD_OK) return VSRD_E_LAUNCH;
    constexpr int kLast = VSRD_HYPER_LAYERS - 1;
    static_assert(kLast == kHyperHidden, "csrc/hypernetwork.h is written for four hidden blocks");
    HyperHiddenForward hidden;
    for (int l = 0; l < kLast; ++l) {
        hidden.v[l] = net->weight_v[l].parameter; hidden.g[l] = net->weight_g[l].parameter; hidden.b[l] = net->bias[l].parameter;
        hidden.z[l] = ws + p.activations + l * slab;
        hidden.inv_norm[l] = ws + p.inv_norm + l * kHyperWidth;
        if (l + 1 < kLast) { hidden.gamma[l] = net->norm_weight[l].parameter; hidden.beta[l] = net->norm_bias[l].parameter; }
    }
    hipLaunchKernelGGL(hyper_hidden_forward_kernel, dim3(N, frames.count), dim3(kHyperChainThreads), 0, s, net->embeddings.parameter, hidden, frames.stride, header);
    hipLaunchKernelGGL(hyper_linear_forward_kernel, dim3((kMlpWeights + kHyperWaves - 1) / kHyperWaves, frames.count), dim3(kHyperThreads), lds, s,
                       ws + p.activations + (kLast - 1) * slab, net->norm_weight[kLast - 1].parameter, net->norm_bias[kLast - 1].parameter,
                       net->weight_v[kLast].parameter, net->weight_g[kLast].parameter, net->bias[kLast].parameter, kMlpWeights, N, mlp_weights,
                       ws + p.inv_norm + kLast * kHyperWidth, frames.stride, header);
    if (centred) hipLaunchKernelGGL(hyper_centre_kernel, dim3(N, frames.count), dim3(128), 0, s, mlp_weights, N, centred, frames.stride, header);
    return launch_status();
}

int32_t vsrd_centre_mlp_weights(const float* mlp_weights, int32_t num_instances, float* centred, void* stream) {
    if (!mlp_weights || !centred || num_instances < 1 || num_instances > VSRD_MAX_INSTANCES) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(hyper_centre_kernel, dim3(num_instances), dim3(128), 0, static_cast<hipStream_t>(stream), mlp_weights, num_instances, centred, 0ll, nullptr);
    return launch_status();
}

int32_t vsrd_hypernetwork_backward_step(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                        const float* grad_mlp_weights, float grad_scale, void* stream) {
    return vsrd_hypernetwork_backward_step_with_header(net, workspace, workspace_bytes, grad_mlp_weights, grad_scale, nullptr, stream);
}

int32_t vsrd_hypernetwork_backward_step_with_header(const vsrd_hypernetwork* net, void* workspace, size_t workspace_bytes,
                                                    const float* grad_mlp_weights, float grad_scale, const vsrd_frame_header* frame_header, void* stream) {
    if (!valid_hypernetwork(net) || !grad_mlp_weights) return VSRD_E_INVALID_ARGUMENT;
    const FrameHeader* header = reinterpret_cast<const FrameHeader*>(frame_header);
    Frames frames;
    if (!frames_of(net->num_frames, net->frame_stride, &frames)) return VSRD_E_INVALID_ARGUMENT;
    const int N = net->num_instances;
    const HyperPlan p = plan_hypernetwork(N);
    if (!workspace || workspace_bytes < p.total * sizeof(float)) return VSRD_E_WORKSPACE;
    float* ws = static_cast<float*>(workspace);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t slab = static_cast<size_t>(N) * kHyperWidth, lds = (slab + kHyperWaves * kHyperWidth + static_cast<size_t>(N) * kHyperWaves) * sizeof(float);
    if (opt_in_lds(hyper_linear_backward_kernel, lds) != VSRD_OK || opt_in_lds(hyper_hidden_update_kernel, lds) != VSRD_OK) return VSRD_E_LAUNCH;
    constexpr int kLast = VSRD_HYPER_LAYERS - 1;
    const HyperAdam adam{net->beta1, net->beta2, net->adam_epsilon};
    auto z = [&](int l) { return ws + p.activations + l * slab; };              // output of linear l (l < 4)
    auto gz = [&](int l) { return ws + p.gz + l * slab; };                       // its adjoint; gz(4): the embeddings' gradient
    auto inv_norm = [&](int l) { return ws + p.inv_norm + l * kHyperWidth; };
    auto norm_shares = [&](int k) { return ws + p.norm_partials + k * 2 * slab; };
    // the final linear: its own update and its workgroups' shares of the input adjoint; their sum through the norm behind linear 3
    const int final_blocks = (kMlpWeights + kHyperWaves - 1) / kHyperWaves;
    hipLaunchKernelGGL(hyper_linear_backward_kernel, dim3(final_blocks, frames.count), dim3(kHyperThreads), lds, s, z(kLast - 1), net->norm_weight[kLast - 1].parameter,
                       net->norm_bias[kLast - 1].parameter, grad_mlp_weights, grad_scale, inv_norm(kLast), kMlpWeights, N, adam_tensors(net->weight_v[kLast]),
                       adam_tensors(net->weight_g[kLast]), adam_tensors(net->bias[kLast]), adam, ws + p.partials, frames.stride, header);
    hipLaunchKernelGGL(hyper_norm_backward_kernel, dim3(N, frames.count), dim3(kHyperNormThreads * kHyperNormSplit), 0, s, ws + p.partials, final_blocks, z(kLast - 1), N,
                       net->norm_weight[kLast - 1].parameter, net->norm_bias[kLast - 1].parameter, gz(kLast - 1), norm_shares(kLast - 1), frames.stride, header);
    // the chain through the hidden blocks (one workgroup per instance), then every hidden linear's own update
    HyperHiddenBackward chain;
    HyperHiddenUpdate update;
    HyperNorms norms;
    HyperStepCounters counters;
    counters.count = 0;
    counters.step[counters.count++] = net->embeddings.step;
    for (int l = 0; l < VSRD_HYPER_LAYERS; ++l) {
        counters.step[counters.count++] = net->weight_v[l].step;
        counters.step[counters.count++] = net->weight_g[l].step;
        counters.step[counters.count++] = net->bias[l].step;
        if (l == kLast) break;
        counters.step[counters.count++] = net->norm_weight[l].step;
        counters.step[counters.count++] = net->norm_bias[l].step;
        norms.gamma[l] = adam_tensors(net->norm_weight[l]);
        norms.beta[l] = adam_tensors(net->norm_bias[l]);
        chain.v[l] = net->weight_v[l].parameter; chain.g[l] = net->weight_g[l].parameter; chain.inv_norm[l] = inv_norm(l);
        chain.gz[l] = gz(l);
        if (l + 1 < kLast) { chain.gamma[l] = net->norm_weight[l].parameter; chain.beta[l] = net->norm_bias[l].parameter; chain.z[l] = z(l); chain.norm_partials[l] = norm_shares(l); }
        update.x[l] = l == 0 ? net->embeddings.parameter : z(l - 1);
        update.gamma[l] = l == 0 ? nullptr : net->norm_weight[l - 1].parameter;
        update.beta[l] = l == 0 ? nullptr : net->norm_bias[l - 1].parameter;
        update.gz[l] = gz(l); update.inv_norm[l] = inv_norm(l);
        update.v[l] = adam_tensors(net->weight_v[l]); update.g[l] = adam_tensors(net->weight_g[l]); update.b[l] = adam_tensors(net->bias[l]);
    }
    chain.embedding_bar = gz(kLast);
    hipLaunchKernelGGL(hyper_hidden_backward_kernel, dim3(N, frames.count), dim3(kHyperChainThreads), 0, s, chain, frames.stride, header);
    hipLaunchKernelGGL(hyper_hidden_update_kernel, dim3(kHyperHidden * (kHyperWidth / kHyperWaves), frames.count), dim3(kHyperThreads), lds, s, update, N, adam, frames.stride, header);
    hipLaunchKernelGGL(hyper_finish_kernel, dim3(1, frames.count), dim3(kHyperChainThreads), 0, s, norms, ws + p.norm_partials, adam_tensors(net->embeddings), gz(kLast), N, adam,
                       counters, net->embeddings.learning_rate, net->weight_v[0].learning_rate, net->lr_gamma, frames.stride, header);
    return launch_status();
}

size_t vsrd_sample_rays_workspace_bytes(void) { return sizeof(SampleScratch); }

int32_t vsrd_sample_rays(const float* weights, int64_t count, int32_t num_samples, uint64_t seed, uint64_t stream_offset,
                         const uint64_t* device_stream_offset, void* workspace, size_t workspace_bytes, int64_t* indices, void* stream) {
    if (!weights || !workspace || !indices || count < 1 || num_samples < 1 || num_samples > kSampleMax) return VSRD_E_INVALID_ARGUMENT;
    if (workspace_bytes < sizeof(SampleScratch)) return VSRD_E_WORKSPACE;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    SampleScratch* scratch = static_cast<SampleScratch*>(workspace);
    const unsigned long long* device_step = reinterpret_cast<const unsigned long long*>(device_stream_offset);
    const long long want = (count + 255) / 256;
    const int blocks = static_cast<int>(want > 4096 ? 4096 : want);
    hipLaunchKernelGGL(sample_clear_kernel, dim3(1), dim3(256), 0, s, scratch);
    // every workgroup ends with one global atomic per occupied bin (~100): few, fat workgroups keep that tail short
    hipLaunchKernelGGL(keys_histogram_kernel, dim3(blocks > 512 ? 512 : blocks), dim3(256), 0, s, weights, static_cast<long long>(count), seed, stream_offset, device_step, scratch);
    hipLaunchKernelGGL(threshold_kernel, dim3(1), dim3(kWave), 0, s, scratch, num_samples);
    hipLaunchKernelGGL(collect_kernel, dim3(blocks), dim3(256), 0, s, weights, static_cast<long long>(count), seed, stream_offset, device_step, scratch);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(1024), 0, s, scratch, num_samples, reinterpret_cast<long long*>(indices));
    return launch_status();
}

size_t vsrd_ray_table_bytes(int64_t count) { return count < 1 ? 0 : ray_table_bytes(count); }

int32_t vsrd_ray_table_build(const float* weights, int64_t count, void* table, size_t table_bytes, void* stream) {
    if (!weights || !table || count < 1 || count >= 0xffffffffll) return VSRD_E_INVALID_ARGUMENT;
    if (table_bytes < ray_table_bytes(count)) return VSRD_E_WORKSPACE;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    RayTableHeader* header = static_cast<RayTableHeader*>(table);
    if (hipMemsetAsync(header, 0, sizeof(RayTableHeader), s) != hipSuccess) return VSRD_E_LAUNCH;
    const long long blocks = ray_table_blocks(count);
    hipLaunchKernelGGL(ray_table_max_kernel, dim3(static_cast<unsigned>(blocks > 1024 ? 1024 : blocks)), dim3(256), 0, s, weights, static_cast<long long>(count), header);
    hipLaunchKernelGGL(ray_table_sums_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, weights, static_cast<long long>(count), header);
    hipLaunchKernelGGL(ray_table_offsets_kernel, dim3(1), dim3(1024), 0, s, static_cast<long long>(count), header);
    hipLaunchKernelGGL(ray_table_fill_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, weights, static_cast<long long>(count), header);
    const long long boundaries = (1ll << ray_table_guide_bits(count)) + 1;
    hipLaunchKernelGGL(ray_table_guide_kernel, dim3(static_cast<unsigned>((boundaries + 255) / 256)), dim3(256), 0, s, static_cast<long long>(count), header);
    return launch_status();
}

int32_t vsrd_sample_rays_table(void* table, int64_t count, int32_t num_samples, uint64_t seed, uint64_t stream_offset,
                               const uint64_t* device_stream_offset, const int64_t* remap, int64_t* indices, void* stream) {
    if (!table || !indices || count < 1 || count >= 0xffffffffll || num_samples < 1 || num_samples > kSampleMax) return VSRD_E_INVALID_ARGUMENT;
    if (opt_in_lds(sample_table_kernel, kTableLdsBytes) != VSRD_OK) return VSRD_E_LAUNCH;
    hipLaunchKernelGGL(sample_table_kernel, dim3(1), dim3(kTableThreads), kTableLdsBytes, static_cast<hipStream_t>(stream), static_cast<RayTableHeader*>(table),
                       static_cast<long long>(count), num_samples, seed, stream_offset, reinterpret_cast<const unsigned long long*>(device_stream_offset),
                       reinterpret_cast<const long long*>(remap), reinterpret_cast<long long*>(indices));
    return launch_status();
}

int32_t vsrd_sample_rays_table_frames(void* table, int64_t count, int32_t num_samples, uint64_t seed, const uint64_t* device_stream_offset,
                                      int64_t* indices, int32_t num_frames, int64_t frame_stride, void* stream) {
    Frames frames;
    if (!table || !indices || !device_stream_offset || count < 1 || count >= 0xffffffffll || num_samples < 1 || num_samples > kSampleMax ||
        !frames_of(num_frames, frame_stride, &frames))
        return VSRD_E_INVALID_ARGUMENT;
    if (opt_in_lds(sample_table_frames_kernel, kTableLdsBytes) != VSRD_OK) return VSRD_E_LAUNCH;
    hipLaunchKernelGGL(sample_table_frames_kernel, dim3(1, frames.count), dim3(kTableThreads), kTableLdsBytes, static_cast<hipStream_t>(stream),
                       static_cast<RayTableHeader*>(table), static_cast<long long>(count), num_samples, seed,
                       reinterpret_cast<const unsigned long long*>(device_stream_offset), reinterpret_cast<long long*>(indices), frames.stride);
    return launch_status();
}

int32_t vsrd_match_boxes(const float* pd_boxes, const float* gt_boxes, int32_t num_pd, int32_t num_gt,
                         int64_t* pd_indices, int64_t* gt_indices, void* stream) {
    if (!pd_boxes || !gt_boxes || !pd_indices || !gt_indices || num_pd < 1 || num_gt < 1 || num_pd > 64 || num_gt > 64) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(match_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), nullptr, pd_boxes, gt_boxes, num_pd, num_gt,
                       reinterpret_cast<long long*>(pd_indices), reinterpret_cast<long long*>(gt_indices));
    return launch_status();
}

int32_t vsrd_linear_sum_assignment(const float* cost, int32_t num_rows, int32_t num_cols, int64_t* row_indices, int64_t* col_indices, void* stream) {
    if (!cost || !row_indices || !col_indices || num_rows < 1 || num_cols < 1 || num_rows > 64 || num_cols > 64) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(match_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), cost, nullptr, nullptr, num_rows, num_cols,
                       reinterpret_cast<long long*>(row_indices), reinterpret_cast<long long*>(col_indices));
    return launch_status();
}

#ifdef VSRD_PHASE_TIMERS
// Experiments only (tools/phase_timers.py): read (and optionally clear) the per-phase tick totals of the fused step kernels.
int32_t vsrd_debug_phase_cycles(unsigned long long* out16, int32_t reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_cycles), 16 * sizeof(unsigned long long)) != hipSuccess) return VSRD_E_LAUNCH;
    if (reset) {
        unsigned long long zeros[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), zeros, sizeof(zeros)) != hipSuccess) return VSRD_E_LAUNCH;
    }
    return VSRD_OK;
}
#endif

// Not part of the public header: exercised by tests/test_hip_wave.py.
int32_t vsrd_selftest_wave(const float* in64, float* out512, void* stream) {
    if (!in64 || !out512) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(wave_selftest_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in64, out512);  // writes 576 floats
    return launch_status();
}

// erf_gelu / erf_gelu_derivative of csrc/hypernetwork.h at n points: out[0..n) values, out[n..2n) derivatives
// (tests/test_hip_step.py::test_hypernetwork_gelu_error_bound).
int32_t vsrd_selftest_gelu(const float* x, int32_t n, float* out, void* stream) {
    if (!x || !out || n < 1) return VSRD_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(gelu_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), x, n, out);
    return launch_status();
}

}  // extern "C"
