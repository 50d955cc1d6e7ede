// Multi-view patch-correlation photometric loss (scripts/main.py:783-851), forward and backward, on the device: for every converged ray
// the plane (position p, normal n) at its surface point induces a homography from the target view into every view; a pw x ph patch around
// the target pixel is sampled bilinearly in every view, the V patches are correlated, the top-k coefficients of every row of the V x V
// matrix are kept, and the loss is (1 - nanmean(kept)) / 2.  The reference composes this from V grid_sample calls, V R small matrix chains
// and a Python loop with cov / diag / sqrt / topk per ray; here it is three launches forward and two backward, no host synchronisation,
// no allocation, capturable.  The arithmetic is tiny (100 rays x 17 views x 121 pixels): the gain is launch count, not throughput.
//
// The reference's quirks are kept (include/vsrd_hip.h has the full list): the align-corners map followed by grid_sample's
// align_corners=False (sample at s W / (W - 1) - 0.5: even the identity homography interpolates), zeros padding, the unbiased covariance,
// sqrt(cov_ii cov_jj + 1e-12) (a constant patch has coefficient 0, not NaN), the self-coefficient among the top-k, NaN ranked first by
// the selection and dropped by the mean.  Two stated deviations: the images are turned gray BEFORE the interpolation (both maps are
// linear: equal in exact arithmetic, a third of the gathers), and a frame without a converged ray has loss 0 and zero gradients where
// the reference adds no term.
//
//   patch_gray_kernel         [V,3,H,W] -> [V,H,W], gray = fma(0.114, b, fma(0.587, g, 0.2989 r)), the products written out;
//   patch_constants_kernel    one wave: A_s = K_s R_s R_t^T K_t^-1, b_s = K_s R_s (R_s^T t_s - R_t^T t_t) in double (the 3x3 inverse by
//                             adjugate, any skew), stored as float [V,12] = (A row-major | b), then K_t^-1 [9]:
//                             H = A_s + b_s (K_t^-T n)^T / (n.p), so h = A_s q + b_s w with w = n.(K_t^-1 q) / (n.p) a scalar of ray and pixel;
//   patch_correlation_forward_kernel   one workgroup of 256 threads per ray.  The four waves stride over the views, a lane takes pixels
//                             lane, lane + 64, ...; the centred patches live in LDS [V][P].  The V (V + 1) / 2 covariances are dealt to
//                             the waves as wave_sums of P products; the rows of the coefficient matrix are dealt to the waves, lane j
//                             holds column j and k passes of a wave-wide maximum over (ordered value, lowest index) select the row's
//                             top-k.  Every ray writes its own (sum, count);
//   patch_loss_kernel         one wave adds the R pairs in ascending blocks of 64 and writes stats and the loss;
//   patch_correlation_backward_kernel  recomputes its ray's forward with the same __device__ functions (the selection is bit-identical by
//                             construction; only the global count is carried over), then d loss / d coefficient -> d covariance ->
//                             d patch value -> the four taps -> the sample coordinates -> the division -> w -> n and p.
// Every reduction has a fixed order (lane partial sums in ascending pixel order, wave_sum, waves and rows in ascending order); there are no
// floating-point atomics.
//
// Sampling hazards: a plane that passes near a source camera sends coordinates to +-5e8 and beyond, and h_z + 1e-6 == 0 makes them
// non-finite.  Inside-ness is decided in floating point (-1 < x < W and -1 < y < H, false for NaN) BEFORE any conversion to integer; only
// then is floor(x) in [-1, W-1] converted, and each of the four taps is bounds-checked as an integer.  A sample that is outside or
// non-finite reads 0 and passes no gradient.
#pragma once
#include "wave.h"

namespace vsrd {

constexpr int kPatchMaxViews = 32;           // VSRD_PATCH_MAX_VIEWS
constexpr int kPatchMaxPixels = 256;         // VSRD_PATCH_MAX_PIXELS
constexpr int kPatchMaxRays = 65535;         // VSRD_PATCH_MAX_RAYS
constexpr int kPatchThreads = 256;
constexpr int kPatchWaves = kPatchThreads / kWave;
constexpr int kPatchViewFloats = 12;         // A_s row-major, b_s

struct PatchArgs {
    int num_views, num_rays, height, width, patch_width, patch_height, top_k, target_view;
    float sample_epsilon, correlation_epsilon;
    const float* gray;                       // [V,H,W]
    const float* intrinsics;                 // [V,3,3]
    const float* extrinsics;                 // [V,4,4]
    const int* pixels;                       // [R,2] = (x, y)
    const float* positions;                  // [R,3]
    const float* normals;                    // [R,3]
    const unsigned char* converged;          // [R]
    float* constants;                        // workspace: [V,12] + K_t^-1 [9] (padded to 12)
    float* ray_stats;                        // workspace: [R,2] = (sum, count) of the ray's selected non-NaN coefficients
    int view_capacity;                       // the extent of every per-view array: num_views, and in a batch with headers the by-value V
    long long frame_stride;                  // a batch of frames (wave.h; the kFrames kernels): bytes between the frames' buffers
    const FrameHeader* header;               // ... and the frames' own view counts, or null: every frame has view_capacity views
};

// The kFrames kernels (a batch of frames, wave.h): the frame is blockIdx.y (the one-frame grids are 1-D), every pointer of `a` moves by its
// frame's shift and num_views becomes the frame's own v_f; view_capacity stays the by-value V, behind whose constants K_t^-1 lies.
// Returns the shift, for the kernel's other pointers.  A frame with fewer views than top_k is not served: the host cannot see v_f, so such
// a frame is treated as a frame without a converged ray (loss 0, stats (0, 0), zero gradients).
__device__ __forceinline__ long long patch_of_frame(PatchArgs& a) {
    const long long shift = frame_shift(a.frame_stride, blockIdx.y);
    a.gray = of_frame_nonnull(a.gray, shift); a.intrinsics = of_frame_nonnull(a.intrinsics, shift); a.extrinsics = of_frame_nonnull(a.extrinsics, shift);
    a.pixels = of_frame_nonnull(a.pixels, shift); a.positions = of_frame_nonnull(a.positions, shift); a.normals = of_frame_nonnull(a.normals, shift);
    a.converged = of_frame_nonnull(a.converged, shift); a.constants = of_frame_nonnull(a.constants, shift); a.ray_stats = of_frame_nonnull(a.ray_stats, shift);
    a.num_views = frame_views(a.header ? of_frame_nonnull(a.header, shift) : nullptr, a.view_capacity);
    return shift;
}
template <bool kFrames>
__device__ __forceinline__ bool patch_served(const PatchArgs& a) { return !kFrames || a.top_k <= a.num_views; }

// ---- grayscale ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float patch_gray(float r, float g, float b) {
    return __fmaf_rn(0.114f, b, __fmaf_rn(0.587f, g, __fmul_rn(0.2989f, r)));
}

// grid (blocks, V).  A view whose four planes are 16-byte aligned goes through float4 accesses with a scalar tail (H W % 4 pixels); any
// other view (H W no multiple of 4 shifts every second plane) through scalar accesses alone.
__global__ __launch_bounds__(256) void patch_gray_kernel(const float* __restrict__ images, float* __restrict__ gray, long long plane) {
    const long long v = blockIdx.y;
    const float* const r = images + 3 * v * plane;
    const float* const g = r + plane;
    const float* const b = g + plane;
    float* const out = gray + v * plane;
    const unsigned long long bits = reinterpret_cast<unsigned long long>(r) | reinterpret_cast<unsigned long long>(g) |
                                    reinterpret_cast<unsigned long long>(b) | reinterpret_cast<unsigned long long>(out);
    const long long body = (bits & 15ull) == 0 ? plane & ~3ll : 0;
    const long long first = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x, stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = first; i < body / 4; i += stride) {
        const float4 r4 = reinterpret_cast<const float4*>(r)[i], g4 = reinterpret_cast<const float4*>(g)[i], b4 = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(patch_gray(r4.x, g4.x, b4.x), patch_gray(r4.y, g4.y, b4.y), patch_gray(r4.z, g4.z, b4.z),
                                                        patch_gray(r4.w, g4.w, b4.w));
    }
    for (long long i = body + first; i < plane; i += stride) out[i] = patch_gray(r[i], g[i], b[i]);
}

// ---- per-view constants ---------------------------------------------------------------------------------------------------------
// One wave.  K_t^-1 first (lane e < 9: entry e, cofactor over determinant, through LDS), then lane-strided over the V x 12 outputs, every
// output its own short sums in double straight from the matrices: no per-lane arrays, a handful of registers.
__device__ __forceinline__ double patch_k(const PatchArgs& a, int v, int i, int j) { return a.intrinsics[9 * v + 3 * i + j]; }
__device__ __forceinline__ double patch_r(const PatchArgs& a, int v, int i, int j) { return a.extrinsics[16 * v + 4 * i + j]; }

template <bool kFrames = false>
__global__ __launch_bounds__(kWave) void patch_constants_kernel(PatchArgs a) {
    __shared__ double inverse[9];
    if (kFrames) patch_of_frame(a);
    const int lane = static_cast<int>(threadIdx.x), t = a.target_view;
    if (lane < 9) {                                              // inverse[i][j] = cofactor[j][i] / det: any skew
        const int i = lane / 3, j = lane % 3;
        const int r1 = (j + 1) % 3, r2 = (j + 2) % 3, c1 = (i + 1) % 3, c2 = (i + 2) % 3;
        const double cofactor = patch_k(a, t, r1, c1) * patch_k(a, t, r2, c2) - patch_k(a, t, r1, c2) * patch_k(a, t, r2, c1);
        const double determinant = patch_k(a, t, 0, 0) * (patch_k(a, t, 1, 1) * patch_k(a, t, 2, 2) - patch_k(a, t, 1, 2) * patch_k(a, t, 2, 1)) -
                                   patch_k(a, t, 0, 1) * (patch_k(a, t, 1, 0) * patch_k(a, t, 2, 2) - patch_k(a, t, 1, 2) * patch_k(a, t, 2, 0)) +
                                   patch_k(a, t, 0, 2) * (patch_k(a, t, 1, 0) * patch_k(a, t, 2, 1) - patch_k(a, t, 1, 1) * patch_k(a, t, 2, 0));
        inverse[lane] = cofactor / determinant;
        a.constants[a.view_capacity * kPatchViewFloats + lane] = static_cast<float>(inverse[lane]);
    }
    __syncthreads();
    for (int e = lane; e < a.num_views * kPatchViewFloats; e += kWave) {
        const int s = e / kPatchViewFloats, o = e % kPatchViewFloats;
        double value = 0.0;
        if (o < 9) {                                             // A_s[i][j] = sum K_s[i][x] R_s[x][c] R_t[y][c] K_t^-1[y][j]
            const int i = o / 3, j = o % 3;
            for (int x = 0; x < 3; ++x)
                for (int y = 0; y < 3; ++y) {
                    double m = 0.0;                              // (R_s R_t^T)[x][y]
                    for (int c = 0; c < 3; ++c) m += patch_r(a, s, x, c) * patch_r(a, t, y, c);
                    value += patch_k(a, s, i, x) * m * inverse[3 * y + j];
                }
        } else {                                                 // b_s[i] = sum K_s[i][x] R_s[x][y] (R_s^T t_s - R_t^T t_t)[y]
            const int i = o - 9;
            for (int y = 0; y < 3; ++y) {
                double c = 0.0;
                for (int m = 0; m < 3; ++m) c += patch_r(a, s, m, y) * patch_r(a, s, m, 3) - patch_r(a, t, m, y) * patch_r(a, t, m, 3);
                double kr = 0.0;
                for (int x = 0; x < 3; ++x) kr += patch_k(a, s, i, x) * patch_r(a, s, x, y);
                value += kr * c;
            }
        }
        a.constants[e] = static_cast<float>(value);
    }
}

// ---- one ray's forward ----------------------------------------------------------------------------------------------------------
struct PatchShared {
    float patches[kPatchMaxViews * kPatchMaxPixels];             // [V][P], centred after patch_ray_sample
    float covariance[kPatchMaxViews * kPatchMaxViews];           // [V][V], symmetric
    unsigned selected[kPatchMaxViews];                           // bit j of row i: coefficient (i, j) is among the row's top-k
    float row_sum[kPatchMaxViews], row_count[kPatchMaxViews];    // over the row's selected non-NaN coefficients
};

struct PatchRay {
    float x, y, n[3], p[3], plane;                               // plane = n.p
    float k_inverse[9];
    float scale_x, scale_y;                                      // W / (W - 1), H / (H - 1)
};

__device__ __forceinline__ PatchRay patch_load_ray(const PatchArgs& a, int ray) {
    PatchRay r;
    r.x = static_cast<float>(a.pixels[2 * ray]); r.y = static_cast<float>(a.pixels[2 * ray + 1]);
    for (int i = 0; i < 3; ++i) { r.n[i] = a.normals[3 * ray + i]; r.p[i] = a.positions[3 * ray + i]; }
    r.plane = __fmaf_rn(r.n[2], r.p[2], __fmaf_rn(r.n[1], r.p[1], __fmul_rn(r.n[0], r.p[0])));
    const float* const k_inverse = a.constants + a.view_capacity * kPatchViewFloats;
    for (int i = 0; i < 9; ++i) r.k_inverse[i] = k_inverse[i];
    r.scale_x = static_cast<float>(a.width) / static_cast<float>(a.width - 1);
    r.scale_y = static_cast<float>(a.height) / static_cast<float>(a.height - 1);
    return r;
}

// Pixel `pixel` of the patch grid (x the fast index, offsets arange(size) - size // 2): the back-projected target pixel g = K_t^-1 q and
// the plane's scalar w = n.g / n.p.
struct PatchPixel { float qx, qy, g[3], w; };
__device__ __forceinline__ PatchPixel patch_pixel(const PatchArgs& a, const PatchRay& r, int pixel) {
    PatchPixel q;
    q.qx = r.x + static_cast<float>(pixel % a.patch_width - a.patch_width / 2);
    q.qy = r.y + static_cast<float>(pixel / a.patch_width - a.patch_height / 2);
    for (int i = 0; i < 3; ++i) q.g[i] = __fmaf_rn(r.k_inverse[3 * i], q.qx, __fmaf_rn(r.k_inverse[3 * i + 1], q.qy, r.k_inverse[3 * i + 2]));
    q.w = __fmaf_rn(r.n[2], q.g[2], __fmaf_rn(r.n[1], q.g[1], __fmul_rn(r.n[0], q.g[0]))) / r.plane;
    return q;
}

// One bilinear sample of a gray plane at the homography's image of the pixel.  `valid` false: outside or non-finite, value and slopes 0.
struct PatchSample { float value, slope_x, slope_y, sx, sy, depth; bool valid; };
__device__ __forceinline__ PatchSample patch_sample(const PatchArgs& a, const PatchRay& r, const float* __restrict__ view /* [12] */,
                                                    const float* __restrict__ plane, const PatchPixel& q) {
    PatchSample s;
    const float hx = __fmaf_rn(view[0], q.qx, __fmaf_rn(view[1], q.qy, __fmaf_rn(view[9], q.w, view[2])));
    const float hy = __fmaf_rn(view[3], q.qx, __fmaf_rn(view[4], q.qy, __fmaf_rn(view[10], q.w, view[5])));
    const float hz = __fmaf_rn(view[6], q.qx, __fmaf_rn(view[7], q.qy, __fmaf_rn(view[11], q.w, view[8])));
    s.depth = hz + a.sample_epsilon;
    s.sx = hx / s.depth; s.sy = hy / s.depth;
    const float px = __fmaf_rn(s.sx, r.scale_x, -0.5f), py = __fmaf_rn(s.sy, r.scale_y, -0.5f);
    s.value = s.slope_x = s.slope_y = 0.0f;
    // decided in floating point, false for NaN: nothing below converts a float that has not passed here
    s.valid = px > -1.0f && px < static_cast<float>(a.width) && py > -1.0f && py < static_cast<float>(a.height);
    if (!s.valid) return s;
    const float x0f = floorf(px), y0f = floorf(py);              // in [-1, W-1] x [-1, H-1]
    const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
    const float fx = px - x0f, fy = py - y0f;
    const bool left = x0 >= 0 && x0 < a.width, right = x0 + 1 >= 0 && x0 + 1 < a.width;
    const bool top = y0 >= 0 && y0 < a.height, bottom = y0 + 1 >= 0 && y0 + 1 < a.height;
    const long long row0 = static_cast<long long>(y0) * a.width, row1 = row0 + a.width;
    const float v00 = top && left ? plane[row0 + x0] : 0.0f, v10 = top && right ? plane[row0 + x0 + 1] : 0.0f;
    const float v01 = bottom && left ? plane[row1 + x0] : 0.0f, v11 = bottom && right ? plane[row1 + x0 + 1] : 0.0f;
    const float upper = __fmaf_rn(fx, v10 - v00, v00), lower = __fmaf_rn(fx, v11 - v01, v01);
    s.value = __fmaf_rn(fy, lower - upper, upper);
    s.slope_x = __fmaf_rn(fy, (v11 - v01) - (v10 - v00), v10 - v00);
    s.slope_y = lower - upper;
    return s;
}

// Phase 1: wave w samples views w, w + 4, ...; the raw patch goes to `patches_out` [V,R,P] when given, its centred form to LDS.
__device__ __forceinline__ void patch_ray_sample(const PatchArgs& a, const PatchRay& r, int ray, PatchShared& sh, float* __restrict__ patches_out) {
    const int lane = lane_id(), P = a.patch_width * a.patch_height;
    for (int v = wave_in_block(); v < a.num_views; v += kPatchWaves) {
        const float* const view = a.constants + v * kPatchViewFloats;
        const float* const plane = a.gray + static_cast<long long>(v) * a.height * a.width;
        float sum = 0.0f;
        for (int pixel = lane; pixel < P; pixel += kWave) {
            const float value = patch_sample(a, r, view, plane, patch_pixel(a, r, pixel)).value;
            sh.patches[v * P + pixel] = value;
            if (patches_out) patches_out[(static_cast<long long>(v) * a.num_rays + ray) * P + pixel] = value;
            sum += value;
        }
        const float mean = wave_sum(sum) / static_cast<float>(P);
        for (int pixel = lane; pixel < P; pixel += kWave) sh.patches[v * P + pixel] -= mean;        // (the lane's own entries)
    }
}

__device__ __forceinline__ float patch_coefficient(float cov_ij, float cov_ii, float cov_jj, float epsilon) {
    return cov_ij / sqrtf(__fmaf_rn(cov_ii, cov_jj, epsilon));
}

// torch.topk's order as an unsigned key: NaN above every number, then the numbers in ascending order (-0 == +0)
__device__ __forceinline__ unsigned patch_order_key(float c) {
    if (c != c) return 0xffffffffu;
    const unsigned bits = c == 0.0f ? 0u : __builtin_bit_cast(unsigned, c);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// Phases 2 and 3 (the caller has put a barrier behind phase 1): covariances, then every row's top-k.  Leaves sh.covariance,
// sh.selected, sh.row_sum and sh.row_count behind a barrier.
__device__ __forceinline__ void patch_ray_correlate(const PatchArgs& a, int ray, PatchShared& sh, float* __restrict__ coefficients, int* __restrict__ selected) {
    const int lane = lane_id(), wave = wave_in_block(), V = a.num_views, P = a.patch_width * a.patch_height;
    const float unbiased = static_cast<float>(P - 1);
    int pair = 0;
    for (int i = 0; i < V; ++i)
        for (int j = i; j < V; ++j, ++pair) {
            if (pair % kPatchWaves != wave) continue;
            float sum = 0.0f;
            for (int pixel = lane; pixel < P; pixel += kWave) sum = __fmaf_rn(sh.patches[i * P + pixel], sh.patches[j * P + pixel], sum);
            const float covariance = wave_sum(sum) / unbiased;
            if (lane == 0) sh.covariance[i * V + j] = sh.covariance[j * V + i] = covariance;
        }
    __syncthreads();
    for (int i = wave; i < V; i += kPatchWaves) {
        const bool column = lane < V;
        const float c = column ? patch_coefficient(sh.covariance[i * V + lane], sh.covariance[i * V + i], sh.covariance[lane * V + lane], a.correlation_epsilon) : 0.0f;
        if (column && coefficients) coefficients[(static_cast<long long>(ray) * V + i) * V + lane] = c;
        const unsigned long long own = (static_cast<unsigned long long>(patch_order_key(c)) << 32) | static_cast<unsigned>(kWave - 1 - lane);
        bool alive = column;
        unsigned chosen = 0u;
        float sum = 0.0f, count = 0.0f;
        for (int pass = 0; pass < a.top_k; ++pass) {             // top_k <= V: some column is alive in every pass
            unsigned long long best = alive ? own : 0ull;        // (a live key is above 0: the lowest ordered value is 0x007fffff)
            for (int step = 1; step < kWave; step <<= 1) {
                const unsigned long long other = __shfl_xor(best, step, kWave);
                best = other > best ? other : best;
            }
            const int winner = __builtin_amdgcn_readfirstlane(kWave - 1 - static_cast<int>(best & 63ull));
            const float value = read_lane(c, winner);
            if (value == value) { sum += value; count += 1.0f; }
            chosen |= 1u << winner;
            if (lane == winner) alive = false;
        }
        if (lane == 0) {
            sh.selected[i] = chosen; sh.row_sum[i] = sum; sh.row_count[i] = count;
            if (selected) selected[ray * V + i] = static_cast<int>(chosen);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void patch_clear_exports(const PatchArgs& a, int ray, float* __restrict__ coefficients, int* __restrict__ selected) {
    const int V = a.num_views;
    for (int e = static_cast<int>(threadIdx.x); e < V * V; e += kPatchThreads) {
        if (coefficients) coefficients[static_cast<long long>(ray) * V * V + e] = 0.0f;
        if (selected && e < V) selected[ray * V + e] = 0;
    }
}

// grid R.  patches [V,R,P], coefficients [R,V,V], selected [R,V]: optional exports.  An unconverged ray writes (0, 0) and zero
// coefficient / selection rows; its patches are sampled only when they are exported (the reference samples every ray's).
template <bool kFrames = false>
__global__ __launch_bounds__(kPatchThreads) void patch_correlation_forward_kernel(PatchArgs a, float* __restrict__ patches, float* __restrict__ coefficients,
                                                                                  int* __restrict__ selected) {
    __shared__ PatchShared sh;
    if (kFrames) {
        const long long shift = patch_of_frame(a);
        VSRD_OF_FRAME(patches, shift); VSRD_OF_FRAME(coefficients, shift); VSRD_OF_FRAME(selected, shift);
    }
    const int ray = static_cast<int>(blockIdx.x);
    const bool converged = a.converged[ray] != 0 && patch_served<kFrames>(a);      // (uniform over the workgroup: everybody leaves or nobody)
    if (converged || patches) {
        const PatchRay r = patch_load_ray(a, ray);
        patch_ray_sample(a, r, ray, sh, patches);
    }
    if (!converged) {
        if (threadIdx.x == 0) { a.ray_stats[2 * ray] = 0.0f; a.ray_stats[2 * ray + 1] = 0.0f; }
        patch_clear_exports(a, ray, coefficients, selected);
        return;
    }
    __syncthreads();
    patch_ray_correlate(a, ray, sh, coefficients, selected);
    if (threadIdx.x == 0) {
        float sum = 0.0f, count = 0.0f;
        for (int i = 0; i < a.num_views; ++i) { sum += sh.row_sum[i]; count += sh.row_count[i]; }
        a.ray_stats[2 * ray] = sum; a.ray_stats[2 * ray + 1] = count;
    }
}

// One wave: the rays' pairs in ascending blocks of 64 (wave_sum inside a block, double across blocks).  stats = (sum, count);
// loss = (1 - sum / count) / 2, NaN when rays converged but every selected coefficient is NaN (the reference's nanmean), and 0 when no
// ray converged (the reference adds no term: the same weighted sum).
template <bool kFrames = false>
__global__ __launch_bounds__(kWave) void patch_loss_kernel(PatchArgs a, float* __restrict__ loss, float* __restrict__ stats) {
    if (kFrames) {
        const long long shift = patch_of_frame(a);
        VSRD_OF_FRAME_NONNULL(loss, shift); VSRD_OF_FRAME_NONNULL(stats, shift);
    }
    const bool served = patch_served<kFrames>(a);
    const int lane = lane_id();
    double sum = 0.0, count = 0.0, converged = 0.0;
    for (int base = 0; base < a.num_rays; base += kWave) {
        const int ray = base + lane;
        const bool inside = ray < a.num_rays;
        sum += static_cast<double>(wave_sum(inside ? a.ray_stats[2 * ray] : 0.0f));
        count += static_cast<double>(wave_sum(inside ? a.ray_stats[2 * ray + 1] : 0.0f));
        converged += static_cast<double>(wave_sum(inside && served && a.converged[ray] != 0 ? 1.0f : 0.0f));
    }
    if (lane == 0) {
        stats[0] = static_cast<float>(sum); stats[1] = static_cast<float>(count);
        loss[0] = converged == 0.0 ? 0.0f : static_cast<float>((1.0 - sum / count) * 0.5);
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// loss = (1 - S / C) / 2: every selected non-NaN coefficient c_ij (row i's selection; the matrix of selections is not symmetric) has
// d loss / d c_ij = -upstream / (2 C) =: G_ij.  With r_ij = (cov_ii cov_jj + eps)^-1/2 and c_ij = cov_ij r_ij, and the entries of cov
// taken as independent,
//   d c_ij / d cov_ij = r_ij,   d c_ij / d cov_ii = -cov_ij cov_jj r_ij^3 / 2,   d c_ij / d cov_jj = -cov_ij cov_ii r_ij^3 / 2,
// so the symmetrised adjoint S = Gcov + Gcov^T is S_ij = (G_ij + G_ji) r_ij minus, on the diagonal, sum_j (G_ij + G_ji) cov_ij cov_jj r_ij^3.
// cov_ab = sum_p c_a[p] c_b[p] / (P - 1) over the centred patches gives d loss / d X_a[p] = sum_b S_ab c_b[p] / (P - 1); the centring's
// own projection is dropped, since the rows c_b sum to 0 up to rounding (1e-7 of the entries).  Entries with G = 0 are skipped, not
// multiplied: a NaN coefficient elsewhere in the matrix passes nothing on.
// Through the sample: X = bilinear(px, py), px = sx W / (W - 1) - 0.5, sx = hx / d, d = hz + eps, h = A q + b w, w = n.g / n.p:
//   d w / d n = (g - w p) / n.p,   d w / d p = -w n / n.p,
// so the ray needs four sums over its V P samples, T0 = sum dw g (three components) and T1 = sum dw w: lane partial sums, wave_sum, then
// the waves in ascending order.  grad_n = (T0 - T1 p) / n.p, grad_p = -T1 n / n.p; a plane through the origin (n.p == 0) has no valid
// sample and gets zeros.
template <bool kFrames = false>
__global__ __launch_bounds__(kPatchThreads) void patch_correlation_backward_kernel(PatchArgs a, const float* __restrict__ stats, const float* __restrict__ upstream,
                                                                                   float* __restrict__ grad_positions, float* __restrict__ grad_normals) {
    __shared__ PatchShared sh;
    __shared__ float adjoint[kPatchMaxViews * kPatchMaxViews];   // S
    __shared__ float partial[kPatchWaves][4];
    if (kFrames) {
        const long long shift = patch_of_frame(a);
        VSRD_OF_FRAME_NONNULL(stats, shift); VSRD_OF_FRAME_NONNULL(upstream, shift); VSRD_OF_FRAME_NONNULL(grad_positions, shift);
        VSRD_OF_FRAME_NONNULL(grad_normals, shift);
    }
    const int ray = static_cast<int>(blockIdx.x), thread = static_cast<int>(threadIdx.x), lane = lane_id(), wave = wave_in_block();
    const int V = a.num_views, P = a.patch_width * a.patch_height;
    if (a.converged[ray] == 0 || !patch_served<kFrames>(a)) {
        if (thread < 3) { grad_positions[3 * ray + thread] = 0.0f; grad_normals[3 * ray + thread] = 0.0f; }
        return;
    }
    const PatchRay r = patch_load_ray(a, ray);
    patch_ray_sample(a, r, ray, sh, nullptr);
    __syncthreads();
    patch_ray_correlate(a, ray, sh, nullptr, nullptr);
    const float g = -0.5f * upstream[0] / stats[1];
    for (int e = thread; e < V * V; e += kPatchThreads) {
        const int i = e / V, j = e % V;
        const float cov_ij = sh.covariance[e], cov_ii = sh.covariance[i * V + i], cov_jj = sh.covariance[j * V + j];
        const float c = patch_coefficient(cov_ij, cov_ii, cov_jj, a.correlation_epsilon);      // (c_ij and c_ji are the same bits)
        const int times = c == c ? static_cast<int>((sh.selected[i] >> j) & 1u) + static_cast<int>((sh.selected[j] >> i) & 1u) : 0;
        adjoint[e] = times == 0 ? 0.0f : static_cast<float>(times) * g / sqrtf(__fmaf_rn(cov_ii, cov_jj, a.correlation_epsilon));
    }
    __syncthreads();
    if (thread < V) {                                            // the diagonal: lane i walks its row in ascending j
        const int i = thread;
        const float cov_ii = sh.covariance[i * V + i];
        float extra = 0.0f;
        for (int j = 0; j < V; ++j) {
            const float s = adjoint[i * V + j];
            if (s == 0.0f) continue;
            const float cov_jj = sh.covariance[j * V + j];
            extra += s * sh.covariance[i * V + j] * cov_jj / __fmaf_rn(cov_ii, cov_jj, a.correlation_epsilon);
        }
        adjoint[i * V + i] -= extra;
    }
    __syncthreads();
    const float unbiased = static_cast<float>(P - 1);
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
    for (int v = wave; v < V; v += kPatchWaves) {
        const float* const view = a.constants + v * kPatchViewFloats;
        const float* const plane = a.gray + static_cast<long long>(v) * a.height * a.width;
        for (int pixel = lane; pixel < P; pixel += kWave) {
            const PatchPixel q = patch_pixel(a, r, pixel);
            const PatchSample s = patch_sample(a, r, view, plane, q);
            if (!s.valid) continue;
            float gx = 0.0f;
            for (int b = 0; b < V; ++b) {
                const float weight = adjoint[v * V + b];         // (uniform over the wave)
                if (weight != 0.0f) gx = __fmaf_rn(weight, sh.patches[b * P + pixel], gx);
            }
            gx /= unbiased;
            const float gsx = gx * s.slope_x * r.scale_x, gsy = gx * s.slope_y * r.scale_y;
            const float dhx = gsx / s.depth, dhy = gsy / s.depth, dhz = -(gsx * s.sx + gsy * s.sy) / s.depth;
            const float dw = view[9] * dhx + view[10] * dhy + view[11] * dhz;
            t0 = __fmaf_rn(dw, q.g[0], t0); t1 = __fmaf_rn(dw, q.g[1], t1); t2 = __fmaf_rn(dw, q.g[2], t2); t3 = __fmaf_rn(dw, q.w, t3);
        }
    }
    t0 = wave_sum(t0); t1 = wave_sum(t1); t2 = wave_sum(t2); t3 = wave_sum(t3);
    if (lane == 0) { partial[wave][0] = t0; partial[wave][1] = t1; partial[wave][2] = t2; partial[wave][3] = t3; }
    __syncthreads();
    if (thread == 0) {
        float total[4];
        for (int c = 0; c < 4; ++c) total[c] = ((partial[0][c] + partial[1][c]) + partial[2][c]) + partial[3][c];
        const float inverse = r.plane != 0.0f ? 1.0f / r.plane : 0.0f;
        for (int c = 0; c < 3; ++c) {
            grad_normals[3 * ray + c] = (total[c] - total[3] * r.p[c]) * inverse;
            grad_positions[3 * ray + c] = -total[3] * r.n[c] * inverse;
        }
    }
}

}  // namespace vsrd
