// vsrd_frame_ingest: a compact frame pack (one polygon and one bit-packed binary mask per (view, instance) entry; vsrd_amd/frames.py)
// straight into the buffers a frame's graphs read -- the soft masks [V*H*W, stride] in the target's instance order, the importance
// weights (their row maximum), the ground-truth 2-D boxes and the visibility.  What the reference does per frame in three places:
// SoftRasterizer (vsrd/transforms/geometric_transforms.py:265-317), BoxGenerator (:151-159) and the re-indexing of every view to the
// target's instance order (scripts/main.py:204-265), followed by the amax of main.py:620-624.
//
// Two kernels.  frame_ingest_boxes_kernel: one workgroup per (view, slot) reduces the entry's bits to its box and its visibility, and
// takes an entry without a set bit out of the table.  frame_ingest_pixels_kernel: the pixel pass, V x N x HW x P segment distances.
//   - a workgroup owns kIngestPixels x 256 consecutive pixels of ONE view, so the slot -> entry table and the polygon are uniform over it;
//   - the constants of a polygon side -- start vertex, side vector, 1 / (|s|^2 + 1e-6) -- are staged in LDS once per workgroup and chunk of
//     kIngestChunk sides (one side, one division per thread); the loop over the sides reads them with one ds_read_b128 and one ds_read_b32
//     from an address all lanes share (a broadcast: no bank conflict), and holds no division and no square root: it takes the minimum
//     of the SQUARED distances, and one sqrtf per (pixel, instance) follows -- sqrtf is correctly rounded and monotone, so
//     sqrt(min d^2) == min sqrt(d^2) bit for bit;
//   - each thread carries kIngestPixels pixels, so one LDS read serves two pixels (as compiled: 24 VALU instructions per side for the
//     two pixels next to one ds_read_b128 and one ds_read_b32; how much of the issue the LDS reads take has not been measured with counters);
//   - a pixel's results stay in registers in groups of four instances and leave as ONE 16-byte store when the row stride allows it; the
//     row maximum is folded into the same pass (all values are >= +0, so starting from 0 it is bit-equal to amax of what was written).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vsrd {

constexpr int kIngestThreads = 256;
constexpr int kIngestPixels = 2;         // pixels per thread
constexpr int kIngestChunk = 256;        // polygon sides staged per pass (one per thread); longer polygons take several passes

// (xmin, ymin, xmax, ymax) of the set bits of every visible (view, slot) as inclusive pixel indices, visibility, and the table's repair:
// an entry without a set bit, or one that does not address the pack, becomes -1, which is what the pixel pass then sees.
__global__ __launch_bounds__(kIngestThreads) void frame_ingest_boxes_kernel(
    int* __restrict__ table, const int* __restrict__ polygon_offsets, int num_entries, int num_vertices,
    const unsigned char* __restrict__ inside, int height, int width, int num_instances, int target_stride,
    float* __restrict__ gt_boxes, unsigned char* __restrict__ visible) {
    __shared__ int reduce[4][kIngestThreads];
    const int v = blockIdx.y, n = blockIdx.x, t = threadIdx.x;
    int e = table[v * num_instances + n];
    if (e >= num_entries) e = -1;
    if (e >= 0) {
        const int first = polygon_offsets[e], last = polygon_offsets[e + 1];
        if (first < 0 || last > num_vertices || last <= first) e = -1;
    }
    const int row_bytes = (width + 7) >> 3;
    int xmin = width, ymin = height, xmax = -1, ymax = -1;
    if (e >= 0) {
        const unsigned char* bits = inside + static_cast<size_t>(e) * height * row_bytes;
        const unsigned tail_mask = (0xFFu << (row_bytes * 8 - width)) & 0xFFu;           // (the last byte of a row: bits past the width do not count)
        const int total = height * row_bytes;
        for (int i = t; i < total; i += kIngestThreads) {
            const int y = i / row_bytes, column = i - y * row_bytes;
            unsigned byte = bits[i];
            if (column == row_bytes - 1) byte &= tail_mask;
            if (byte) {
                const int lo = column * 8 + (__clz(static_cast<int>(byte)) - 24);          // most significant bit first
                const int hi = column * 8 + 7 - (__ffs(static_cast<int>(byte)) - 1);
                xmin = min(xmin, lo); xmax = max(xmax, hi);
                ymin = min(ymin, y); ymax = max(ymax, y);
            }
        }
    }
    reduce[0][t] = xmin; reduce[1][t] = ymin; reduce[2][t] = -xmax; reduce[3][t] = -ymax;
    __syncthreads();
    for (int half = kIngestThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int k = 0; k < 4; ++k) reduce[k][t] = min(reduce[k][t], reduce[k][t + half]);
        }
        __syncthreads();
    }
    if (t == 0) {
        const bool seen = e >= 0 && reduce[2][0] <= 0;
        if (!seen) table[v * num_instances + n] = -1;
        const size_t slot = static_cast<size_t>(v) * target_stride + n;
        if (visible) visible[slot] = seen ? 1 : 0;
        if (gt_boxes) {
            gt_boxes[slot * 4 + 0] = seen ? static_cast<float>(reduce[0][0]) : 0.0f;
            gt_boxes[slot * 4 + 1] = seen ? static_cast<float>(reduce[1][0]) : 0.0f;
            gt_boxes[slot * 4 + 2] = seen ? static_cast<float>(-reduce[2][0]) : 0.0f;
            gt_boxes[slot * 4 + 3] = seen ? static_cast<float>(-reduce[3][0]) : 0.0f;
        }
    }
}

// The pixel pass (see the head of the file).  kVector: target_stride % 4 == 0 and a 16-byte aligned soft_masks.
template <bool kVector>
__global__ __launch_bounds__(kIngestThreads) void frame_ingest_pixels_kernel(
    const int* __restrict__ table, const int* __restrict__ polygon_offsets, const int* __restrict__ vertices,
    const unsigned char* __restrict__ inside, int height, int width, int num_instances, int target_stride, float temperature,
    float* __restrict__ soft_masks, float* __restrict__ sampling_weights) {
    __shared__ float4 side_lds[kIngestChunk];        // start vertex (x, y), side vector (x, y)
    __shared__ float scale_lds[kIngestChunk];        // 1 / (|side|^2 + 1e-6)
    const int v = blockIdx.y, t = threadIdx.x;
    const int pixels = height * width;
    const int row_bytes = (width + 7) >> 3;
    int pixel[kIngestPixels], byte_of[kIngestPixels], shift_of[kIngestPixels];
    float px[kIngestPixels], py[kIngestPixels], row_max[kIngestPixels];
    bool live[kIngestPixels];
#pragma unroll
    for (int p = 0; p < kIngestPixels; ++p) {
        const int idx = (blockIdx.x * kIngestPixels + p) * kIngestThreads + t;
        live[p] = idx < pixels;
        pixel[p] = live[p] ? idx : pixels - 1;          // (every thread walks every barrier: a pixel past the end recomputes the last one and stores nothing)
        const int y = pixel[p] / width, x = pixel[p] - y * width;
        px[p] = static_cast<float>(x); py[p] = static_cast<float>(y);
        byte_of[p] = y * row_bytes + (x >> 3);
        shift_of[p] = 7 - (x & 7);
        row_max[p] = 0.0f;
    }
    for (int first = 0; first < num_instances; first += 4) {
        float out[kIngestPixels][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = first + j;
            const int e = n < num_instances ? table[v * num_instances + n] : -1;      // uniform over the workgroup
#pragma unroll
            for (int p = 0; p < kIngestPixels; ++p) out[p][j] = 0.0f;                  // an invisible pair: exactly 0 (main.py:204-265 pads with zeros)
            if (e < 0) continue;
            const int offset = polygon_offsets[e], count = polygon_offsets[e + 1] - offset;
            float best[kIngestPixels];
#pragma unroll
            for (int p = 0; p < kIngestPixels; ++p) best[p] = 3.0e38f;
            for (int chunk = 0; chunk < count; chunk += kIngestChunk) {
                const int staged = min(kIngestChunk, count - chunk);
                __syncthreads();                                                         // (the previous chunk has been read)
                if (t < staged) {
                    const int k = chunk + t, next = (k + 1 == count) ? 0 : k + 1;      // torch.roll(polygons, -1)
                    const float ax = static_cast<float>(vertices[2 * (offset + k)]), ay = static_cast<float>(vertices[2 * (offset + k) + 1]);
                    const float sx = static_cast<float>(vertices[2 * (offset + next)]) - ax, sy = static_cast<float>(vertices[2 * (offset + next) + 1]) - ay;
                    side_lds[t] = make_float4(ax, ay, sx, sy);
                    scale_lds[t] = 1.0f / (sx * sx + sy * sy + 1.0e-6f);
                }
                __syncthreads();
                for (int k = 0; k < staged; ++k) {
                    const float4 s = side_lds[k];
                    const float scale = scale_lds[k];
#pragma unroll
                    for (int p = 0; p < kIngestPixels; ++p) {
                        const float rx = px[p] - s.x, ry = py[p] - s.y;
                        const float ratio = fminf(fmaxf((s.z * rx + s.w * ry) * scale, 0.0f), 1.0f);
                        const float nx = rx - s.z * ratio, ny = ry - s.w * ratio;
                        best[p] = fminf(best[p], nx * nx + ny * ny);
                    }
                }
            }
            const unsigned char* bits = inside + static_cast<size_t>(e) * height * row_bytes;
#pragma unroll
            for (int p = 0; p < kIngestPixels; ++p) {
                const float distance = sqrtf(best[p]);
                const float sdf = ((bits[byte_of[p]] >> shift_of[p]) & 1) ? distance : -distance;
                out[p][j] = 1.0f / (1.0f + expf(-sdf / temperature));
                row_max[p] = fmaxf(row_max[p], out[p][j]);
            }
        }
        if (soft_masks) {
#pragma unroll
            for (int p = 0; p < kIngestPixels; ++p) {
                if (!live[p]) continue;
                float* row = soft_masks + (static_cast<size_t>(v) * pixels + pixel[p]) * target_stride + first;
                if (kVector && first + 4 <= num_instances) {
                    *reinterpret_cast<float4*>(row) = make_float4(out[p][0], out[p][1], out[p][2], out[p][3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (first + j < num_instances) row[j] = out[p][j];              // (columns N .. stride - 1 are never written)
                }
            }
        }
    }
    if (sampling_weights) {
#pragma unroll
        for (int p = 0; p < kIngestPixels; ++p)
            if (live[p]) sampling_weights[static_cast<size_t>(v) * pixels + pixel[p]] = row_max[p];
    }
}

}  // namespace vsrd
