// vsrd_frame_log: the scalar history and the step snapshots of a frame's optimisation, kept on the device -- what the reference's loop leaves
// behind every `scalar_intervals` and `ckpt_intervals` steps (scripts/main.py:870-953, 1109-1121) -- gathered by ONE launch between two
// replays of the step graphs and read by the host once, when the frame is finished.  Pure gather and copy: every value is moved as the 32
// bits it is, nothing is computed from it.
//
// Grid (blocks, frames), 256 threads.  Every block reads its frame's step counter once, as a wave-uniform scalar -- the int64 the epilogue
// increments: after step s it holds c = s + 1 -- and leaves at once when c sits on no boundary of either interval:
//
//   history    c % scalar_interval == 0: block 0's first wave writes row c / scalar_interval - 1, lane j scalar j of
//              (step | record[5] | *learning_rates[0..5) | schedule[3] | summary[8] or NaN);
//   snapshot   c % checkpoint_interval == 0: all blocks copy the segments of the frame's table into slot c / checkpoint_interval - 1 with
//              grid-stride 16-byte loads and stores; a segment's tail (count % 4 dwords), and a whole segment whose source or destination is
//              not 16-byte aligned, go through dword copies.
//
// A row or slot at or beyond its capacity is dropped and counted.  Block 0's thread 0 is the one writer of a frame's four counters and of
// snapshot_steps; no other thread of the launch reads them.  A segment that does not fit the slot (negative count or offset, offset + count
// beyond snapshot_floats) is skipped: the launch writes nothing outside the frame's history rows and snapshot slots.  No LDS.
#pragma once
#include "wave.h"

namespace vsrd {

constexpr int kLogScalars = 22;          // VSRD_LOG_SCALARS
constexpr int kLogMaxSegments = 32;      // VSRD_LOG_MAX_SEGMENTS
constexpr int kLogThreads = 256;
constexpr int kLogMaxBlocks = 64;        // per frame: one pass of the grid moves 64 x 256 x 16 bytes = 256 KiB

struct LogSegment {                      // vsrd_log_segment
    const unsigned* source;
    long long count;                     // dwords
    long long offset;                    // dwords, inside a slot
};

struct LogArgs {
    int scalar_interval, checkpoint_interval;
    int history_capacity, snapshot_capacity;
    long long snapshot_floats;
    int num_segments;
    long long frame_stride;
    const long long* step;               // [1]
    const unsigned* record;              // [5]
    const unsigned* const* learning_rates;   // [5] pointers
    const unsigned* schedule;            // [3]
    const unsigned* summary;             // [8] or null
    const LogSegment* segments;          // [num_segments]
    unsigned* history;                   // [history_capacity, kLogScalars]
    unsigned* snapshots;                 // [snapshot_capacity, snapshot_floats]
    int* snapshot_steps;                 // [snapshot_capacity]
    int* counters;                       // [4] = rows_written, rows_dropped, slots_written, slots_dropped
};

__device__ __forceinline__ void shift_frame(LogArgs& a, long long shift) {
    a.step = of_frame(a.step, shift); a.record = of_frame(a.record, shift); a.learning_rates = of_frame(a.learning_rates, shift);
    a.schedule = of_frame(a.schedule, shift); a.summary = of_frame(a.summary, shift); a.segments = of_frame(a.segments, shift);
    a.history = of_frame(a.history, shift); a.snapshots = of_frame(a.snapshots, shift); a.snapshot_steps = of_frame(a.snapshot_steps, shift);
    a.counters = of_frame(a.counters, shift);
}

__global__ __launch_bounds__(kLogThreads) void frame_log_kernel(LogArgs a) {
    if (a.frame_stride != 0) shift_frame(a, frame_shift(a.frame_stride, blockIdx.y));     // a batch of frames (wave.h)
    const long long c = *a.step;         // (a uniform address: a scalar load)
    const bool logs = a.scalar_interval > 0 && c > 0 && c % a.scalar_interval == 0;
    const bool snaps = a.checkpoint_interval > 0 && c > 0 && c % a.checkpoint_interval == 0;
    if (!logs && !snaps) return;
    const long long row = logs ? c / a.scalar_interval - 1 : 0, slot = snaps ? c / a.checkpoint_interval - 1 : 0;
    const bool row_fits = logs && row < a.history_capacity, slot_fits = snaps && slot < a.snapshot_capacity;
    const int thread = static_cast<int>(threadIdx.x);
    if (blockIdx.x == 0) {
        if (thread == 0) {               // the frame's counters: one writer
            if (logs) {
                if (row_fits) { if (a.counters[0] < row + 1) a.counters[0] = static_cast<int>(row + 1); }
                else a.counters[1] += 1;
            }
            if (snaps) {
                if (slot_fits) {
                    if (a.counters[2] < slot + 1) a.counters[2] = static_cast<int>(slot + 1);
                    a.snapshot_steps[slot] = static_cast<int>(c - 1);
                } else a.counters[3] += 1;
            }
        }
        if (row_fits && thread < kLogScalars) {          // lane j copies scalar j
            unsigned value;
            if (thread == 0) value = static_cast<unsigned>(static_cast<int>(c - 1));
            else if (thread < 6) value = a.record[thread - 1];
            else if (thread < 11) value = a.learning_rates[thread - 6][0];
            else if (thread < 14) value = a.schedule[thread - 11];
            else value = a.summary ? a.summary[thread - 14] : 0x7fc00000u;
            a.history[row * kLogScalars + thread] = value;
        }
    }
    if (!slot_fits) return;
    unsigned* const base = a.snapshots + slot * a.snapshot_floats;
    const long long first = static_cast<long long>(blockIdx.x) * kLogThreads + thread, stride = static_cast<long long>(gridDim.x) * kLogThreads;
    for (int s = 0; s < a.num_segments; ++s) {
        const LogSegment segment = a.segments[s];
        if (segment.source == nullptr || segment.count <= 0 || segment.offset < 0 || segment.count > a.snapshot_floats - segment.offset) continue;
        const unsigned* const source = segment.source;
        unsigned* const target = base + segment.offset;
        const bool aligned = ((reinterpret_cast<unsigned long long>(source) | reinterpret_cast<unsigned long long>(target)) & 15ull) == 0;
        const long long body = aligned ? segment.count & ~3ll : 0;
        const uint4* const source4 = reinterpret_cast<const uint4*>(source);
        uint4* const target4 = reinterpret_cast<uint4*>(target);
        for (long long i = first; i < body / 4; i += stride) target4[i] = source4[i];
        for (long long i = body + first; i < segment.count; i += stride) target[i] = source[i];
    }
}

}  // namespace vsrd
