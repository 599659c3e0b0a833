// ro_raw.h -- the raw I/Q of each event on the device (ro_raw.hip): the samples behind every captured snapshot, cut out of
// the sample buffers the transform read and packed as (float)re, (float)im pairs into one arena with a directory (what
// writeRaw() writes for a snapshot with includeRawData, src/BolidRecorder.cpp:262, src/WaterfallBackend.cpp:77-81,
// :214-267).  include/ro_stft.h states the rules candidate by candidate; this header has what the host side needs to
// launch the kernels, and the arithmetic the host twin (ro_raw.cpp) shares with them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"

// candidates of one tile of raw_plan_kernel: one per lane of its one workgroup, four waves
#define RO_RAW_TILE 256
// pairs of one block of raw_copy_kernel: what one wave copies at a time, 64 lanes x 8 pairs in flight; a block belongs to
// one directory entry
#define RO_RAW_BLOCK 512

namespace ro {

constexpr int64_t RAW_MAX_CANDIDATES = (int64_t)1 << 24;

// fftSamplesToRaw of the recorder (src/WaterfallBackend.h:84-87): R = (int)fft_sample_rate, both as doubles here
__host__ __device__ inline int64_t raw_length(int64_t len, double rate_r, double sample_rate)
{
    return (int64_t)(((double)len / rate_r) * sample_rate);
}
// fftMarkToRaw(start): z = 1 without overlap, where the mark is read before the row's samples have moved on
__host__ __device__ inline int64_t raw_first_sample(int64_t start, int64_t hop, int64_t z)
{
    return start >= 1 ? (start - z) * hop + 1 : 0;
}

// raw_plan_kernel -> raw_copy_kernel: what there is to copy.  first_block[d] is the block (RO_RAW_BLOCK pairs of ONE
// entry; an entry's last block may be short) where raw directory entry d's run starts, or would start if it had samples:
// never descending.
struct RawPlanHead {
    int64_t resolved;              // entries of the raw directory and of first_block
    int64_t blocks;                // blocks of all captured runs
};

struct RawArgs {
    const ro_snapshot_t     *dir;              // the snapshots' directory, or null with dir_capacity 0
    const ro_snap_summary_t *snap_summary;
    int64_t              dir_capacity;
    const void          *iq[RO_MAX_IQ_SPANS];
    int64_t              first[RO_MAX_IQ_SPANS];       // stream index of a span's first sample ...
    int64_t              count[RO_MAX_IQ_SPANS];       // ... and how many it holds
    int32_t              format[RO_MAX_IQ_SPANS];
    int                  spans;
    int64_t              base_sample, head_sample;     // first[0], and the end of the last span
    int64_t              hop, z;
    double               rate_r, sample_rate;          // (int)fft_sample_rate and the sample rate
    ro_snapshot_t       *pending;                      // [pending_capacity], compacted in place
    int64_t             *pending_count;
    int64_t              pending_capacity;
    ro_raw_capture_t    *raw_dir;
    float               *arena;
    int64_t              arena_floats;
    ro_raw_summary_t    *raw_summary;
    RawPlanHead         *head;                         // scratch
    int64_t             *first_block;                  // scratch: [pending_capacity + dir_capacity]
};

// bytes of scratch a call needs (8-byte aligned device memory), and its layout into head / first_block
size_t raw_scratch_bytes(int64_t dir_capacity, int64_t pending_capacity);
void raw_scratch_layout(RawArgs &a, void *scratch);

// the plan and the copy on `s`: two launches; cus: the device's compute units (the copy's grid is four workgroups for each)
hipError_t launch_raw(const RawArgs &a, int cus, hipStream_t s);

}  // namespace ro
