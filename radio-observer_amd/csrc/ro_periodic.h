// ro_periodic.h -- the periodic snapshots' files on the device (ro_periodic.hip): the FITS data unit of every due snapshot
// of up to RO_MAX_PERIODIC always-on recorders, cut from the row ring's slots to the recorder's columns, byte-swapped and
// zero-padded to 2880 bytes (what SnapshotRecorder::update / startWriting / write and FITSWriter make of the ring,
// src/WaterfallBackend.cpp:415-427, :107-127, :141-211).  include/ro_stft.h states the cadence and the rules; the plan is
// host arithmetic (ro_periodic_plan, ro_periodic.cpp), and this header has what reaches the kernel: scalars only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"

// floats of one block of periodic_copy_kernel: one FITS block, what one wave copies at a time; a block belongs to one unit
#define RO_PERIODIC_BLOCK_FLOATS (RO_FITS_BLOCK / 4)

namespace ro {

// blocks of a unit of `rows` rows (4 x naxis1 x rows bytes of ring memory: far below 2^63)
__host__ __device__ inline int64_t periodic_blocks(int32_t naxis1, int64_t rows)
{
    return (4 * (int64_t)naxis1 * rows + RO_FITS_BLOCK - 1) / RO_FITS_BLOCK;
}

// The WRITTEN units of one recorder: `units` of them, back to back in d_units from block `block0` on.  Unit j is rows
// [row0 + j S, + S) -- the last one `last_rows` of them (S, or what a final snapshot has) -- and takes `unit_blocks` blocks
// (the last one what its rows need).  units == 0: the recorder has nothing in this launch.
struct PeriodicRun {
    int64_t row0;                  // first_row of the first written snapshot
    int64_t block0;                // block of d_units where its unit starts
    int64_t units;
    int64_t unit_blocks;           // of a unit of S rows
    int32_t snapshot_rows;         // S
    int32_t last_rows;             // 1 ... S
    int32_t first_col, naxis1;     // the window, in ring columns
};

struct PeriodicArgs {
    const float *ring;             // ring_rows x ring_stride floats; stream row r lives in slot r % ring_rows
    int64_t      ring_stride, ring_rows;
    int32_t      cols;             // floats of a slot that hold a row
    char        *units;
    int64_t      blocks;           // of all runs: work items [0, blocks); item b is block b of d_units
    PeriodicRun  run[RO_MAX_PERIODIC];         // in ascending block0; unused ones have units == 0
};

// (periodic_copy_kernel keeps its own text of the two device functions below: written through them hipcc allocates its
// registers differently, and its code object is to stay what it was.  ro_levels.hip's kernels use these.)
// the run of work item b among a.run: the last one that starts at or in front of it.  Runs without units are passed over.
// Which run it is takes two words of each; the run itself is then one scalar load from the kernel arguments (b is
// wave-uniform)
__device__ __forceinline__ int periodic_run_index(const PeriodicArgs &a, int64_t b)
{
    int at = 0;
#pragma unroll
    for (int i = 1; i < RO_MAX_PERIODIC; ++i) at = a.run[i].units > 0 && a.run[i].block0 <= b ? i : at;
    return at;
}

// The copy's gather out of the ring: float x of a unit's rows from the row in slot0 on -- x counts from that row's first
// window column on, a row of the unit is naxis1 floats -- clamped into [0, last].  A unit has at most ring_rows rows, so
// slot0 + x / naxis1 wraps at most once where the float is the unit's; the others are clamped and the caller masks them
__device__ __forceinline__ int64_t periodic_ring_at(int64_t ring_rows, int64_t ring_stride, int64_t slot0, unsigned x,
                                                    unsigned naxis1, int32_t first_col, int64_t last)
{
    const unsigned dr = x / naxis1;
    int64_t slot = slot0 + dr;
    slot = slot >= ring_rows ? slot - ring_rows : slot;
    const int64_t at = slot * ring_stride + first_col + (x - dr * naxis1);
    return at < 0 ? 0 : (at > last ? last : at);
}

// what a launch over the runs asks of them (host): the ring's shape, and runs that pack the blocks from 0 on to a.blocks
inline bool periodic_runs_ok(const PeriodicArgs &a)
{
    if (a.blocks < 0 || !a.ring || a.ring_rows < 1 || a.cols < 1 || a.ring_stride < a.cols) return false;
    int64_t end = 0;
    for (int i = 0; i < RO_MAX_PERIODIC; ++i) {
        const PeriodicRun &r = a.run[i];
        if (r.units == 0) continue;
        if (r.units < 0 || r.block0 != end || r.row0 < 0 || r.snapshot_rows < 1 ||
            (r.units > 1 ? r.snapshot_rows : r.last_rows) > a.ring_rows ||          // a unit's rows are in the ring at once
            r.last_rows < 1 || r.last_rows > r.snapshot_rows || r.first_col < 0 || r.naxis1 < 1 ||
            (int64_t)r.first_col + r.naxis1 > a.cols || r.unit_blocks != periodic_blocks(r.naxis1, r.snapshot_rows))
            return false;
        end += (r.units - 1) * r.unit_blocks + periodic_blocks(r.naxis1, r.last_rows);
    }
    return end == a.blocks;
}

// the copy on `s`: one launch, none when there are no blocks; cus: the device's compute units (the grid is at most four
// workgroups for each)
hipError_t launch_periodic(const PeriodicArgs &a, int cus, hipStream_t s);

}  // namespace ro
