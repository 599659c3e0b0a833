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

// the copy on `s`: one launch, none when there are no blocks; cus: the device's compute units (the grid is at most four
// workgroups for each)
hipError_t launch_periodic(const PeriodicArgs &a, int cus, hipStream_t s);

}  // namespace ro
