// ro_levels.h -- the grey-level previews on the device (ro_levels.hip): the viewer's ln image of every snapshot as one byte
// per pixel, zero-padded to RO_LEVEL_BLOCK bytes (fits2png:46, :444-445, :476-502), for the event snapshots of an arena and
// for the periodic snapshots of a plan.  include/ro_stft.h states the rules; this header has what the host side needs to
// launch the kernels.  A level image has as many 720-byte blocks as its FITS unit has 2880-byte ones, so the plans are the
// units' plans (ro_units.h, ro_periodic.h) with every offset divided by four.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"
#include "ro_periodic.h"
#include "ro_units.h"

namespace ro {

static_assert(4 * RO_LEVEL_BLOCK == RO_FITS_BLOCK, "a level block is a quarter of a FITS block: block b of the levels is block b of the units");

// reduce -> fold: the order keys (ro_device_util.h) of the min / max of logf over a block's non-zero pixels; {~0, 0}
// without one
struct LevelKeys {
    unsigned kmin, kmax;
};

// The event snapshots' call.  `plan` is what units_plan_kernel takes, in UNIT terms: its unit_dir and summary are scratch
// (the fold translates them into level_dir and level_summary), its units_bytes is 4 x levels_bytes and its units null
struct SnapshotLevelsArgs {
    UnitsArgs           plan;
    ro_fits_unit_t     *level_dir;
    ro_level_range_t   *ranges;
    char               *levels;
    int64_t             levels_bytes;
    ro_unit_summary_t  *level_summary;
    LevelKeys          *keys;                  // scratch: [levels_bytes / RO_LEVEL_BLOCK], block b's at [b]
};

// bytes of scratch a call needs (8-byte aligned device memory), and its layout into the plan's tables and the keys
size_t snapshot_levels_scratch_bytes(int64_t dir_capacity, int64_t levels_bytes);
void snapshot_levels_scratch_layout(SnapshotLevelsArgs &a, void *scratch);

// the plan (ro_units.hip's, launched from there), the reduce, the fold and the store on `s`; cus: the device's compute units
hipError_t launch_snapshot_levels(const SnapshotLevelsArgs &a, int cus, hipStream_t s);

// The periodic snapshots' call.  `p` is what periodic_copy_kernel takes (its units null): the runs.  The WRITTEN entries
// of run i are directory entries entry0[i], entry0[i] + 1, ...; unit0[i] counts the units of the runs in front of it
struct PeriodicLevelsArgs {
    PeriodicArgs        p;
    int64_t             entry0[RO_MAX_PERIODIC], unit0[RO_MAX_PERIODIC];
    int64_t             units;                 // of all runs
    ro_level_range_t   *ranges;
    char               *levels;
    LevelKeys          *keys;                  // scratch: [p.blocks]
};

// the reduce, the fold and the store on `s`; nothing when there are no blocks
hipError_t launch_periodic_levels(const PeriodicLevelsArgs &a, int cus, hipStream_t s);

}  // namespace ro
