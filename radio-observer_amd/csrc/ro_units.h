// ro_units.h -- the events' files on the device (ro_units.hip): the FITS data unit of every captured snapshot and of every
// captured raw run, cut to the firing recorder's columns, byte-swapped and zero-padded to 2880 bytes, packed into one buffer
// with a directory (what the worker and FITSWriter make of an image, src/WaterfallBackend.cpp:176-177, :202-205, :235,
// :258-261, src/FITSWriter.cpp).  include/ro_stft.h states the rules entry by entry; this header has what the host side
// needs to launch the kernels, and the entry rules the host twins (ro_units.cpp) share with them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"

// entries of one tile of units_plan_kernel: one per lane of its one workgroup, four waves
#define RO_UNITS_TILE 256
// floats of one block of units_copy_kernel: one FITS block, what one wave copies at a time; a block belongs to one unit
#define RO_UNITS_BLOCK_FLOATS (RO_FITS_BLOCK / 4)

namespace ro {

constexpr int64_t UNITS_MAX_ENTRIES = (int64_t)1 << 24;
constexpr int UNIT_SLOTS = 1 + RO_MAX_EXTRA_BANDS;

// What one source entry asks for, before the room is looked at: status RO_UNIT_SKIPPED or RO_UNIT_INVALID, or
// RO_UNIT_WRITTEN for a writable one with its shape and the arena float its first float is.
struct UnitWant {
    int32_t status;
    int32_t naxis1;
    int64_t naxis2;
    int64_t first;                 // arena float of the unit's float 0
};

// rule 2 of both calls: `count` floats at `offset` lie inside [0, arena_floats) (no sum that could overflow)
__host__ __device__ inline bool unit_inside(int64_t offset, int64_t count, int64_t arena_floats)
{
    return offset >= 0 && offset <= arena_floats && count <= arena_floats - offset;
}

// an image: win_first / win_cols are slot `slot`'s window, looked up by the caller (only when slot_ok)
__host__ __device__ inline UnitWant unit_want_image(int32_t status, int32_t slot, int32_t rows, int64_t offset, int32_t cols,
                                                    int64_t arena_floats, int32_t win_first, int32_t win_cols)
{
    UnitWant w = {RO_UNIT_SKIPPED, 0, 0, 0};
    if (status != RO_SNAP_CAPTURED) return w;
    w.status = RO_UNIT_INVALID;
    if (slot < 0 || slot >= UNIT_SLOTS || rows < 1 || !unit_inside(offset, (int64_t)rows * cols, arena_floats)) return w;
    w.status = RO_UNIT_SKIPPED;
    if (win_cols == 0) return w;
    w.status = RO_UNIT_WRITTEN;
    w.naxis1 = win_cols;
    w.naxis2 = rows;
    w.first = offset + win_first;
    return w;
}

// a raw run: 2 x samples
__host__ __device__ inline UnitWant unit_want_raw(int32_t status, int64_t samples, int64_t offset, int64_t arena_floats)
{
    UnitWant w = {RO_UNIT_SKIPPED, 0, 0, 0};
    if (status != RO_SNAP_CAPTURED) return w;
    w.status = RO_UNIT_INVALID;
    if (samples < 1 || offset < 0 || offset > arena_floats || samples > (arena_floats - offset) / 2) return w;
    w.status = RO_UNIT_WRITTEN;
    w.naxis1 = 2;
    w.naxis2 = samples;
    w.first = offset;
    return w;
}

// blocks of a writable entry (its floats lie inside the arena, which is real memory: 4 x them is far below 2^63)
__host__ __device__ inline int64_t unit_blocks(int32_t naxis1, int64_t naxis2)
{
    return (4 * (int64_t)naxis1 * naxis2 + RO_FITS_BLOCK - 1) / RO_FITS_BLOCK;
}

// units_plan_kernel -> units_copy_kernel: what there is to copy.  first_block[d] is the block of d_units where entry d's
// unit starts, or would start if it had one: the exclusive prefix of the writable entries' blocks, never descending.
// first_float[d] is the arena float that is float 0 of entry d's unit.
struct UnitsPlanHead {
    int64_t entries;               // entries of the unit directory and of the two tables
    int64_t blocks;                // blocks of all WRITTEN units
};

enum { UNITS_OF_IMAGES = 0, UNITS_OF_RAW = 1 };

struct UnitsArgs {
    const void          *dir;                  // ro_snapshot_t (images) or ro_raw_capture_t (raw), or null with dir_capacity 0
    const int64_t       *resolved;             // the source summary's first word
    int64_t              dir_capacity;
    const float         *arena;
    int64_t              arena_floats;
    int32_t              cols;                 // floats of one arena row (raw: 2)
    int32_t              win_first[UNIT_SLOTS], win_cols[UNIT_SLOTS];      // images
    ro_fits_unit_t      *unit_dir;
    char                *units;
    int64_t              units_bytes;
    ro_unit_summary_t   *summary;
    UnitsPlanHead       *head;                 // scratch
    int64_t             *first_block;          // scratch: [dir_capacity]
    int64_t             *first_float;          // scratch: [dir_capacity]
};

// bytes of scratch a call needs (8-byte aligned device memory), and its layout into head / first_block / first_float
size_t units_scratch_bytes(int64_t dir_capacity);
void units_scratch_layout(UnitsArgs &a, void *scratch);

// the plan and the copy on `s`: two launches; kind: UNITS_OF_IMAGES or UNITS_OF_RAW; cus: the device's compute units (the
// copy's grid is four workgroups for each)
hipError_t launch_units(const UnitsArgs &a, int kind, int cus, hipStream_t s);
// the plan alone, for a caller with a copy of its own (ro_levels.hip): a.units is not looked at, a.units_bytes is the room
hipError_t launch_units_plan(const UnitsArgs &a, int kind, hipStream_t s);

}  // namespace ro
