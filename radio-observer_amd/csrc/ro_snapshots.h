// ro_snapshots.h -- event snapshots on the device (ro_snapshots.hip): rows into a row ring in HBM, and the rows of every
// complete event's snapshot out of it into one arena with a directory (the end of BolidRecorder's METEOR DETECTED branch,
// src/BolidRecorder.cpp:262-263, and the reservation of src/WaterfallBackend.cpp:107-127).  include/ro_stft.h states the
// rules candidate by candidate; this header has what the host side needs to launch the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"

// candidates of one tile of snap_plan_kernel: one per lane of its one workgroup, four waves
#define RO_SNAP_TILE 256

namespace ro {

constexpr int SNAP_MAX_SLOTS = 1 + RO_MAX_EXTRA_BANDS;
constexpr int64_t SNAP_MAX_CANDIDATES = (int64_t)1 << 24;

// rows of `image` into their ring slots
struct RingPutArgs {
    const float *image;            // rows x image_stride
    float       *ring;             // ring_rows x ring_stride
    int64_t      image_stride, ring_stride;
    int64_t      first_row;        // stream row of image row 0
    int64_t      rows;             // 1 ... ring_rows (the caller has dropped the rows a later one overwrites)
    int64_t      ring_rows;
    int          cols;
};

// snap_plan_kernel -> snap_copy_kernel: what there is to copy.  first_packed[d] is the packed row (a row of the arena, cols
// floats each) where directory entry d's image starts, or would start if it had rows: never descending.
struct SnapPlanHead {
    int64_t resolved;              // entries of the directory and of first_packed
    int64_t packed_rows;           // rows of all captured images
};

struct SnapArgs {
    const ro_event_t          *events;         // [slot][capacity], or null with capacity 0
    const ro_detect_summary_t *summary;        // [slot], or null: no events are read
    int64_t              capacity;
    unsigned             slot_mask;
    int                  slots;                // highest bit of the mask + 1
    int32_t              snapshot_rows[SNAP_MAX_SLOTS];
    const float         *ring;
    int64_t              ring_stride, ring_rows;
    int                  cols;
    int64_t              head_row;
    ro_event_t          *pending;              // [slots][pending_capacity]
    int64_t             *pending_count;        // [slots]
    int64_t              pending_capacity;
    ro_snapshot_t       *dir;
    float               *arena;
    int64_t              arena_floats;
    int64_t              arena_rows;           // arena_floats / cols
    ro_snap_summary_t   *snap_summary;
    SnapPlanHead        *head;                 // scratch
    int64_t             *first_packed;         // scratch: [slots x (capacity + pending_capacity)]
    ro_event_t          *pending_new;          // scratch: [slots][pending_capacity], the compacted lists before they go back
};

// bytes of scratch a call needs (8-byte aligned device memory), and its layout into head / first_packed / pending_new
size_t snap_scratch_bytes(int slots, int64_t capacity, int64_t pending_capacity);
void snap_scratch_layout(SnapArgs &a, void *scratch);

// one launch on `s`
hipError_t launch_ring_put(const RingPutArgs &a, hipStream_t s);
// the plan and the copy on `s`: two launches; cus: the device's compute units (the copy's grid is four workgroups for each)
hipError_t launch_snapshots(const SnapArgs &a, int cus, hipStream_t s);

}  // namespace ro
