// ro_events.h -- the detector on the device (ro_events.hip): the decision and the three-state machine of
// BolidRecorder::update (src/BolidRecorder.cpp:135, :171-267) as a scan over the scan records of up to 8 band sets.
// include/ro_stft.h states the machine's closed form; this header has what the host side needs to launch it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"

// rows of one slot that one workgroup reduces (pass 1) and emits (pass 3): one row per lane, four waves
#define RO_EVENTS_TILE_ROWS 256
// rows of one chunk: a call of more rows is cut into chunks that are chained through d_state on the stream.  The tiles of a
// chunk (1024) are what pass 2's one workgroup per slot scans, four per lane.
#define RO_EVENTS_CHUNK_ROWS 262144

namespace ro {

constexpr int EVENTS_MAX_SLOTS = 1 + RO_MAX_EXTRA_BANDS;
constexpr int EVENTS_MAX_TILES = RO_EVENTS_CHUNK_ROWS / RO_EVENTS_TILE_ROWS;

// pass 1 -> pass 2: a tile's total of the summary (first, last, gstart) as rows of the chunk counted from 1, all three 0
// for a tile without a detect row, and its counts.  `fires` are the fire rows the tile can tell by itself (the last detect
// row in front of them lies in the tile); pass 2 adds the one a group from before the tile may fire in it.
struct EventsTileTotal {
    int32_t first, last, gstart;
    int32_t fires, detect_rows, marginal_rows;
};
// pass 2 -> pass 3: the exclusive prefix of a tile, carried state included, in stream rows, and the events fired before it
// in this call
struct EventsTilePrefix {
    int64_t last, gstart;
    int64_t fires_before;
    int32_t open;                  // 0: the prefix is empty
    int32_t pad;
};
// per slot: the record of the state a chunk started from (pass 3 reads it for a group that began before the chunk, pass 2
// has overwritten d_state by then) and the call's counts up to and including this chunk
struct EventsSlotHead {
    float   noise;
    int32_t peak;
    float   magnitude;
    int32_t pad;
    int64_t events, detect_rows, marginal_rows;
};

// one chunk of at most RO_EVENTS_CHUNK_ROWS rows
struct EventsArgs {
    const ro_scan_record_t *primary;       // slot 0: rows records, or null
    const ro_scan_record_t *extra;         // slots 1 + s: [row][count] records, or null
    int                  count;            // extra sets of the handle
    int                  accumulate;       // 0: the call's first chunk (the counts start from zero)
    int64_t              first_row, rows;
    ro_detect_state_t   *state;            // [1 + count]
    ro_event_t          *events;           // [1 + count][capacity], or null
    int64_t              capacity;
    ro_detect_summary_t *summary;          // [1 + count], or null
    uint8_t             *detect;           // [rows][1 + count], or null
    EventsSlotHead      *heads;            // scratch: [EVENTS_MAX_SLOTS]
    EventsTileTotal     *totals;           // scratch: [EVENTS_MAX_SLOTS][EVENTS_MAX_TILES]
    EventsTilePrefix    *prefix;           // scratch: [EVENTS_MAX_SLOTS][EVENTS_MAX_TILES]
    ro_detector_t        det[EVENTS_MAX_SLOTS];
};

constexpr size_t EVENTS_SCRATCH_BYTES =
    EVENTS_MAX_SLOTS * (sizeof(EventsSlotHead) + EVENTS_MAX_TILES * (sizeof(EventsTileTotal) + sizeof(EventsTilePrefix)));

// scratch: EVENTS_SCRATCH_BYTES of device memory, 8-byte aligned; fills in heads / totals / prefix of `a`
void events_scratch_layout(EventsArgs &a, void *scratch);
// the three launches of one chunk on `s`
hipError_t launch_events(const EventsArgs &a, hipStream_t s);

}  // namespace ro
