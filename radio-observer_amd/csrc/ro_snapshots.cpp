// ro_snapshots.cpp -- the row ring in HBM and the event snapshots cut from it (include/ro_stft.h; kernels: ro_snapshots.hip):
// argument checks, the handle's scratch, the launches.  Nothing here reads device memory: the number of events, what is
// complete and where it goes in the arena are decided on the device.
#include "ro_host.h"

using namespace ro::host;

extern "C" int ro_stft_ring_put_resident(ro_stft_t *h, const float *d_image, int64_t image_stride, int64_t first_row,
                                         int64_t rows, const ro_row_ring_t *ring, void *stream)
{
    const char *who = "ro_stft_ring_put_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    const int rc = ring_check(who, ring);
    if (rc != RO_OK) return rc;
    if (!d_image) return fail(RO_ERR_INVALID, "%s: null d_image", who);
    if (first_row < 0 || rows < 0)
        return fail(RO_ERR_INVALID, "%s: first_row %lld, rows %lld: neither may be negative", who, (long long)first_row,
                    (long long)rows);
    if (image_stride < ring->cols)
        return fail(RO_ERR_INVALID, "%s: image_stride %lld < the ring's %d columns", who, (long long)image_stride, ring->cols);
    if (rows == 0) return RO_OK;
    HIP_TRY(hipSetDevice(h->device));
    // more rows than slots: the earlier ones would be overwritten by this very call, so they are left out and every slot is
    // stored once
    const int64_t skip = rows > ring->ring_rows ? rows - ring->ring_rows : 0;
    ro::RingPutArgs a{};
    a.image = d_image + skip * image_stride;
    a.ring = ring->d_rows;
    a.image_stride = image_stride;
    a.ring_stride = ring->stride;
    a.first_row = first_row + skip;
    a.rows = rows - skip;
    a.ring_rows = ring->ring_rows;
    a.cols = ring->cols;
    HIP_TRY(ro::launch_ring_put(a, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_stft_snapshots_resident(ro_stft_t *h, const ro_event_t *d_events, int64_t capacity,
                                          const ro_detect_summary_t *d_summary, uint32_t slot_mask,
                                          const int32_t *snapshot_rows, const ro_row_ring_t *ring, int64_t head_row,
                                          ro_event_t *d_pending, int64_t *d_pending_count, int64_t pending_capacity,
                                          ro_snapshot_t *d_dir, float *d_arena, int64_t arena_floats,
                                          ro_snap_summary_t *d_snap_summary, void *stream)
{
    const char *who = "ro_stft_snapshots_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    int slots = 0;
    const int rc = snapshots_check(who, "d_", d_events, capacity, d_summary, slot_mask, snapshot_rows, ring, head_row, d_pending,
                                   d_pending_count, pending_capacity, d_dir, d_arena, arena_floats, d_snap_summary, &slots);
    if (rc != RO_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const size_t need = ro::snap_scratch_bytes(slots, capacity, pending_capacity);
    if (h->d_snap_scratch.count() < need) {
        if (h->d_snap_scratch) HIP_TRY(hipDeviceSynchronize());   // (an earlier launch may still be using the old block)
        HIP_TRY(h->d_snap_scratch.alloc(need));
    }
    ro::SnapArgs a{};
    a.events = d_events;
    a.summary = d_summary;
    a.capacity = capacity;
    a.slot_mask = slot_mask;
    a.slots = slots;
    for (int s = 0; s < slots; ++s) a.snapshot_rows[s] = ((slot_mask >> s) & 1u) ? snapshot_rows[s] : 1;
    a.ring = ring->d_rows;
    a.ring_stride = ring->stride;
    a.ring_rows = ring->ring_rows;
    a.cols = ring->cols;
    a.head_row = head_row;
    a.pending = d_pending;
    a.pending_count = d_pending_count;
    a.pending_capacity = pending_capacity;
    a.dir = d_dir;
    a.arena = d_arena;
    a.arena_floats = arena_floats;
    a.arena_rows = arena_floats / ring->cols;
    a.snap_summary = d_snap_summary;
    ro::snap_scratch_layout(a, h->d_snap_scratch);
    HIP_TRY(ro::launch_snapshots(a, (hipStream_t)stream));
    return RO_OK;
}
