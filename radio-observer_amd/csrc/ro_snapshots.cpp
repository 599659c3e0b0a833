// ro_snapshots.cpp -- the row ring in HBM and the event snapshots cut from it (include/ro_stft.h; kernels: ro_snapshots.hip):
// argument checks, the handle's scratch, the launches; and ro_snapshots_host, the same rules candidate by candidate over host
// memory.  Nothing in the resident calls reads device memory: the number of events, what is complete and where it goes in the
// arena are decided on the device.
#include "ro_host.h"

using namespace ro::host;

static_assert(sizeof(ro_row_ring_t) == 32 && sizeof(ro_snapshot_t) == 72 && sizeof(ro_snap_summary_t) == 64,
              "the snapshots' structs are ABI");

// what the calls ask of a ring (null: refused too), as a refusal in the name of `who` (ro_periodic.cpp asks the same)
int ro::host::ring_check(const char *who, const ro_row_ring_t *ring)
{
    if (!ring) return fail(RO_ERR_INVALID, "%s: null ring", who);
    if (!ring->d_rows) return fail(RO_ERR_INVALID, "%s: ring: null d_rows", who);
    if (ring->ring_rows < 1 || ring->cols < 1 || ring->stride < ring->cols || ring->reserved != 0)
        return fail(RO_ERR_INVALID, "%s: ring: ring_rows %lld, cols %d, stride %lld, reserved %d: needs ring_rows >= 1, "
                    "cols >= 1, stride >= cols, reserved 0", who, (long long)ring->ring_rows, ring->cols, (long long)ring->stride,
                    ring->reserved);
    return RO_OK;
}

namespace {

// what ro_snapshots_host and ro_stft_snapshots_resident ask of their common arguments, as a refusal in the name of `who`;
// d: "d_" where the arrays are the device's (the argument names of the resident call), "" on the host.  *slots: the mask's
// highest bit + 1
int snapshots_check(const char *who, const char *d, const ro_event_t *events, int64_t capacity,
                    const ro_detect_summary_t *summary, uint32_t slot_mask, const int32_t *snapshot_rows,
                    const ro_row_ring_t *ring, int64_t head_row, const ro_event_t *pending, const int64_t *pending_count,
                    int64_t pending_capacity, const ro_snapshot_t *dir, const float *arena, int64_t arena_floats,
                    const ro_snap_summary_t *snap_summary, int *slots)
{
    const int rc = ring_check(who, ring);
    if (rc != RO_OK) return rc;
    if (capacity < 0 || pending_capacity < 0 || arena_floats < 0 || head_row < 0)
        return fail(RO_ERR_INVALID, "%s: capacity %lld, pending_capacity %lld, arena_floats %lld, head_row %lld: none may be "
                    "negative", who, (long long)capacity, (long long)pending_capacity, (long long)arena_floats, (long long)head_row);
    if (slot_mask == 0u || (slot_mask >> (1 + RO_MAX_EXTRA_BANDS)) != 0u)
        return fail(RO_ERR_INVALID, "%s: slot_mask 0x%x: needs at least one of the bits 0 ... %d and no other", who, slot_mask,
                    RO_MAX_EXTRA_BANDS);
    if (!snapshot_rows) return fail(RO_ERR_INVALID, "%s: null snapshot_rows", who);
    if (!pending_count) return fail(RO_ERR_INVALID, "%s: null %spending_count", who, d);
    if (pending_capacity > 0 && !pending)
        return fail(RO_ERR_INVALID, "%s: null %spending with pending_capacity %lld", who, d, (long long)pending_capacity);
    if (!dir || !snap_summary) return fail(RO_ERR_INVALID, "%s: null %s%s", who, d, !dir ? "dir" : "snap_summary");
    if (capacity > 0 && (!events || !summary))
        return fail(RO_ERR_INVALID, "%s: null %s%s with capacity %lld", who, d, !events ? "events" : "summary", (long long)capacity);
    if (arena_floats > 0 && !arena)
        return fail(RO_ERR_INVALID, "%s: null %sarena with arena_floats %lld", who, d, (long long)arena_floats);
    int n = 0, masked = 0;
    for (int s = 0; s <= RO_MAX_EXTRA_BANDS; ++s)
        if ((slot_mask >> s) & 1u) {
            n = s + 1;
            masked += 1;
            if (snapshot_rows[s] < 1)
                return fail(RO_ERR_INVALID, "%s: snapshot_rows[%d] is %d: at least 1", who, s, snapshot_rows[s]);
        }
    if (capacity > ro::SNAP_MAX_CANDIDATES || pending_capacity > ro::SNAP_MAX_CANDIDATES ||
        masked * (capacity + pending_capacity) > ro::SNAP_MAX_CANDIDATES)
        return fail(RO_ERR_INVALID, "%s: %d slots x (capacity %lld + pending_capacity %lld): more than 2^24 candidates", who,
                    masked, (long long)capacity, (long long)pending_capacity);
    *slots = n;
    return RO_OK;
}

}  // namespace

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
    int rc = snapshots_check(who, "d_", d_events, capacity, d_summary, slot_mask, snapshot_rows, ring, head_row, d_pending,
                                   d_pending_count, pending_capacity, d_dir, d_arena, arena_floats, d_snap_summary, &slots);
    if (rc != RO_OK) return rc;
    int cus = 0;
    if ((rc = scratch_for(h, h->d_snap_scratch, ro::snap_scratch_bytes(slots, capacity, pending_capacity), &cus)) != RO_OK) return rc;
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
    HIP_TRY(ro::launch_snapshots(a, cus, (hipStream_t)stream));
    return RO_OK;
}

// event snapshots on the host: the rules of include/ro_stft.h candidate by candidate (startWriting()'s clamp and reservation,
// src/WaterfallBackend.cpp:107-127, with the ring sized by the caller).  ro_snapshots.hip computes the same with scans.
extern "C" int ro_snapshots_host(const ro_event_t *events, int64_t capacity, const ro_detect_summary_t *summary,
                                 uint32_t slot_mask, const int32_t *snapshot_rows, const ro_row_ring_t *ring, int64_t head_row,
                                 ro_event_t *pending, int64_t *pending_count, int64_t pending_capacity, ro_snapshot_t *dir,
                                 float *arena, int64_t arena_floats, ro_snap_summary_t *snap_summary)
{
    int slots = 0;
    const int rc = snapshots_check("ro_snapshots_host", "", events, capacity, summary, slot_mask, snapshot_rows, ring, head_row,
                                   pending, pending_count, pending_capacity, dir, arena, arena_floats, snap_summary, &slots);
    if (rc != RO_OK) return rc;
    ro_snap_summary_t sum{};
    const int64_t cols = ring->cols;
    int64_t offset = 0;                          // floats of every capturable candidate so far, fitting or not
    bool full = false;                           // one did not fit: nothing behind it does (the prefix only grows)
    for (int s = 0; s < slots; ++s) {
        if (!((slot_mask >> s) & 1u)) continue;
        const int64_t have = std::min(std::max<int64_t>(pending_count[s], 0), pending_capacity);
        const int64_t fired = summary ? std::max<int64_t>(summary[s].events, 0) : 0;
        const int64_t listed = std::min(fired, capacity);
        sum.unlisted += fired - listed;
        ro_event_t *list = pending + s * pending_capacity;
        int64_t still = 0;                       // candidates that stay pending; the first pending_capacity are kept
        for (int64_t c = 0; c < have + listed; ++c) {
            // (a kept candidate lands at or in front of the place it was read from: the list is compacted in place)
            const ro_event_t e = c < have ? list[c] : events[s * capacity + (c - have)];
            const int64_t len = std::min<int64_t>(e.length, snapshot_rows[s]);           // :113-115: the first rows are kept
            const int64_t lo = std::max<int64_t>(e.start_row, 0), hi = e.start_row + len;
            int status = -1;
            int64_t size = 0;
            if (hi > head_row) status = -1;
            else if (hi <= lo) status = RO_SNAP_EMPTY;
            else if (lo < head_row - ring->ring_rows) status = RO_SNAP_LOST;
            else {
                size = (hi - lo) * cols;
                if (!full && size <= arena_floats - offset) status = RO_SNAP_CAPTURED;
                else full = true;
            }
            if (status < 0) {
                if (still < pending_capacity) list[still] = e;
                still += 1;
            } else {
                ro_snapshot_t &out = dir[sum.resolved++];
                out.event = e;
                out.first_row = lo;
                out.offset = status == RO_SNAP_CAPTURED ? offset : 0;
                out.rows = status == RO_SNAP_CAPTURED ? (int32_t)(hi - lo) : 0;
                out.slot = s;
                out.status = status;
                out.reserved = 0;
                if (status == RO_SNAP_CAPTURED) {
                    for (int64_t k = 0; k < hi - lo; ++k)
                        std::memcpy(arena + offset + k * cols, ring->d_rows + ((lo + k) % ring->ring_rows) * ring->stride,
                                    (size_t)cols * sizeof(float));
                    sum.captured += 1;
                    sum.arena_floats = offset + size;
                } else if (status == RO_SNAP_EMPTY) sum.empty += 1;
                else sum.lost += 1;
            }
            if (!full) offset += size;
        }
        const int64_t kept = std::min(still, pending_capacity);
        pending_count[s] = kept;
        sum.pending += kept;
        sum.pending_dropped += still - kept;
    }
    *snap_summary = sum;
    return RO_OK;
}
