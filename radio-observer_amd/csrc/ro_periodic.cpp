// ro_periodic.cpp -- the periodic snapshots (include/ro_stft.h; kernel: ro_periodic.hip): ro_snapshot_rows and
// ro_periodic_plan, the cadence of SnapshotRecorder::update / startWriting / stop in closed form, pure host arithmetic; the
// argument checks and the one launch of ro_stft_periodic_units_resident; and ro_periodic_units_host, the same rules entry by
// entry over host memory.  The resident call reads no device memory and the kernel no directory: what the directory says
// is folded into a few scalars per recorder here.
#include "ro_host.h"

using namespace ro::host;

static_assert(sizeof(ro_periodic_t) == 12 && sizeof(ro_periodic_entry_t) == 56 && sizeof(ro_periodic_summary_t) == 64 &&
                  offsetof(ro_periodic_entry_t, rows) == 40 && offsetof(ro_periodic_entry_t, status) == 52,
              "the periodic snapshots' structs are ABI");

namespace {

// what every call asks of the recorders, as a refusal in the name of `who`; cols: of a ring row
int recorders_check(const char *who, const ro_periodic_t *recorders, int count, int32_t cols)
{
    if (!recorders) return fail(RO_ERR_INVALID, "%s: null recorders", who);
    if (count < 1 || count > RO_MAX_PERIODIC)
        return fail(RO_ERR_INVALID, "%s: count %d: 1 ... %d recorders", who, count, RO_MAX_PERIODIC);
    for (int i = 0; i < count; ++i) {
        const ro_periodic_t &p = recorders[i];
        if (p.snapshot_rows < 1)
            return fail(RO_ERR_INVALID, "%s: recorders[%d]: snapshot_rows %d: at least 1", who, i, p.snapshot_rows);
        if (p.window.first_col < 0 || p.window.cols < 1 || (int64_t)p.window.first_col + p.window.cols > cols)
            return fail(RO_ERR_INVALID, "%s: recorders[%d]: window: columns [%d, +%d) do not lie inside the ring's %d", who, i,
                        p.window.first_col, p.window.cols, cols);
    }
    return RO_OK;
}

// The directory as the kernel takes it: the WRITTEN entries of each recorder as one run.  Refuses, in the name of `who`,
// a directory that is not what ro_periodic_plan writes for these recorders; room: the blocks the buffer holds, names and
// buf_bytes: how the refusal speaks of it
int runs_of(const char *who, const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
            const ro_periodic_entry_t *dir, int64_t entries, int64_t room, const PeriodicNames &names, int64_t buf_bytes,
            ro::PeriodicArgs *a)
{
    int64_t end = 0;                             // blocks of the WRITTEN entries so far
    bool full = false;                           // a NO_ROOM entry has been seen: nothing behind it is WRITTEN
    for (int64_t d = 0; d < entries; ++d) {
        const ro_periodic_entry_t &e = dir[d];
        const ro_periodic_entry_t *prev = d > 0 && dir[d - 1].recorder == e.recorder ? &dir[d - 1] : nullptr;
        if (e.recorder < 0 || e.recorder >= count || (d > 0 && e.recorder < dir[d - 1].recorder))
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: recorder %d: 0 ... %d, ascending", who, (long long)d, e.recorder, count - 1);
        const ro_periodic_t &p = recorders[e.recorder];
        const int64_t S = p.snapshot_rows;
        if (e.index < 0 || e.index > (INT64_MAX >> 1) / S || (prev && e.index != prev->index + 1) || e.first_row != e.index * S)
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: index %lld, first_row %lld: a recorder's indices are consecutive and "
                        "first_row is index x snapshot_rows (%d)", who, (long long)d, (long long)e.index, (long long)e.first_row,
                        p.snapshot_rows);
        if (e.status != RO_PERIODIC_WRITTEN && e.status != RO_PERIODIC_LOST && e.status != RO_PERIODIC_NO_ROOM)
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: status %d", who, (long long)d, e.status);
        if (e.rows < 1 || e.rows > S || (prev && prev->rows != S) || (e.status != RO_PERIODIC_LOST && e.rows > ring->ring_rows))
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: rows %d: snapshot_rows (%d) but for a recorder's last entry, and, unless LOST, at "
                        "most the ring's %lld", who, (long long)d, e.rows, p.snapshot_rows, (long long)ring->ring_rows);
        const int64_t bytes = e.status == RO_PERIODIC_LOST ? 0 : 4 * (int64_t)p.window.cols * e.rows;
        if (e.naxis1 != p.window.cols || e.bytes != bytes)
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: naxis1 %d, bytes %lld: the window has %d columns and the entry %d rows", who,
                        (long long)d, e.naxis1, (long long)e.bytes, p.window.cols, e.rows);
        if (e.status == RO_PERIODIC_NO_ROOM) full = true;
        if (e.status != RO_PERIODIC_WRITTEN) {
            if (e.offset != 0) return fail(RO_ERR_INVALID, "%s: dir[%lld]: offset %lld of an entry that is not WRITTEN", who,
                                           (long long)d, (long long)e.offset);
            continue;
        }
        const int64_t blocks = ro::periodic_blocks(e.naxis1, e.rows);
        if (full || e.offset != end * RO_FITS_BLOCK || blocks > room - end)
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: offset %lld: the WRITTEN entries are packed from 0 on in multiples of %d, "
                        "inside %s %lld%s, in front of every NO_ROOM one", who, (long long)d, (long long)e.offset,
                        RO_FITS_BLOCK, names.bytes, (long long)buf_bytes, names.room);
        ro::PeriodicRun &r = a->run[e.recorder];
        if (r.units == 0) {
            r.row0 = e.first_row;
            r.block0 = end;
            r.unit_blocks = ro::periodic_blocks(e.naxis1, S);
            r.snapshot_rows = p.snapshot_rows;
            r.first_col = p.window.first_col;
            r.naxis1 = e.naxis1;
        } else if (!prev || prev->status != RO_PERIODIC_WRITTEN)
            return fail(RO_ERR_INVALID, "%s: dir[%lld]: a recorder's WRITTEN entries follow one another", who, (long long)d);
        r.units += 1;
        r.last_rows = e.rows;
        end += blocks;
    }
    a->blocks = end;
    return RO_OK;
}

const PeriodicNames UNITS = {"units", "units_bytes", ""};

}  // namespace

namespace ro {
namespace host {

int periodic_check(const char *who, const char *d, const PeriodicNames &names, int64_t block, bool aligned,
                   const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count, const ro_periodic_entry_t *dir,
                   int64_t entries, void *buf, int64_t buf_bytes, ro::PeriodicArgs *a)
{
    int rc = ring_check(who, ring);
    if (rc != RO_OK) return rc;
    if ((rc = recorders_check(who, recorders, count, ring->cols)) != RO_OK) return rc;
    if (entries < 0 || buf_bytes < 0)
        return fail(RO_ERR_INVALID, "%s: entries %lld, %s %lld: neither may be negative", who, (long long)entries, names.bytes,
                    (long long)buf_bytes);
    if (entries > 0 && !dir) return fail(RO_ERR_INVALID, "%s: null dir with entries %lld", who, (long long)entries);
    if (buf_bytes > 0 && !buf)
        return fail(RO_ERR_INVALID, "%s: null %s%s with %s %lld", who, d, names.buf, names.bytes, (long long)buf_bytes);
    if (aligned && ((uintptr_t)buf & 15u) != 0) return fail(RO_ERR_INVALID, "%s: %s%s is not aligned to 16 bytes", who, d, names.buf);
    if (buf_bytes > 0) {
        const uintptr_t u = (uintptr_t)buf, r = (uintptr_t)ring->d_rows;
        const uintptr_t ring_bytes = 4 * (uintptr_t)((ring->ring_rows - 1) * ring->stride + ring->cols);
        if (u < r + ring_bytes && r < u + (uintptr_t)buf_bytes)
            return fail(RO_ERR_INVALID, "%s: %s%s overlaps the ring: the %s are written while the ring is read", who, d, names.buf,
                        names.buf);
    }
    a->ring = ring->d_rows;
    a->ring_stride = ring->stride;
    a->ring_rows = ring->ring_rows;
    a->cols = ring->cols;
    return runs_of(who, ring, recorders, count, dir, entries, buf_bytes / block, names, buf_bytes, a);
}

}  // namespace host
}  // namespace ro

extern "C" int ro_snapshot_rows(int sample_rate, int bins, int overlap, int snapshot_length)
{
    const float rate = ro_fft_sample_rate(sample_rate, bins, overlap);
    const int rows = (int)std::ceil(snapshot_length * rate);                    // src/WaterfallBackend.cpp:341-342: a float product
    return rows < 1 ? 1 : rows;                                                 // :343-345
}

// The cadence in closed form (include/ro_stft.h): snapshot k of a recorder is due iff (k + 1) S + 2 <= H, so floor((H - 2) / S)
// of them are; stop() adds [k' S, min((k' + 1) S, H)) for the first k' that is not due, unless it has no rows.
extern "C" int ro_periodic_plan(const ro_periodic_t *recorders, int count, int64_t *next_index, int64_t head_row, int final,
                                int64_t ring_rows, int32_t cols, int64_t units_bytes, ro_periodic_entry_t *dir,
                                int64_t capacity, ro_periodic_summary_t *summary)
{
    const char *who = "ro_periodic_plan";
    if (cols < 1) return fail(RO_ERR_INVALID, "%s: cols %d: a ring row has at least one float", who, cols);
    const int rc = recorders_check(who, recorders, count, cols);
    if (rc != RO_OK) return rc;
    if (!next_index || !summary) return fail(RO_ERR_INVALID, "%s: null %s", who, !next_index ? "next_index" : "summary");
    if (head_row < 0 || head_row > INT64_MAX >> 1 || units_bytes < 0 || capacity < 0)
        return fail(RO_ERR_INVALID, "%s: head_row %lld, units_bytes %lld, capacity %lld: none may be negative (head_row: at "
                    "most 2^62)", who, (long long)head_row, (long long)units_bytes, (long long)capacity);
    if (ring_rows < 1) return fail(RO_ERR_INVALID, "%s: ring_rows %lld: at least 1", who, (long long)ring_rows);
    if (capacity > 0 && !dir) return fail(RO_ERR_INVALID, "%s: null dir with capacity %lld", who, (long long)capacity);
    for (int i = 0; i < count; ++i)
        if (next_index[i] < 0 || next_index[i] > (INT64_MAX >> 1) / recorders[i].snapshot_rows - 1)
            return fail(RO_ERR_INVALID, "%s: next_index[%d] is %lld: not negative, and its rows below 2^62", who, i,
                        (long long)next_index[i]);
    ro_periodic_summary_t sum{};
    const int64_t room = units_bytes / RO_FITS_BLOCK;
    int64_t first_b = 0;                         // blocks of every writable candidate so far, fitting or not
    for (int i = 0; i < count; ++i) {
        const int64_t S = recorders[i].snapshot_rows;
        const int32_t naxis1 = recorders[i].window.cols;
        const int64_t due = head_row >= 2 ? (head_row - 2) / S : 0;            // snapshots 0 ... due - 1 are due
        const int64_t from = next_index[i];
        // stop(): the first snapshot that is not due.  A next_index beyond it says that stop() has been answered already
        const int64_t last_rows = final && from <= due ? std::min((due + 1) * S, head_row) - due * S : 0;
        const int64_t candidates = std::max<int64_t>(due - from, 0) + (last_rows > 0 ? 1 : 0);
        bool leading = true;                     // every candidate of this recorder so far has resolved
        int64_t c = 0;
        for (; c < candidates && sum.entries < capacity; ++c) {
            const int64_t k = from + c;
            ro_periodic_entry_t e{};
            e.index = k;
            e.first_row = k * S;
            e.rows = (int32_t)(k < due ? S : last_rows);
            e.due_row = k < due ? (k + 1) * S + 1 : head_row - 1;
            e.naxis1 = naxis1;
            e.recorder = i;
            if (e.first_row < head_row - ring_rows) {                           // rows have been overwritten
                e.status = RO_PERIODIC_LOST;
                sum.lost += 1;
            } else {
                const int64_t blocks = ro::periodic_blocks(naxis1, e.rows);
                e.bytes = 4 * (int64_t)naxis1 * e.rows;
                if (first_b + blocks <= room) {
                    e.status = RO_PERIODIC_WRITTEN;
                    e.offset = first_b * RO_FITS_BLOCK;
                    sum.written += 1;
                    sum.units_bytes = (first_b + blocks) * RO_FITS_BLOCK;
                } else {
                    e.status = RO_PERIODIC_NO_ROOM;
                    sum.no_room += 1;
                    leading = false;
                }
                first_b += blocks;
            }
            if (leading) next_index[i] = k + 1;
            dir[sum.entries++] = e;
        }
        sum.unlisted += candidates - c;
    }
    sum.needed_bytes = first_b * RO_FITS_BLOCK;
    *summary = sum;
    return RO_OK;
}

extern "C" int ro_stft_periodic_units_resident(ro_stft_t *h, const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                                               const ro_periodic_entry_t *dir, int64_t entries, void *d_units,
                                               int64_t units_bytes, void *stream)
{
    const char *who = "ro_stft_periodic_units_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    ro::PeriodicArgs a{};
    int rc = periodic_check(who, "d_", UNITS, RO_FITS_BLOCK, true, ring, recorders, count, dir, entries, d_units, units_bytes, &a);
    if (rc != RO_OK) return rc;
    a.units = static_cast<char *>(d_units);
    if (a.blocks == 0) return RO_OK;
    HIP_TRY(hipSetDevice(h->device));
    int cus = 0;
    if ((rc = device_cus(h, &cus)) != RO_OK) return rc;
    HIP_TRY(ro::launch_periodic(a, cus, (hipStream_t)stream));
    return RO_OK;
}

// the units on the host, entry by entry and float by float: the four bytes of ring float
// ((first_row + r) % ring_rows) stride + first_col + c, reversed
extern "C" int ro_periodic_units_host(const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                                      const ro_periodic_entry_t *dir, int64_t entries, void *units, int64_t units_bytes)
{
    ro::PeriodicArgs a{};
    const int rc = periodic_check("ro_periodic_units_host", "", UNITS, RO_FITS_BLOCK, false, ring, recorders, count, dir, entries, units,
                                  units_bytes, &a);
    if (rc != RO_OK) return rc;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(ring->d_rows);
    for (int64_t d = 0; d < entries; ++d) {
        const ro_periodic_entry_t &e = dir[d];
        if (e.status != RO_PERIODIC_WRITTEN) continue;
        const int64_t first_col = recorders[e.recorder].window.first_col;
        unsigned char *dst = static_cast<unsigned char *>(units) + e.offset;
        for (int64_t r = 0; r < e.rows; ++r) {
            const int64_t slot = (e.first_row + r) % ring->ring_rows;
            for (int64_t c = 0; c < e.naxis1; ++c, dst += 4) {
                const unsigned char *f = src + 4 * (slot * ring->stride + first_col + c);
                dst[0] = f[3];
                dst[1] = f[2];
                dst[2] = f[1];
                dst[3] = f[0];
            }
        }
        std::memset(dst, 0, (size_t)(ro::periodic_blocks(e.naxis1, e.rows) * RO_FITS_BLOCK - e.bytes));
    }
    return RO_OK;
}
