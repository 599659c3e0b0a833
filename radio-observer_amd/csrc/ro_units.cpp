// ro_units.cpp -- the events' files as FITS data units (include/ro_stft.h; kernels: ro_units.hip): argument checks, the
// handle's scratch, the launches; and ro_snapshot_units_host / ro_raw_units_host, the same rules entry by entry over host
// memory.  Nothing in the resident calls reads device memory: how many entries there are, which of them get a unit and
// where it goes are decided on the device.
#include "ro_host.h"

using namespace ro::host;

static_assert(sizeof(ro_fits_unit_t) == 32 && sizeof(ro_unit_summary_t) == 64 && RO_FITS_BLOCK == 2880,
              "the units' structs are ABI");

namespace {

// what the four calls ask of their common arguments, as a refusal in the name of `who`; d: "d_" where the arrays are the
// device's (the argument names of the resident calls), "" on the host; raw: the directory is ro_raw_capture_t (no cols, no
// slot windows); aligned: the device's stores are 16 bytes wide
int units_check(const char *who, const char *d, bool raw, bool aligned, const void *dir, int64_t dir_capacity,
                const void *summary, const float *arena, int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows,
                const ro_fits_unit_t *unit_dir, const void *units, int64_t units_bytes, const ro_unit_summary_t *unit_summary)
{
    const char *dir_name = raw ? "raw_dir" : "dir", *sum_name = raw ? "raw_summary" : "snap_summary";
    if (dir_capacity < 0 || arena_floats < 0 || units_bytes < 0)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld, arena_floats %lld, units_bytes %lld: none may be negative", who,
                    (long long)dir_capacity, (long long)arena_floats, (long long)units_bytes);
    if (!summary) return fail(RO_ERR_INVALID, "%s: null %s%s", who, d, sum_name);
    if (dir_capacity > 0 && !dir)
        return fail(RO_ERR_INVALID, "%s: null %s%s with dir_capacity %lld", who, d, dir_name, (long long)dir_capacity);
    if (dir_capacity > ro::UNITS_MAX_ENTRIES)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld: more than 2^24 entries", who, (long long)dir_capacity);
    if (arena_floats > 0 && !arena)
        return fail(RO_ERR_INVALID, "%s: null %sarena with arena_floats %lld", who, d, (long long)arena_floats);
    if (!raw) {
        if (cols < 1) return fail(RO_ERR_INVALID, "%s: cols %d: an arena row has at least one float", who, cols);
        if (!slot_windows) return fail(RO_ERR_INVALID, "%s: null slot_windows", who);
        for (int i = 0; i < ro::UNIT_SLOTS; ++i) {
            const ro_band_window_t &w = slot_windows[i];
            if (w.first_col < 0 || w.cols < 0 || (int64_t)w.first_col + w.cols > cols)
                return fail(RO_ERR_INVALID, "%s: slot_windows[%d]: columns [%d, +%d) do not lie inside the image's %d", who, i,
                            w.first_col, w.cols, cols);
        }
    }
    if (!unit_dir || !unit_summary)
        return fail(RO_ERR_INVALID, "%s: null %s%s", who, d, !unit_dir ? "unit_dir" : "unit_summary");
    if (units_bytes > 0 && !units)
        return fail(RO_ERR_INVALID, "%s: null %sunits with units_bytes %lld", who, d, (long long)units_bytes);
    if (aligned && ((uintptr_t)units & 15u) != 0) return fail(RO_ERR_INVALID, "%s: %sunits is not aligned to 16 bytes", who, d);
    if (units_bytes > 0 && arena_floats > 0) {
        const uintptr_t u = (uintptr_t)units, a = (uintptr_t)arena;
        if (u < a + 4 * (uintptr_t)arena_floats && a < u + (uintptr_t)units_bytes)
            return fail(RO_ERR_INVALID, "%s: %sunits overlaps %sarena: the units are written while the arena is read", who, d, d);
    }
    return RO_OK;
}

int units_launch(ro_stft_t *h, ro::UnitsArgs &a, int kind, void *stream)
{
    HIP_TRY(hipSetDevice(h->device));
    int cus = 0, rc = device_cus(h, &cus);
    if (rc != RO_OK) return rc;
    // one block per kind: the images' call and the raw runs' call of a chunk may be in flight on two streams
    if ((rc = grow_scratch(h->d_units_scratch[kind], ro::units_scratch_bytes(a.dir_capacity))) != RO_OK) return rc;
    ro::units_scratch_layout(a, h->d_units_scratch[kind]);
    HIP_TRY(ro::launch_units(a, kind, cus, (hipStream_t)stream));
    return RO_OK;
}

// The twins' walk.  want(d): what source entry d asks for (ro_units.h); the unit of a written one is made here, float by
// float: the four bytes of arena float first + r stride + c, reversed
template <class Want>
void units_walk(int64_t n, Want want, const float *arena, int64_t stride, ro_fits_unit_t *unit_dir, void *units,
                int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    ro_unit_summary_t sum{};
    sum.entries = n;
    const int64_t room = units_bytes / RO_FITS_BLOCK;
    int64_t first_b = 0;                         // blocks of every writable entry so far, fitting or not
    for (int64_t d = 0; d < n; ++d) {
        const ro::UnitWant w = want(d);
        ro_fits_unit_t out{};
        out.status = w.status;
        if (w.status == RO_UNIT_SKIPPED) sum.skipped += 1;
        else if (w.status == RO_UNIT_INVALID) sum.invalid += 1;
        else {
            const int64_t blocks = ro::unit_blocks(w.naxis1, w.naxis2);
            out.bytes = 4 * (int64_t)w.naxis1 * w.naxis2;
            out.naxis2 = w.naxis2;
            out.naxis1 = w.naxis1;
            if (first_b + blocks <= room) {
                out.offset = first_b * RO_FITS_BLOCK;
                unsigned char *dst = static_cast<unsigned char *>(units) + out.offset;
                const unsigned char *src = reinterpret_cast<const unsigned char *>(arena);
                for (int64_t r = 0; r < w.naxis2; ++r)
                    for (int64_t c = 0; c < w.naxis1; ++c, dst += 4) {
                        const unsigned char *f = src + 4 * (w.first + r * stride + c);
                        dst[0] = f[3];
                        dst[1] = f[2];
                        dst[2] = f[1];
                        dst[3] = f[0];
                    }
                std::memset(dst, 0, (size_t)(blocks * RO_FITS_BLOCK - out.bytes));
                sum.written += 1;
                sum.units_bytes = (first_b + blocks) * RO_FITS_BLOCK;
            } else {
                out.status = RO_UNIT_NO_ROOM;
                sum.no_room += 1;
            }
            first_b += blocks;
        }
        unit_dir[d] = out;
    }
    sum.needed_bytes = first_b * RO_FITS_BLOCK;
    *unit_summary = sum;
}

int64_t entries_of(int64_t resolved, int64_t dir_capacity) { return std::min(std::max<int64_t>(resolved, 0), dir_capacity); }

void fill_args(ro::UnitsArgs &a, const void *dir, int64_t dir_capacity, const void *summary, const float *arena,
               int64_t arena_floats, int32_t cols, ro_fits_unit_t *unit_dir, void *units, int64_t units_bytes,
               ro_unit_summary_t *unit_summary)
{
    a.dir = dir;
    a.resolved = static_cast<const int64_t *>(summary);           // `resolved` is the first word of both summaries
    a.dir_capacity = dir_capacity;
    a.arena = arena;
    a.arena_floats = arena_floats;
    a.cols = cols;
    a.unit_dir = unit_dir;
    a.units = static_cast<char *>(units);
    a.units_bytes = units_bytes;
    a.summary = unit_summary;
}

}  // namespace

static_assert(offsetof(ro_snap_summary_t, resolved) == 0 && offsetof(ro_raw_summary_t, resolved) == 0, "fill_args reads it there");

extern "C" int ro_stft_snapshot_units_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                                               const ro_snap_summary_t *d_snap_summary, const float *d_arena,
                                               int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows,
                                               ro_fits_unit_t *d_unit_dir, void *d_units, int64_t units_bytes,
                                               ro_unit_summary_t *d_unit_summary, void *stream)
{
    const char *who = "ro_stft_snapshot_units_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    const int rc = units_check(who, "d_", false, true, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, slot_windows,
                               d_unit_dir, d_units, units_bytes, d_unit_summary);
    if (rc != RO_OK) return rc;
    ro::UnitsArgs a{};
    fill_args(a, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, d_unit_dir, d_units, units_bytes, d_unit_summary);
    for (int i = 0; i < ro::UNIT_SLOTS; ++i) {
        a.win_first[i] = slot_windows[i].first_col;
        a.win_cols[i] = slot_windows[i].cols;
    }
    return units_launch(h, a, ro::UNITS_OF_IMAGES, stream);
}

extern "C" int ro_stft_raw_units_resident(ro_stft_t *h, const ro_raw_capture_t *d_raw_dir, int64_t dir_capacity,
                                          const ro_raw_summary_t *d_raw_summary, const float *d_arena, int64_t arena_floats,
                                          ro_fits_unit_t *d_unit_dir, void *d_units, int64_t units_bytes,
                                          ro_unit_summary_t *d_unit_summary, void *stream)
{
    const char *who = "ro_stft_raw_units_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    const int rc = units_check(who, "d_", true, true, d_raw_dir, dir_capacity, d_raw_summary, d_arena, arena_floats, 2, nullptr,
                               d_unit_dir, d_units, units_bytes, d_unit_summary);
    if (rc != RO_OK) return rc;
    ro::UnitsArgs a{};
    fill_args(a, d_raw_dir, dir_capacity, d_raw_summary, d_arena, arena_floats, 2, d_unit_dir, d_units, units_bytes, d_unit_summary);
    return units_launch(h, a, ro::UNITS_OF_RAW, stream);
}

extern "C" int ro_snapshot_units_host(const ro_snapshot_t *dir, int64_t dir_capacity, const ro_snap_summary_t *snap_summary,
                                      const float *arena, int64_t arena_floats, int32_t cols,
                                      const ro_band_window_t *slot_windows, ro_fits_unit_t *unit_dir, void *units,
                                      int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    const int rc = units_check("ro_snapshot_units_host", "", false, false, dir, dir_capacity, snap_summary, arena, arena_floats, cols,
                               slot_windows, unit_dir, units, units_bytes, unit_summary);
    if (rc != RO_OK) return rc;
    units_walk(entries_of(snap_summary->resolved, dir_capacity), [&](int64_t d) {
        const ro_snapshot_t &e = dir[d];
        const bool slot_ok = e.slot >= 0 && e.slot < ro::UNIT_SLOTS;
        return ro::unit_want_image(e.status, e.slot, e.rows, e.offset, cols, arena_floats,
                                   slot_ok ? slot_windows[e.slot].first_col : 0, slot_ok ? slot_windows[e.slot].cols : 0);
    }, arena, cols, unit_dir, units, units_bytes, unit_summary);
    return RO_OK;
}

extern "C" int ro_raw_units_host(const ro_raw_capture_t *raw_dir, int64_t dir_capacity, const ro_raw_summary_t *raw_summary,
                                 const float *arena, int64_t arena_floats, ro_fits_unit_t *unit_dir, void *units,
                                 int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    const int rc = units_check("ro_raw_units_host", "", true, false, raw_dir, dir_capacity, raw_summary, arena, arena_floats, 2,
                               nullptr, unit_dir, units, units_bytes, unit_summary);
    if (rc != RO_OK) return rc;
    units_walk(entries_of(raw_summary->resolved, dir_capacity), [&](int64_t d) {
        const ro_raw_capture_t &e = raw_dir[d];
        return ro::unit_want_raw(e.status, e.samples, e.offset, arena_floats);
    }, arena, 2, unit_dir, units, units_bytes, unit_summary);
    return RO_OK;
}
