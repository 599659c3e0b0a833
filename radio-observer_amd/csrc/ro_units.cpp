// ro_units.cpp -- the events' files as FITS data units (include/ro_stft.h; kernels: ro_units.hip): argument checks, the
// handle's scratch, the launches; and ro_snapshot_units_host / ro_raw_units_host, the same rules entry by entry over host
// memory.  Nothing in the resident calls reads device memory: how many entries there are, which of them get a unit and
// where it goes are decided on the device.
#include "ro_host.h"

using namespace ro::host;

static_assert(sizeof(ro_fits_unit_t) == 32 && sizeof(ro_unit_summary_t) == 64 && RO_FITS_BLOCK == 2880,
              "the units' structs are ABI");

namespace ro {
namespace host {

int units_check(const char *who, const char *d, const UnitNames &names, bool raw, bool aligned, const void *dir,
                int64_t dir_capacity, const void *summary, const float *arena, int64_t arena_floats, int32_t cols,
                const ro_band_window_t *slot_windows, const ro_fits_unit_t *unit_dir, const void *units, int64_t units_bytes,
                const ro_unit_summary_t *unit_summary)
{
    const char *dir_name = raw ? "raw_dir" : "dir", *sum_name = raw ? "raw_summary" : "snap_summary";
    if (dir_capacity < 0 || arena_floats < 0 || units_bytes < 0)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld, arena_floats %lld, %s %lld: none may be negative", who,
                    (long long)dir_capacity, (long long)arena_floats, names.bytes, (long long)units_bytes);
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
        return fail(RO_ERR_INVALID, "%s: null %s%s", who, d, !unit_dir ? names.dir : names.summary);
    if (units_bytes > 0 && !units)
        return fail(RO_ERR_INVALID, "%s: null %s%s with %s %lld", who, d, names.buf, names.bytes, (long long)units_bytes);
    if (aligned && ((uintptr_t)units & 15u) != 0)
        return fail(RO_ERR_INVALID, "%s: %s%s is not aligned to 16 bytes", who, d, names.buf);
    if (units_bytes > 0 && arena_floats > 0) {
        const uintptr_t u = (uintptr_t)units, a = (uintptr_t)arena;
        if (u < a + 4 * (uintptr_t)arena_floats && a < u + (uintptr_t)units_bytes)
            return fail(RO_ERR_INVALID, "%s: %s%s overlaps %sarena: the %s are written while the arena is read", who, d, names.buf,
                        d, names.buf);
    }
    return RO_OK;
}

void units_fill_args(ro::UnitsArgs &a, const void *dir, int64_t dir_capacity, const void *summary, const float *arena,
                     int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows, ro_fits_unit_t *unit_dir,
                     void *units, int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    a.dir = dir;
    a.resolved = static_cast<const int64_t *>(summary);           // `resolved` is the first word of both summaries
    a.dir_capacity = dir_capacity;
    a.arena = arena;
    a.arena_floats = arena_floats;
    a.cols = cols;
    for (int i = 0; i < ro::UNIT_SLOTS && slot_windows; ++i) {
        a.win_first[i] = slot_windows[i].first_col;
        a.win_cols[i] = slot_windows[i].cols;
    }
    a.unit_dir = unit_dir;
    a.units = static_cast<char *>(units);
    a.units_bytes = units_bytes;
    a.summary = unit_summary;
}

}  // namespace host
}  // namespace ro

namespace {

const UnitNames UNITS = {"unit_dir", "units", "units_bytes", "unit_summary"};

int units_launch(ro_stft_t *h, ro::UnitsArgs &a, int kind, void *stream)
{
    // one block per kind: the images' call and the raw runs' call of a chunk may be in flight on two streams
    int cus = 0;
    const int rc = scratch_for(h, h->d_units_scratch[kind], ro::units_scratch_bytes(a.dir_capacity), &cus);
    if (rc != RO_OK) return rc;
    ro::units_scratch_layout(a, h->d_units_scratch[kind]);
    HIP_TRY(ro::launch_units(a, kind, cus, (hipStream_t)stream));
    return RO_OK;
}

// the unit of a written entry, float by float: the four bytes of arena float first + r stride + c, reversed
void swapped_floats(const float *arena, int64_t stride, const ro::UnitWant &w, unsigned char *dst)
{
    const unsigned char *src = reinterpret_cast<const unsigned char *>(arena);
    for (int64_t r = 0; r < w.naxis2; ++r)
        for (int64_t c = 0; c < w.naxis1; ++c, dst += 4) {
            const unsigned char *f = src + 4 * (w.first + r * stride + c);
            dst[0] = f[3];
            dst[1] = f[2];
            dst[2] = f[1];
            dst[3] = f[0];
        }
}

// the twins: pack_walk over the call's entry rule, in units of 2880-byte blocks
template <class Want>
void units_walk(int64_t n, Want want, const float *arena, int64_t stride, ro_fits_unit_t *unit_dir, void *units,
                int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    pack_walk(n, [&](int64_t d) { return walk_want(want(d), 4, RO_FITS_BLOCK); },
              [&](int64_t d, unsigned char *dst) { swapped_floats(arena, stride, want(d), dst); }, unit_dir, units, units_bytes,
              unit_summary);
}

}  // namespace

static_assert(offsetof(ro_snap_summary_t, resolved) == 0 && offsetof(ro_raw_summary_t, resolved) == 0, "units_fill_args reads it there");

extern "C" int ro_stft_snapshot_units_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                                               const ro_snap_summary_t *d_snap_summary, const float *d_arena,
                                               int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows,
                                               ro_fits_unit_t *d_unit_dir, void *d_units, int64_t units_bytes,
                                               ro_unit_summary_t *d_unit_summary, void *stream)
{
    const char *who = "ro_stft_snapshot_units_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    const int rc = units_check(who, "d_", UNITS, false, true, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, slot_windows,
                               d_unit_dir, d_units, units_bytes, d_unit_summary);
    if (rc != RO_OK) return rc;
    ro::UnitsArgs a{};
    units_fill_args(a, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, slot_windows, d_unit_dir, d_units, units_bytes,
                    d_unit_summary);
    return units_launch(h, a, ro::UNITS_OF_IMAGES, stream);
}

extern "C" int ro_stft_raw_units_resident(ro_stft_t *h, const ro_raw_capture_t *d_raw_dir, int64_t dir_capacity,
                                          const ro_raw_summary_t *d_raw_summary, const float *d_arena, int64_t arena_floats,
                                          ro_fits_unit_t *d_unit_dir, void *d_units, int64_t units_bytes,
                                          ro_unit_summary_t *d_unit_summary, void *stream)
{
    const char *who = "ro_stft_raw_units_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    const int rc = units_check(who, "d_", UNITS, true, true, d_raw_dir, dir_capacity, d_raw_summary, d_arena, arena_floats, 2, nullptr,
                               d_unit_dir, d_units, units_bytes, d_unit_summary);
    if (rc != RO_OK) return rc;
    ro::UnitsArgs a{};
    units_fill_args(a, d_raw_dir, dir_capacity, d_raw_summary, d_arena, arena_floats, 2, nullptr, d_unit_dir, d_units, units_bytes,
                    d_unit_summary);
    return units_launch(h, a, ro::UNITS_OF_RAW, stream);
}

extern "C" int ro_snapshot_units_host(const ro_snapshot_t *dir, int64_t dir_capacity, const ro_snap_summary_t *snap_summary,
                                      const float *arena, int64_t arena_floats, int32_t cols,
                                      const ro_band_window_t *slot_windows, ro_fits_unit_t *unit_dir, void *units,
                                      int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    const int rc = units_check("ro_snapshot_units_host", "", UNITS, false, false, dir, dir_capacity, snap_summary, arena, arena_floats, cols,
                               slot_windows, unit_dir, units, units_bytes, unit_summary);
    if (rc != RO_OK) return rc;
    units_walk(entries_of(snap_summary->resolved, dir_capacity),
               [&](int64_t d) { return unit_want_snapshot(dir[d], cols, arena_floats, slot_windows); }, arena, cols, unit_dir,
               units, units_bytes, unit_summary);
    return RO_OK;
}

extern "C" int ro_raw_units_host(const ro_raw_capture_t *raw_dir, int64_t dir_capacity, const ro_raw_summary_t *raw_summary,
                                 const float *arena, int64_t arena_floats, ro_fits_unit_t *unit_dir, void *units,
                                 int64_t units_bytes, ro_unit_summary_t *unit_summary)
{
    const int rc = units_check("ro_raw_units_host", "", UNITS, true, false, raw_dir, dir_capacity, raw_summary, arena, arena_floats, 2,
                               nullptr, unit_dir, units, units_bytes, unit_summary);
    if (rc != RO_OK) return rc;
    units_walk(entries_of(raw_summary->resolved, dir_capacity), [&](int64_t d) {
        const ro_raw_capture_t &e = raw_dir[d];
        return ro::unit_want_raw(e.status, e.samples, e.offset, arena_floats);
    }, arena, 2, unit_dir, units, units_bytes, unit_summary);
    return RO_OK;
}
