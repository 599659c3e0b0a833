// ro_levels.cpp -- the grey-level previews (include/ro_stft.h; kernels: ro_levels.hip): the viewer's ln image of every
// captured event snapshot of an arena and of every written snapshot of a periodic plan, one byte per pixel: argument
// checks (the units' own, ro_units.cpp and ro_periodic.cpp, under the levels' argument names), the handle's scratch, the
// launches; and ro_snapshot_levels_host / ro_periodic_levels_host, the same rules entry by entry over host memory with the
// C library's logf and ro_ln_levels.  Nothing in the resident calls reads device memory.
#include "ro_host.h"

using namespace ro::host;

static_assert(sizeof(ro_level_range_t) == 8 && RO_LEVEL_BLOCK == 720, "the levels' struct and block are ABI");

namespace {

const UnitNames SNAPSHOT_NAMES = {"level_dir", "levels", "levels_bytes", "level_summary"};
const PeriodicNames PERIODIC_NAMES = {"levels", "levels_bytes", " (the levels take a quarter of their units' bytes: offset / 4 + 720 per block)"};

// one image on the host: `count` pixels, pixel i at src[at(i)], to the range and to `count` levels at dst
template <class At> void image_levels(const float *src, int64_t count, At at, ro_level_range_t *range, unsigned char *dst)
{
    std::vector<float> ln((size_t)count);
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t i = 0; i < count; ++i) {
        const float v = src[at(i)];
        const float l = logf(v);
        ln[(size_t)i] = l;
        if (v != 0.f) {
            mn = l < mn ? l : mn;
            mx = l > mx ? l : mx;
        }
    }
    range->ln_min = mn;
    range->ln_max = mx;
    ro_ln_levels(ln.data(), count, mn, mx, dst);
}

// the directory entries of each run's first unit and the units in front of each run; the WRITTEN entries of a recorder
// follow one another (periodic_check).  Returns the WRITTEN entries
int64_t runs_entries(const ro_periodic_entry_t *dir, int64_t entries, ro::PeriodicLevelsArgs *a)
{
    bool seen[RO_MAX_PERIODIC] = {};
    for (int64_t d = 0; d < entries; ++d)
        if (dir[d].status == RO_PERIODIC_WRITTEN && !seen[dir[d].recorder]) {
            seen[dir[d].recorder] = true;
            a->entry0[dir[d].recorder] = d;
        }
    a->units = 0;
    for (int i = 0; i < RO_MAX_PERIODIC; ++i) {
        a->unit0[i] = a->units;
        a->units += a->p.run[i].units;
    }
    return a->units;
}

}  // namespace

extern "C" int ro_stft_snapshot_levels_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                                                const ro_snap_summary_t *d_snap_summary, const float *d_arena,
                                                int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows,
                                                ro_fits_unit_t *d_level_dir, ro_level_range_t *d_ranges, void *d_levels,
                                                int64_t levels_bytes, ro_unit_summary_t *d_level_summary, void *stream)
{
    const char *who = "ro_stft_snapshot_levels_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    int rc = units_check(who, "d_", SNAPSHOT_NAMES, false, true, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols,
                         slot_windows, d_level_dir, d_levels, levels_bytes, d_level_summary);
    if (rc != RO_OK) return rc;
    if (dir_capacity > 0 && !d_ranges)
        return fail(RO_ERR_INVALID, "%s: null d_ranges with dir_capacity %lld", who, (long long)dir_capacity);
    if (levels_bytes > INT64_MAX / 4)
        return fail(RO_ERR_INVALID, "%s: levels_bytes %lld: at most 2^61", who, (long long)levels_bytes);
    ro::SnapshotLevelsArgs a{};
    // the units' plan with the room of the units these levels belong to; its directory and summary go to scratch
    units_fill_args(a.plan, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, slot_windows, nullptr, nullptr,
                    levels_bytes / RO_LEVEL_BLOCK * RO_FITS_BLOCK, nullptr);
    a.level_dir = d_level_dir;
    a.ranges = d_ranges;
    a.levels = static_cast<char *>(d_levels);
    a.levels_bytes = levels_bytes;
    a.level_summary = d_level_summary;
    int cus = 0;
    if ((rc = scratch_for(h, h->d_levels_scratch[0], ro::snapshot_levels_scratch_bytes(dir_capacity, levels_bytes), &cus)) != RO_OK) return rc;
    ro::snapshot_levels_scratch_layout(a, h->d_levels_scratch[0]);
    HIP_TRY(ro::launch_snapshot_levels(a, cus, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_snapshot_levels_host(const ro_snapshot_t *dir, int64_t dir_capacity, const ro_snap_summary_t *snap_summary,
                                       const float *arena, int64_t arena_floats, int32_t cols,
                                       const ro_band_window_t *slot_windows, ro_fits_unit_t *level_dir, ro_level_range_t *ranges,
                                       void *levels, int64_t levels_bytes, ro_unit_summary_t *level_summary)
{
    const char *who = "ro_snapshot_levels_host";
    const int rc = units_check(who, "", SNAPSHOT_NAMES, false, false, dir, dir_capacity, snap_summary, arena, arena_floats, cols,
                               slot_windows, level_dir, levels, levels_bytes, level_summary);
    if (rc != RO_OK) return rc;
    if (dir_capacity > 0 && !ranges) return fail(RO_ERR_INVALID, "%s: null ranges with dir_capacity %lld", who, (long long)dir_capacity);
    const int64_t n = entries_of(snap_summary->resolved, dir_capacity);
    for (int64_t d = 0; d < n; ++d) ranges[d] = ro_level_range_t{0.f, 0.f};
    auto want = [&](int64_t d) { return unit_want_snapshot(dir[d], cols, arena_floats, slot_windows); };
    pack_walk(n, [&](int64_t d) { return walk_want(want(d), 1, RO_LEVEL_BLOCK); }, [&](int64_t d, unsigned char *dst) {
        const ro::UnitWant w = want(d);
        image_levels(arena, (int64_t)w.naxis1 * w.naxis2, [&](int64_t i) { return w.first + i / w.naxis1 * cols + i % w.naxis1; },
                     &ranges[d], dst);
    }, level_dir, levels, levels_bytes, level_summary);
    return RO_OK;
}

extern "C" int ro_stft_periodic_levels_resident(ro_stft_t *h, const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                                                const ro_periodic_entry_t *dir, int64_t entries, ro_level_range_t *d_ranges,
                                                void *d_levels, int64_t levels_bytes, void *stream)
{
    const char *who = "ro_stft_periodic_levels_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    ro::PeriodicLevelsArgs a{};
    int rc = periodic_check(who, "d_", PERIODIC_NAMES, RO_LEVEL_BLOCK, true, ring, recorders, count, dir, entries, d_levels,
                            levels_bytes, &a.p);
    if (rc != RO_OK) return rc;
    if (runs_entries(dir, entries, &a) == 0) return RO_OK;
    if (!d_ranges) return fail(RO_ERR_INVALID, "%s: null d_ranges with a WRITTEN entry", who);
    a.ranges = d_ranges;
    a.levels = static_cast<char *>(d_levels);
    int cus = 0;
    if ((rc = scratch_for(h, h->d_levels_scratch[1], (size_t)a.p.blocks * sizeof(ro::LevelKeys), &cus)) != RO_OK) return rc;
    a.keys = reinterpret_cast<ro::LevelKeys *>(static_cast<char *>(h->d_levels_scratch[1]));
    HIP_TRY(ro::launch_periodic_levels(a, cus, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_periodic_levels_host(const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                                       const ro_periodic_entry_t *dir, int64_t entries, ro_level_range_t *ranges, void *levels,
                                       int64_t levels_bytes)
{
    const char *who = "ro_periodic_levels_host";
    ro::PeriodicLevelsArgs a{};
    const int rc = periodic_check(who, "", PERIODIC_NAMES, RO_LEVEL_BLOCK, false, ring, recorders, count, dir, entries, levels,
                                  levels_bytes, &a.p);
    if (rc != RO_OK) return rc;
    if (runs_entries(dir, entries, &a) == 0) return RO_OK;
    if (!ranges) return fail(RO_ERR_INVALID, "%s: null ranges with a WRITTEN entry", who);
    for (int64_t d = 0; d < entries; ++d) {
        const ro_periodic_entry_t &e = dir[d];
        if (e.status != RO_PERIODIC_WRITTEN) continue;
        const int64_t first_col = recorders[e.recorder].window.first_col;
        const int64_t pixels = (int64_t)e.naxis1 * e.rows;
        unsigned char *dst = static_cast<unsigned char *>(levels) + e.offset / 4;
        image_levels(ring->d_rows, pixels, [&](int64_t i) {
            return (e.first_row + i / e.naxis1) % ring->ring_rows * ring->stride + first_col + i % e.naxis1;
        }, &ranges[d], dst);
        std::memset(dst + pixels, 0, (size_t)(ro::periodic_blocks(e.naxis1, e.rows) * RO_LEVEL_BLOCK - pixels));
    }
    return RO_OK;
}
