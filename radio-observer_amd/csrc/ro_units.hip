// ro_units.hip -- the events' files on the device: the FITS data unit of every captured snapshot (cut to the columns of the
// recorder that fired) and of every captured raw run, every float big-endian, zero-padded to 2880 bytes, packed into one
// buffer with a directory.  What the worker and FITSWriter make of an image (src/WaterfallBackend.cpp:176-177, :202-205;
// raw: :235, :258-261; src/FITSWriter.cpp).  include/ro_stft.h states the rules entry by entry.  Nothing is remembered from
// call to call and the arenas and their directories are only read.
//
// Plain launches, as in ro_snapshots.hip and ro_raw.hip; no workgroup waits for another one of its launch, no atomics, so
// the same input gives the same bytes:
//   units_plan_kernel<KIND>  the plan of ro_pack_plan.h over the source directory (KIND: how an entry is read --
//                     ro_snapshot_t with the slot's window, or ro_raw_capture_t): what is scanned are the writable entries'
//                     blocks.  It writes the unit directory (entry d is source entry d: nothing is compacted), the summary
//                     and the plan (ro_units.h)
//   units_copy_kernel  one kernel for both calls: the copy of ro_pack_plan.h over the 2880-byte blocks of the written
//                     units.  It gathers a block's 720 floats -- row and column from the wave-uniform naxis1 where the unit
//                     is a cut, straight on where it is contiguous -- reverses each float's bytes and stores it, lanes on
//                     consecutive floats, zeros behind the unit's data.  The loads are 4 bytes each: a window's first
//                     column may be odd; a 16-byte store per lane of four floats was measured slower
#include "ro_pack_plan.h"
#include "ro_units.h"

namespace ro {

namespace {

constexpr int T = RO_UNITS_TILE;
constexpr int BF = RO_UNITS_BLOCK_FLOATS;
static_assert(T == PLAN_TILE, "one entry per lane, four waves");
static_assert(BF == 720, "a block is 720 floats");
static_assert(sizeof(ro_fits_unit_t) == 32 && offsetof(ro_fits_unit_t, naxis1) == 24 && offsetof(ro_fits_unit_t, status) == 28 &&
                  sizeof(ro_unit_summary_t) == 64,
              "units_plan_kernel writes a unit as its four words");

template <int KIND> __device__ __forceinline__ UnitWant want_of(const UnitsArgs &a, int64_t d);

template <> __device__ __forceinline__ UnitWant want_of<UNITS_OF_IMAGES>(const UnitsArgs &a, int64_t d)
{
    const SnapWords e = load_snapshot(static_cast<const ro_snapshot_t *>(a.dir) + d);    // (only the words read are loaded)
    const int32_t slot = e.slot();
    int32_t first = 0, cols = 0;
#pragma unroll
    for (int s = 0; s < UNIT_SLOTS; ++s) {         // (constant indices: the table stays in the kernel arguments)
        first = slot == s ? a.win_first[s] : first;
        cols = slot == s ? a.win_cols[s] : cols;
    }
    return unit_want_image(e.status(), slot, e.rows(), e.offset(), a.cols, a.arena_floats, first, cols);
}

template <> __device__ __forceinline__ UnitWant want_of<UNITS_OF_RAW>(const UnitsArgs &a, int64_t d)
{
    const RawCaptureWords e = load_raw_capture(static_cast<const ro_raw_capture_t *>(a.dir) + d);
    return unit_want_raw(e.status(), e.samples(), e.offset(), a.arena_floats);
}

// The plan.  An entry FITS when the blocks up to and including its own are at most units_bytes / 2880.
template <int KIND> __global__ __launch_bounds__(T) void units_plan_kernel(UnitsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wblocks[1][PLAN_WAVES], wend[1][PLAN_WAVES];
    __shared__ int wcnt[PLAN_CLASSES][PLAN_WAVES];    // written, skipped, no room, invalid of each wave
    int64_t n = *a.resolved;
    n = n < 0 ? 0 : (n > a.dir_capacity ? a.dir_capacity : n);
    const int64_t room = a.units_bytes / RO_FITS_BLOCK;
    int64_t block_base = 0;                      // blocks of the writable entries in front of the tile
    int64_t used = 0;                            // ... of the written ones: where the last written unit ends
    int64_t written = 0, skipped = 0, no_room = 0, invalid = 0;
#pragma unroll 1
    for (int64_t t0 = 0; t0 < n; t0 += T) {
        const int64_t c = t0 + threadIdx.x;
        // (lanes past the last entry read it once more and take no part: no guarded load of a struct)
        const UnitWant w = want_of<KIND>(a, c < n ? c : n - 1);
        const bool live = c < n;
        const bool writable = live && w.status == RO_UNIT_WRITTEN;
        const int64_t blocks = writable ? unit_blocks(w.naxis1, w.naxis2) : 0;
        const int64_t take[1] = {blocks};
        const TileScan<1> scan = tile_scan(take, wblocks, lane, wave);
        const int64_t first_b = block_base + scan.before[0];
        const bool fits = writable && first_b + blocks <= room;
        const bool is[PLAN_CLASSES] = {fits, live && w.status == RO_UNIT_SKIPPED, writable && !fits,
                                       live && w.status == RO_UNIT_INVALID};
        const int64_t end[1] = {first_b + blocks};
        const TileCount<1> count = tile_count(is, end, wcnt, wend, lane, wave);
        written += count.total[0];
        skipped += count.total[1];
        no_room += count.total[2];
        invalid += count.total[3];
        used = count.end[0] > used ? count.end[0] : used;
        if (live) {
            const int status = writable ? (fits ? RO_UNIT_WRITTEN : RO_UNIT_NO_ROOM) : w.status;
            int64_t *out = reinterpret_cast<int64_t *>(a.unit_dir + c);         // ro_fits_unit_t, word by word
            out[0] = fits ? first_b * RO_FITS_BLOCK : 0;                                                  // offset
            out[1] = writable ? 4 * (int64_t)w.naxis1 * w.naxis2 : 0;                                     // bytes
            out[2] = writable ? w.naxis2 : 0;                                                             // naxis2
            out[3] = two_int32(writable ? w.naxis1 : 0, status);                                          // naxis1, status
            a.first_block[c] = first_b;
            a.first_float[c] = writable ? w.first : 0;
        }
        block_base += scan.total[0];
    }
    if (threadIdx.x == 0) {
        ro_unit_summary_t sum;
        sum.entries = n;
        sum.written = written;
        sum.skipped = skipped;
        sum.no_room = no_room;
        sum.invalid = invalid;
        sum.units_bytes = used * RO_FITS_BLOCK;
        sum.needed_bytes = block_base * RO_FITS_BLOCK;
        sum.reserved = 0;
        *a.summary = sum;
        UnitsPlanHead head;
        head.entries = n;
        head.blocks = used;
        *a.head = head;
    }
}

constexpr int STEPS = (BF + 63) / 64;            // floats per lane and block: 12, the last one for 16 lanes

// the block's floats of this lane into v, lanes on consecutive floats, all loads issued before the first value is looked
// at.  Float t of the block is unit float i0 + t; FLAT: arena float base + t; else the block's first float sits in column c0
// of a row that starts at arena float base, a row of the unit is naxis1 floats and a row of the arena `stride`.  Every lane
// loads every step, its index clamped into the arena, so no load is guarded and none leaves the buffer; floats at and
// behind `left` (what the unit still has from i0 on) become the zeros of the padding.
template <bool FLAT>
__device__ __forceinline__ void block_floats(const unsigned *arena, int64_t last, int64_t base, unsigned c0, unsigned naxis1,
                                             int64_t stride, int64_t left, int lane, unsigned (&v)[STEPS])
{
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const unsigned t = (unsigned)(lane + 64 * s);
        int64_t at;
        if (FLAT) {
            at = base + t;
            at = at < 0 ? 0 : (at > last ? last : at);
        } else at = cut_at(base, c0 + t, naxis1, stride, last);      // c0 < naxis1 < 2^31 and t < 768
        v[s] = arena[at];
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) v[s] = lane + 64 * s < left ? __builtin_bswap32(v[s]) : 0u;
}

// The copy: a work item is a block of the units.
__global__ __launch_bounds__(64 * COPY_WAVES) void units_copy_kernel(UnitsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.head->blocks;
    const int64_t entries = a.head->entries;
    if (total <= 0 || a.arena_floats < 1) return;
    const unsigned *arena = reinterpret_cast<const unsigned *>(a.arena);
    const int64_t last = a.arena_floats - 1;
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < total; b += wv.waves) {
        const int64_t d = plan_entry(a.first_block, entries, b);
        if (d < 0) continue;
        const ro_fits_unit_t *u = a.unit_dir + d;
        const int64_t k = b - a.first_block[d];                      // the block of the unit
        const int64_t floats = u->bytes >> 2, offset = u->offset;
        const int32_t naxis1 = u->naxis1;
        const int64_t i0 = k * BF;                                   // the block's first float of the unit
        if (u->status != RO_UNIT_WRITTEN || naxis1 < 1 || i0 >= floats || offset < 0 ||
            offset + (k + 1) * RO_FITS_BLOCK > a.units_bytes)
            continue;
        const int64_t first = a.first_float[d];
        const int64_t stride = a.cols;
        unsigned v[STEPS];
        if (naxis1 == stride) block_floats<true>(arena, last, first + i0, 0u, 1u, stride, floats - i0, lane, v);
        else {
            const int64_t r0 = i0 / naxis1;                          // wave-uniform: once per block
            block_floats<false>(arena, last, first + r0 * stride, (unsigned)(i0 - r0 * naxis1), (unsigned)naxis1, stride,
                                floats - i0, lane, v);
        }
        char *out = a.units + offset + k * RO_FITS_BLOCK;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int q = lane + 64 * s;
            if (q < BF) reinterpret_cast<unsigned *>(out)[q] = v[s];
        }
    }
}

}  // namespace

size_t units_scratch_bytes(int64_t dir_capacity)
{
    return sizeof(UnitsPlanHead) + 2 * (size_t)dir_capacity * sizeof(int64_t);
}

void units_scratch_layout(UnitsArgs &a, void *scratch)
{
    char *p = static_cast<char *>(scratch);
    a.head = reinterpret_cast<UnitsPlanHead *>(p);
    a.first_block = reinterpret_cast<int64_t *>(p + sizeof(UnitsPlanHead));
    a.first_float = a.first_block + a.dir_capacity;
}

namespace {

// what the plan reads of its arguments
bool plan_args_ok(const UnitsArgs &a, int kind)
{
    if ((kind != UNITS_OF_IMAGES && kind != UNITS_OF_RAW) || a.dir_capacity < 0 || a.dir_capacity > UNITS_MAX_ENTRIES ||
        (a.dir_capacity > 0 && !a.dir) || !a.resolved || a.arena_floats < 0 || (a.arena_floats > 0 && !a.arena) || a.cols < 1 ||
        !a.unit_dir || a.units_bytes < 0 || !a.summary || !a.head || !a.first_block || !a.first_float)
        return false;
    for (int i = 0; i < UNIT_SLOTS && kind == UNITS_OF_IMAGES; ++i)
        if (a.win_first[i] < 0 || a.win_cols[i] < 0 || (int64_t)a.win_first[i] + a.win_cols[i] > a.cols) return false;
    return true;
}

void plan_launch(const UnitsArgs &a, int kind, hipStream_t s)
{
    if (kind == UNITS_OF_IMAGES) hipLaunchKernelGGL(units_plan_kernel<UNITS_OF_IMAGES>, dim3(1), dim3(T), 0, s, a);
    else hipLaunchKernelGGL(units_plan_kernel<UNITS_OF_RAW>, dim3(1), dim3(T), 0, s, a);
}

}  // namespace

hipError_t launch_units_plan(const UnitsArgs &a, int kind, hipStream_t s)
{
    if (!plan_args_ok(a, kind)) return hipErrorInvalidValue;
    plan_launch(a, kind, s);
    return hipGetLastError();
}

hipError_t launch_units(const UnitsArgs &a, int kind, int cus, hipStream_t s)
{
    if (!plan_args_ok(a, kind) || (a.units_bytes > 0 && !a.units) || ((uintptr_t)a.units & 15u) != 0) return hipErrorInvalidValue;
    plan_launch(a, kind, s);
    hipLaunchKernelGGL(units_copy_kernel, dim3(copy_grid(cus)), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
