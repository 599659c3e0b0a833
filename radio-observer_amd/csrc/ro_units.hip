// ro_units.hip -- the events' files on the device: the FITS data unit of every captured snapshot (cut to the columns of the
// recorder that fired) and of every captured raw run, every float big-endian, zero-padded to 2880 bytes, packed into one
// buffer with a directory.  What the worker and FITSWriter make of an image (src/WaterfallBackend.cpp:176-177, :202-205;
// raw: :235, :258-261; src/FITSWriter.cpp).  include/ro_stft.h states the rules entry by entry.  Nothing is remembered from
// call to call and the arenas and their directories are only read.
//
// Plain launches, as in ro_snapshots.hip and ro_raw.hip; no workgroup waits for another one of its launch, no atomics, so
// the same input gives the same bytes:
//   units_plan_kernel<KIND>  ONE workgroup walks the source directory RO_UNITS_TILE entries at a time (KIND: how an entry
//                     is read -- ro_snapshot_t with the slot's window, or ro_raw_capture_t) and carries the exclusive
//                     prefix of the writable entries' blocks from tile to tile in 64 bits.  It writes the unit directory
//                     (entry d is source entry d: nothing is compacted), the summary and the plan (ro_units.h)
//   units_copy_kernel  one kernel for both calls; a grid sized by the host from the CU count; every wave strides over the
//                     2880-byte blocks of the written units, finds a block's unit by binary search in the plan (the block
//                     index is wave-uniform: no divergent loop), gathers the block's 720 floats -- row and column from the
//                     wave-uniform naxis1 where the unit is a cut, straight on where it is contiguous -- reverses each
//                     float's bytes and stores it, lanes on consecutive floats, zeros behind the unit's data.  The loads
//                     are 4 bytes each: a window's first column may be odd.  Units start at multiples of 2880 = 180 x 16
//                     in a buffer aligned to 16, so a lane could take four floats and make one 16-byte store; that form
//                     was built and measured SLOWER, 120 us against 81 us for 197 MB of raw runs -- its
//                     four 4-byte loads per lane sit 16 bytes apart, so every load instruction touches four times the
//                     cache lines -- and is gone
#include <algorithm>
#include <cstddef>

#include "ro_device_util.h"
#include "ro_units.h"

namespace ro {

namespace {

constexpr int T = RO_UNITS_TILE;
constexpr int WAVES = T / 64;
constexpr int BF = RO_UNITS_BLOCK_FLOATS;
static_assert(T == 256 && WAVES == 4, "one entry per lane, four waves");
static_assert(BF == 720, "a block is 720 floats");

// A source entry travels as the three 64-bit words behind its event (every ABI struct here is 8-byte aligned and has no
// padding).
static_assert(sizeof(ro_snapshot_t) == 72 && offsetof(ro_snapshot_t, offset) == 48 && offsetof(ro_snapshot_t, rows) == 56 &&
                  offsetof(ro_snapshot_t, slot) == 60 && offsetof(ro_snapshot_t, status) == 64 &&
                  sizeof(ro_raw_capture_t) == 72 && offsetof(ro_raw_capture_t, samples) == 48 &&
                  offsetof(ro_raw_capture_t, offset) == 56 && offsetof(ro_raw_capture_t, status) == 68 &&
                  sizeof(ro_fits_unit_t) == 32 && offsetof(ro_fits_unit_t, naxis1) == 24 && offsetof(ro_fits_unit_t, status) == 28 &&
                  sizeof(ro_unit_summary_t) == 64,
              "the words below are these fields");

template <int KIND> __device__ __forceinline__ UnitWant want_of(const UnitsArgs &a, int64_t d);

template <> __device__ __forceinline__ UnitWant want_of<UNITS_OF_IMAGES>(const UnitsArgs &a, int64_t d)
{
    const int64_t *q = reinterpret_cast<const int64_t *>(static_cast<const ro_snapshot_t *>(a.dir) + d);
    const int64_t offset = q[6];
    const uint64_t rows_slot = (uint64_t)q[7];
    const int32_t status = (int32_t)(uint32_t)q[8];
    const int32_t rows = (int32_t)(uint32_t)rows_slot, slot = (int32_t)(uint32_t)(rows_slot >> 32);
    int32_t first = 0, cols = 0;
#pragma unroll
    for (int s = 0; s < UNIT_SLOTS; ++s) {         // (constant indices: the table stays in the kernel arguments)
        first = slot == s ? a.win_first[s] : first;
        cols = slot == s ? a.win_cols[s] : cols;
    }
    return unit_want_image(status, slot, rows, offset, a.cols, a.arena_floats, first, cols);
}

template <> __device__ __forceinline__ UnitWant want_of<UNITS_OF_RAW>(const UnitsArgs &a, int64_t d)
{
    const int64_t *q = reinterpret_cast<const int64_t *>(static_cast<const ro_raw_capture_t *>(a.dir) + d);
    return unit_want_raw((int32_t)(uint32_t)((uint64_t)q[8] >> 32), q[6], q[7], a.arena_floats);
}

// inclusive prefix sum of a 64-bit count over the 64 lanes: four runs of wave_inclusive_sum, on 16 bits each (64 x 65535
// fits a run with room to spare), put together modulo 2^64 -- a raw run of 2^31 pairs has more blocks than one run holds
__device__ __forceinline__ int64_t wave_inclusive_sum64(int64_t x)
{
    const uint64_t u = (uint64_t)x;
    uint64_t sum = 0;
#pragma unroll
    for (int limb = 0; limb < 4; ++limb)
        sum += (uint64_t)wave_inclusive_sum((unsigned)(u >> (16 * limb)) & 0xffffu) << (16 * limb);
    return (int64_t)sum;
}

// One workgroup.  Per tile: every lane classifies its entry; the blocks of the writable ones are scanned (the waves' totals
// meet in LDS) -- an entry FITS when the blocks up to and including its own are at most units_bytes / 2880, and since the
// scan runs over every writable entry, fitting or not, nothing behind the first that does not fit can fit either.
template <int KIND> __global__ __launch_bounds__(T) void units_plan_kernel(UnitsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wblocks[WAVES], wend[WAVES];
    __shared__ int wcnt[4][WAVES];               // written, skipped, no room, invalid of each wave
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
        const int64_t inc = wave_inclusive_sum64(blocks);
        if (lane == 63) wblocks[wave] = inc;
        wg_sync();
        int64_t first_b = block_base + inc - blocks, tile_b = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) {
            if (v < wave) first_b += wblocks[v];
            tile_b += wblocks[v];
        }
        const bool fits = writable && first_b + blocks <= room;
        const unsigned long long mw = __ballot(fits), ms = __ballot(live && w.status == RO_UNIT_SKIPPED),
                                 mn = __ballot(writable && !fits), mi = __ballot(live && w.status == RO_UNIT_INVALID);
        if (lane == 0) {
            wcnt[0][wave] = __popcll(mw);
            wcnt[1][wave] = __popcll(ms);
            wcnt[2][wave] = __popcll(mn);
            wcnt[3][wave] = __popcll(mi);
        }
        // the written entries are a prefix of the writable ones: the wave's last one ends its blocks
        if (mw == 0ull ? lane == 0 : lane == 63 - __clzll((long long)mw)) wend[wave] = mw == 0ull ? 0 : first_b + blocks;
        wg_sync();
#pragma unroll
        for (int v = 0; v < WAVES; ++v) {
            written += wcnt[0][v];
            skipped += wcnt[1][v];
            no_room += wcnt[2][v];
            invalid += wcnt[3][v];
            used = wend[v] > used ? wend[v] : used;
        }
        if (live) {
            const int status = writable ? (fits ? RO_UNIT_WRITTEN : RO_UNIT_NO_ROOM) : w.status;
            int64_t *out = reinterpret_cast<int64_t *>(a.unit_dir + c);         // ro_fits_unit_t, word by word
            out[0] = fits ? first_b * RO_FITS_BLOCK : 0;                                                  // offset
            out[1] = writable ? 4 * (int64_t)w.naxis1 * w.naxis2 : 0;                                     // bytes
            out[2] = writable ? w.naxis2 : 0;                                                             // naxis2
            out[3] = (int64_t)(((uint64_t)(unsigned)status << 32) | (unsigned)(writable ? w.naxis1 : 0)); // naxis1, status
            a.first_block[c] = first_b;
            a.first_float[c] = writable ? w.first : 0;
        }
        block_base += tile_b;
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

constexpr int COPY_WAVES = 4;
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
        if (FLAT) at = base + t;
        else {
            const unsigned x = c0 + t;           // c0 < naxis1 < 2^31 and t < 768
            const unsigned dr = x / naxis1;
            at = base + (int64_t)dr * stride + (x - dr * naxis1);
        }
        at = at < 0 ? 0 : (at > last ? last : at);
        v[s] = arena[at];
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) v[s] = lane + 64 * s < left ? __builtin_bswap32(v[s]) : 0u;
}

// Every wave takes blocks wave, wave + waves, ...; nothing to do when the plan's total is zero.  The entry of block b is
// the last one whose first block is at most b: the table never descends, an entry without a unit in front of a written one
// holds the same value and comes first, and every entry behind the last written one holds at least the total.
__global__ __launch_bounds__(64 * COPY_WAVES) void units_copy_kernel(UnitsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.head->blocks;
    const int64_t entries = a.head->entries;
    if (total <= 0 || a.arena_floats < 1) return;
    const unsigned *arena = reinterpret_cast<const unsigned *>(a.arena);
    const int64_t last = a.arena_floats - 1;
    const unsigned waves = gridDim.x * COPY_WAVES;
    const unsigned me = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * COPY_WAVES + (threadIdx.x >> 6)));
    for (int64_t b = me; b < total; b += waves) {
        int64_t lo = 0, hi = entries;            // the first entry whose first block lies beyond b
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.first_block[mid] <= b) lo = mid + 1;
            else hi = mid;
        }
        if (lo == 0) continue;
        const ro_fits_unit_t *u = a.unit_dir + (lo - 1);
        const int64_t k = b - a.first_block[lo - 1];                 // the block of the unit
        const int64_t floats = u->bytes >> 2, offset = u->offset;
        const int32_t naxis1 = u->naxis1;
        const int64_t i0 = k * BF;                                   // the block's first float of the unit
        if (u->status != RO_UNIT_WRITTEN || naxis1 < 1 || i0 >= floats || offset < 0 ||
            offset + (k + 1) * RO_FITS_BLOCK > a.units_bytes)
            continue;
        const int64_t first = a.first_float[lo - 1];
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

hipError_t launch_units(const UnitsArgs &a, int kind, int cus, hipStream_t s)
{
    if ((kind != UNITS_OF_IMAGES && kind != UNITS_OF_RAW) || a.dir_capacity < 0 || a.dir_capacity > UNITS_MAX_ENTRIES ||
        (a.dir_capacity > 0 && !a.dir) || !a.resolved || a.arena_floats < 0 || (a.arena_floats > 0 && !a.arena) || a.cols < 1 ||
        !a.unit_dir || a.units_bytes < 0 || (a.units_bytes > 0 && !a.units) || ((uintptr_t)a.units & 15u) != 0 || !a.summary ||
        !a.head || !a.first_block || !a.first_float)
        return hipErrorInvalidValue;
    for (int i = 0; i < UNIT_SLOTS && kind == UNITS_OF_IMAGES; ++i)
        if (a.win_first[i] < 0 || a.win_cols[i] < 0 || (int64_t)a.win_first[i] + a.win_cols[i] > a.cols) return hipErrorInvalidValue;
    if (kind == UNITS_OF_IMAGES) hipLaunchKernelGGL(units_plan_kernel<UNITS_OF_IMAGES>, dim3(1), dim3(T), 0, s, a);
    else hipLaunchKernelGGL(units_plan_kernel<UNITS_OF_RAW>, dim3(1), dim3(T), 0, s, a);
    // the work is known on the device only: four workgroups per CU, every wave strides over the blocks
    hipLaunchKernelGGL(units_copy_kernel, dim3((unsigned)(4 * std::max(cus, 1))), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
