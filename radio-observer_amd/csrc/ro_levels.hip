// ro_levels.hip -- the grey-level previews on the device: what the stations' fits2png makes of every snapshot file -- the
// natural log of the non-zero pixels, the image's own min / max of it, (ln - min) / (max - min) * 255 cut to one byte per
// pixel (fits2png:46, :444-445, :476-502) -- for every captured snapshot of an arena (the entry rules and the plan of
// ro_units.hip) and for every written snapshot of a periodic plan (the runs of ro_periodic.hip), each image zero-padded
// to RO_LEVEL_BLOCK = 720 bytes.  An image has as many 720-byte blocks as its FITS unit has 2880-byte ones, so block b of
// the levels is block b of the units and the plans are the units' plans.  The pixel rule is ln_reduce_kernel's and
// ln_quant_kernel's (ro_kernels.hip), logf called as they call it.  include/ro_stft.h states the rules.
//
// Plain launches; no workgroup waits for another one of its launch, no atomics, no LDS, so the same input gives the same
// bytes.  An image's range is a segmented min / max over images whose sizes only the plan knows: instead of atomics on a
// pair per image, every block leaves its own pair and a fold reads them in a fixed order.
//   (units_plan_kernel<UNITS_OF_IMAGES>, launched from ro_units.hip: the event snapshots' plan, in unit terms, to scratch)
//   *_reduce_kernel   the copy of ro_pack_plan.h over the 720-pixel blocks of the written images: a wave takes a block, finds
//                     its entry (plan_entry) or its run, gathers the block's pixels as units_copy_kernel /
//                     periodic_copy_kernel gather them -- 4-byte loads, clamped into the source and never guarded -- and
//                     writes the order keys of the block's min / max of logf over its non-zero pixels to scratch
//   *_fold_kernel     a wave takes an image and folds its blocks' keys into d_ranges; the snapshots' one also translates
//                     the plan's unit directory and summary into level terms (offsets and bytes divided by four)
//   *_store_kernel    the blocks again: logf once more, quantised against the image's range, four levels per dword, lanes
//                     on consecutive dwords, zeros behind the image's pixels up to the block's end
// Every source float is read twice and a byte is written per pixel.
#include "ro_pack_plan.h"
#include "ro_levels.h"

namespace ro {

namespace {

constexpr int BP = RO_LEVEL_BLOCK;               // pixels of one block: what one wave takes at a time; a block belongs to one image
static_assert(BP == 720 && BP % 16 == 0, "a block is 720 pixels, 180 dwords; blocks keep the alignment of d_levels");
constexpr int STEPS = (BP + 63) / 64;            // the reduce: pixels per lane and block, lanes on consecutive pixels: 12
constexpr int QUADS = BP / 4;                    // the store: dwords of a block
constexpr int QSTEPS = (QUADS + 63) / 64;        // ... per lane: 3, lanes on consecutive dwords
static_assert(sizeof(ro_level_range_t) == 8 && sizeof(LevelKeys) == 8, "a pair of words each");

// Where pixel t of a block lies in the source, clamped into it.  Pixel t of the block is image pixel i0 + t; the block's
// first pixel sits in column c0 < naxis1 < 2^31 of an image row, and t < 768.
// An arena image: units_copy_kernel's gather (cut_at, ro_pack_plan.h) from the row that starts at arena float `base`
struct ArenaAt {
    int64_t base, stride, last;
    unsigned c0, naxis1;
    __device__ __forceinline__ int64_t operator()(unsigned t) const { return cut_at(base, c0 + t, naxis1, stride, last); }
};
// A ring image: periodic_copy_kernel's gather (periodic_ring_at, ro_periodic.h) from the row that lives in slot0
struct RingAt {
    int64_t ring_rows, ring_stride, slot0, last;
    int32_t first_col;
    unsigned c0, naxis1;
    __device__ __forceinline__ int64_t operator()(unsigned t) const
    {
        return periodic_ring_at(ring_rows, ring_stride, slot0, c0 + t, naxis1, first_col, last);
    }
};

// one block of one image: `left` pixels of the image from the block's first on (at least 1), gathered through `at`
template <class At> struct LevelBlock {
    int64_t image;                               // whose range it shares: the entry (snapshots), the unit of all runs (periodic)
    int64_t left;
    At at;
};

// the keys of a block: every lane loads every step (all loads issued before the first value is looked at), pixels at and
// behind `left` and behind the block take no part
template <class At> __device__ __forceinline__ LevelKeys block_keys(const float *src, const LevelBlock<At> &blk, int lane)
{
    float v[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) v[s] = src[blk.at((unsigned)(lane + 64 * s))];
    unsigned kmin = 0xffffffffu, kmax = 0u;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int t = lane + 64 * s;
        const float l = logf(v[s]);
        if (v[s] != 0.f && t < BP && t < blk.left) {
            const unsigned k = order_key(l);
            kmin = min(kmin, k);
            kmax = max(kmax, k);
        }
    }
    return LevelKeys{wave_min_u32(kmin), wave_max_u32(kmax)};
}

// the range of keys folded: +inf / -inf for an image without a non-zero pixel
__device__ __forceinline__ ro_level_range_t range_of(unsigned kmin, unsigned kmax)
{
    ro_level_range_t r;
    r.ln_min = kmin == 0xffffffffu ? __builtin_inff() : key_to_float(kmin);
    r.ln_max = kmax == 0u ? -__builtin_inff() : key_to_float(kmax);
    return r;
}

// an image's range from its blocks' keys [first, first + blocks): lanes stride over them, every lane returns the range
__device__ __forceinline__ ro_level_range_t fold_keys(const LevelKeys *keys, int64_t first, int64_t blocks, int lane)
{
    unsigned kmin = 0xffffffffu, kmax = 0u;
    for (int64_t i = lane; i < blocks; i += 64) {
        const LevelKeys k = keys[first + i];
        kmin = min(kmin, k.kmin);
        kmax = max(kmax, k.kmax);
    }
    return range_of(wave_min_u32(kmin), wave_max_u32(kmax));
}

// the levels of a block to `out` (the block's 720 bytes, 16-byte aligned): ln_quant_kernel's arithmetic, float32 throughout
template <class At>
__device__ __forceinline__ void block_store(const float *src, const LevelBlock<At> &blk, ro_level_range_t range, char *out, int lane)
{
    float v[QSTEPS][4];
#pragma unroll
    for (int s = 0; s < QSTEPS; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[s][j] = src[blk.at((unsigned)(4 * (lane + 64 * s) + j))];
    const float mn = range.ln_min, span = range.ln_max - range.ln_min;
#pragma unroll
    for (int s = 0; s < QSTEPS; ++s) {
        const int q = lane + 64 * s;
        unsigned word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = v[s][j];
            const float l = logf(x);
            const float level = (l - mn) / span * 255.f;
            const uint8_t u = (x != 0.f && span > 0.f) ? (uint8_t)(int)level : (uint8_t)0;
            word |= (4 * q + j < blk.left ? (unsigned)u : 0u) << (8 * j);
        }
        if (q < QUADS) reinterpret_cast<unsigned *>(out)[q] = word;
    }
}

// ---- the event snapshots ----------------------------------------------------------------------------------------------------
// block b of the written images, as units_copy_kernel reads the plan; false: nothing to do for it
__device__ __forceinline__ bool snapshot_block(const SnapshotLevelsArgs &a, int64_t entries, int64_t b, LevelBlock<ArenaAt> &blk,
                                               int64_t &out_byte)
{
    const UnitsArgs &p = a.plan;
    const int64_t d = plan_entry(p.first_block, entries, b);
    if (d < 0) return false;
    const ro_fits_unit_t *u = p.unit_dir + d;    // in unit terms
    const int64_t k = b - p.first_block[d];      // the block of the image
    const int64_t pixels = u->bytes >> 2, offset = u->offset;
    const int32_t naxis1 = u->naxis1;
    const int64_t i0 = k * BP;
    out_byte = (offset >> 2) + k * BP;
    if (u->status != RO_UNIT_WRITTEN || naxis1 < 1 || i0 >= pixels || offset < 0 || out_byte + BP > a.levels_bytes ||
        b >= a.levels_bytes / BP)
        return false;
    const int64_t stride = p.cols;
    const int64_t r0 = i0 / naxis1;              // wave-uniform: once per block
    blk.image = d;
    blk.left = pixels - i0;
    blk.at = ArenaAt{p.first_float[d] + r0 * stride, stride, p.arena_floats - 1, (unsigned)(i0 - r0 * naxis1), (unsigned)naxis1};
    return true;
}

__global__ __launch_bounds__(64 * COPY_WAVES) void snapshot_levels_reduce_kernel(SnapshotLevelsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.plan.head->blocks, entries = a.plan.head->entries;
    if (total <= 0 || a.plan.arena_floats < 1) return;
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < total; b += wv.waves) {
        LevelBlock<ArenaAt> blk;
        int64_t out_byte;
        if (!snapshot_block(a, entries, b, blk, out_byte)) continue;
        const LevelKeys k = block_keys(a.plan.arena, blk, lane);
        if (lane == 63) a.keys[b] = k;
    }
}

// a wave per entry: its level directory entry and its range; the first wave also writes the summary
__global__ __launch_bounds__(64 * COPY_WAVES) void snapshot_levels_fold_kernel(SnapshotLevelsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t entries = a.plan.head->entries, total = a.plan.head->blocks;
    const CopyWave wv = copy_wave();
    if (wv.me == 0 && lane == 0) {
        ro_unit_summary_t sum = *a.plan.summary;
        sum.units_bytes >>= 2;
        sum.needed_bytes >>= 2;
        *a.level_summary = sum;
    }
    for (int64_t d = wv.me; d < entries; d += wv.waves) {
        ro_fits_unit_t u = a.plan.unit_dir[d];
        ro_level_range_t range = {0.f, 0.f};
        if (u.status == RO_UNIT_WRITTEN) {
            const int64_t first = a.plan.first_block[d];
            int64_t blocks = unit_blocks(u.naxis1, u.naxis2);
            blocks = first < 0 || first > total ? 0 : (blocks > total - first ? total - first : blocks);
            range = fold_keys(a.keys, first, blocks, lane);
        }
        if (lane == 0) {
            u.offset >>= 2;
            u.bytes >>= 2;
            a.level_dir[d] = u;
            a.ranges[d] = range;
        }
    }
}

__global__ __launch_bounds__(64 * COPY_WAVES) void snapshot_levels_store_kernel(SnapshotLevelsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.plan.head->blocks, entries = a.plan.head->entries;
    if (total <= 0 || a.plan.arena_floats < 1) return;
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < total; b += wv.waves) {
        LevelBlock<ArenaAt> blk;
        int64_t out_byte;
        if (!snapshot_block(a, entries, b, blk, out_byte)) continue;
        block_store(a.plan.arena, blk, a.ranges[blk.image], a.levels + out_byte, lane);
    }
}

// ---- the periodic snapshots -------------------------------------------------------------------------------------------------
// the run of unit u of all runs: the last one that starts at or in front of it (as periodic_run_index finds a block's)
__device__ __forceinline__ int run_of_unit(const PeriodicLevelsArgs &a, int64_t u)
{
    int at = 0;
#pragma unroll
    for (int i = 1; i < RO_MAX_PERIODIC; ++i) at = a.p.run[i].units > 0 && a.unit0[i] <= u ? i : at;
    return at;
}

// block b of the written images, as periodic_copy_kernel reads the runs
__device__ __forceinline__ bool periodic_block(const PeriodicLevelsArgs &a, int64_t b, LevelBlock<RingAt> &blk)
{
    const PeriodicArgs &p = a.p;
    const int i = periodic_run_index(p, b);
    const PeriodicRun r = p.run[i];
    if (r.units < 1 || r.naxis1 < 1 || r.unit_blocks < 1 || b < r.block0) return false;
    const int64_t in_run = b - r.block0;
    const int64_t j = in_run / r.unit_blocks;                                   // the unit of the run (wave-uniform)
    if (j >= r.units) return false;
    const int64_t k = in_run - j * r.unit_blocks;                               // the block of the image
    const int64_t rows = j == r.units - 1 ? r.last_rows : r.snapshot_rows;
    const unsigned naxis1 = (unsigned)r.naxis1;
    const int64_t pixels = rows * naxis1;
    const int64_t i0 = k * BP;
    if (i0 >= pixels) return false;
    const int64_t r0 = i0 / naxis1;
    blk.image = a.unit0[i] + j;
    blk.left = pixels - i0;
    blk.at = RingAt{p.ring_rows, p.ring_stride, (r.row0 + j * r.snapshot_rows + r0) % p.ring_rows,                              // one modulo per block
                    (p.ring_rows - 1) * p.ring_stride + p.cols - 1, r.first_col, (unsigned)(i0 - r0 * naxis1), naxis1};
    return true;
}

__global__ __launch_bounds__(64 * COPY_WAVES) void periodic_levels_reduce_kernel(PeriodicLevelsArgs a)
{
    const int lane = threadIdx.x & 63;
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < a.p.blocks; b += wv.waves) {
        LevelBlock<RingAt> blk;
        if (!periodic_block(a, b, blk)) continue;
        const LevelKeys k = block_keys(a.p.ring, blk, lane);
        if (lane == 63) a.keys[b] = k;
    }
}

// the directory entry and the first block of unit u of all runs, and how many blocks it has; false: no such unit
__device__ __forceinline__ bool periodic_unit(const PeriodicLevelsArgs &a, int64_t u, int64_t &entry, int64_t &first, int64_t &blocks)
{
    const int i = run_of_unit(a, u);
    const PeriodicRun r = a.p.run[i];
    const int64_t j = u - a.unit0[i];
    if (r.units < 1 || j < 0 || j >= r.units) return false;
    entry = a.entry0[i] + j;
    first = r.block0 + j * r.unit_blocks;
    blocks = j == r.units - 1 ? periodic_blocks(r.naxis1, r.last_rows) : r.unit_blocks;
    return first >= 0 && blocks >= 0 && blocks <= a.p.blocks - first;
}

__global__ __launch_bounds__(64 * COPY_WAVES) void periodic_levels_fold_kernel(PeriodicLevelsArgs a)
{
    const int lane = threadIdx.x & 63;
    const CopyWave wv = copy_wave();
    for (int64_t u = wv.me; u < a.units; u += wv.waves) {
        int64_t entry, first, blocks;
        if (!periodic_unit(a, u, entry, first, blocks)) continue;
        const ro_level_range_t range = fold_keys(a.keys, first, blocks, lane);
        if (lane == 0) a.ranges[entry] = range;
    }
}

__global__ __launch_bounds__(64 * COPY_WAVES) void periodic_levels_store_kernel(PeriodicLevelsArgs a)
{
    const int lane = threadIdx.x & 63;
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < a.p.blocks; b += wv.waves) {
        LevelBlock<RingAt> blk;
        if (!periodic_block(a, b, blk)) continue;
        int64_t entry, first, blocks;
        if (!periodic_unit(a, blk.image, entry, first, blocks)) continue;
        block_store(a.p.ring, blk, a.ranges[entry], a.levels + b * BP, lane);
    }
}

// no more workgroups than there are items for their waves
unsigned grid_for(int cus, int64_t items)
{
    const int64_t need = (items + COPY_WAVES - 1) / COPY_WAVES;
    return (unsigned)std::max<int64_t>(std::min<int64_t>(copy_grid(cus), need), 1);
}

}  // namespace

size_t snapshot_levels_scratch_bytes(int64_t dir_capacity, int64_t levels_bytes)
{
    return units_scratch_bytes(dir_capacity) + (size_t)dir_capacity * sizeof(ro_fits_unit_t) + sizeof(ro_unit_summary_t) +
           (size_t)(levels_bytes / BP) * sizeof(LevelKeys);
}

void snapshot_levels_scratch_layout(SnapshotLevelsArgs &a, void *scratch)
{
    units_scratch_layout(a.plan, scratch);
    char *p = static_cast<char *>(scratch) + units_scratch_bytes(a.plan.dir_capacity);
    a.plan.unit_dir = reinterpret_cast<ro_fits_unit_t *>(p);
    p += (size_t)a.plan.dir_capacity * sizeof(ro_fits_unit_t);
    a.plan.summary = reinterpret_cast<ro_unit_summary_t *>(p);
    a.keys = reinterpret_cast<LevelKeys *>(p + sizeof(ro_unit_summary_t));
}

hipError_t launch_snapshot_levels(const SnapshotLevelsArgs &a, int cus, hipStream_t s)
{
    // the plan's room in unit terms is exactly the blocks levels_bytes holds
    if (a.levels_bytes < 0 || a.plan.units_bytes != a.levels_bytes / BP * RO_FITS_BLOCK || (a.levels_bytes > 0 && !a.levels) ||
        ((uintptr_t)a.levels & 15u) != 0 || !a.level_dir || (a.plan.dir_capacity > 0 && !a.ranges) || !a.level_summary || !a.keys)
        return hipErrorInvalidValue;
    const hipError_t e = launch_units_plan(a.plan, UNITS_OF_IMAGES, s);
    if (e != hipSuccess) return e;
    // the work is known on the device only, but it is at most the blocks of the room
    const unsigned blocks_grid = grid_for(cus, a.levels_bytes / BP);
    hipLaunchKernelGGL(snapshot_levels_reduce_kernel, dim3(blocks_grid), dim3(64 * COPY_WAVES), 0, s, a);
    hipLaunchKernelGGL(snapshot_levels_fold_kernel, dim3(grid_for(cus, a.plan.dir_capacity)), dim3(64 * COPY_WAVES), 0, s, a);
    hipLaunchKernelGGL(snapshot_levels_store_kernel, dim3(blocks_grid), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_periodic_levels(const PeriodicLevelsArgs &a, int cus, hipStream_t s)
{
    const PeriodicArgs &p = a.p;
    if (!periodic_runs_ok(p)) return hipErrorInvalidValue;
    int64_t units = 0;                           // unit0[] counts the units of the runs in front
    for (int i = 0; i < RO_MAX_PERIODIC; ++i) {
        if (p.run[i].units == 0) continue;
        if (a.unit0[i] != units || a.entry0[i] < 0) return hipErrorInvalidValue;
        units += p.run[i].units;
    }
    if (units != a.units) return hipErrorInvalidValue;
    if (p.blocks == 0) return hipSuccess;
    if (!a.ranges || !a.levels || ((uintptr_t)a.levels & 15u) != 0 || !a.keys) return hipErrorInvalidValue;
    const unsigned blocks_grid = grid_for(cus, p.blocks);
    hipLaunchKernelGGL(periodic_levels_reduce_kernel, dim3(blocks_grid), dim3(64 * COPY_WAVES), 0, s, a);
    hipLaunchKernelGGL(periodic_levels_fold_kernel, dim3(grid_for(cus, a.units)), dim3(64 * COPY_WAVES), 0, s, a);
    hipLaunchKernelGGL(periodic_levels_store_kernel, dim3(blocks_grid), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
