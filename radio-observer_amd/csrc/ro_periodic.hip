// ro_periodic.hip -- the periodic snapshots' files on the device: the FITS data unit of every due snapshot of up to
// RO_MAX_PERIODIC always-on recorders, cut from the row ring's slots to the recorder's columns, every float big-endian,
// zero-padded to 2880 bytes.  What SnapshotRecorder::write and FITSWriter make of the ring's rows
// (src/WaterfallBackend.cpp:176-177, :202-205; src/FITSWriter.cpp), for the snapshots update() queues (:415-427).
// include/ro_stft.h states the cadence and the rules.  The plan is host arithmetic (ro_periodic.cpp): what is due, what fits
// and where it goes are known before the launch, so nothing but scalars arrives here and there is no plan kernel.
//
// ONE plain launch; no workgroup waits for another, no atomics, no LDS, so the same input gives the same bytes:
//   periodic_copy_kernel  the copy of ro_pack_plan.h over the 2880-byte blocks of the written units, as units_copy_kernel
//                     (ro_units.hip) does it: a wave takes a block, finds its recorder's run among the eight in the kernel
//                     arguments, the unit and the unit's first row from the run's scalars, and gathers the block's 720
//                     floats from the ring's slots -- the block's first slot is one int64 modulo per block, wave-uniform;
//                     a lane's row is that slot plus its row within the block, wrapped once -- reverses each float's bytes
//                     and stores it, lanes on consecutive floats, zeros behind the unit's data.  The loads are 4 bytes
//                     each (a window's first column may be odd), clamped into the ring and never guarded.
#include "ro_pack_plan.h"
#include "ro_periodic.h"

namespace ro {

namespace {

constexpr int BF = RO_PERIODIC_BLOCK_FLOATS;
static_assert(BF == 720, "a block is 720 floats");
constexpr int STEPS = (BF + 63) / 64;            // floats per lane and block: 12, the last one for 16 lanes

// the run of work item b: the last one that starts at or in front of it.  Runs without units are passed over.  Which run
// it is takes two words of each; the run itself is then one scalar load from the kernel arguments (b is wave-uniform)
__device__ __forceinline__ PeriodicRun run_of(const PeriodicArgs &a, int64_t b)
{
    int at = 0;
#pragma unroll
    for (int i = 1; i < RO_MAX_PERIODIC; ++i) at = a.run[i].units > 0 && a.run[i].block0 <= b ? i : at;
    return a.run[at];
}

// The copy: a work item is a block of the units; item b is block b of d_units.
__global__ __launch_bounds__(64 * COPY_WAVES) void periodic_copy_kernel(PeriodicArgs a)
{
    const int lane = threadIdx.x & 63;
    const unsigned *ring = reinterpret_cast<const unsigned *>(a.ring);
    const int64_t last = (a.ring_rows - 1) * a.ring_stride + a.cols - 1;      // the last float of the last slot's row
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < a.blocks; b += wv.waves) {
        const PeriodicRun r = run_of(a, b);
        if (r.units < 1 || r.naxis1 < 1 || r.unit_blocks < 1 || b < r.block0) continue;
        const int64_t in_run = b - r.block0;
        const int64_t j = in_run / r.unit_blocks;                               // the unit of the run (wave-uniform)
        if (j >= r.units) continue;                                             // (a run's blocks end where the next one starts)
        const int64_t k = in_run - j * r.unit_blocks;                           // the block of the unit
        const int64_t rows = j == r.units - 1 ? r.last_rows : r.snapshot_rows;
        const unsigned naxis1 = (unsigned)r.naxis1;
        const int64_t floats = rows * naxis1;
        const int64_t i0 = k * BF;                                              // the block's first float of the unit
        if (i0 >= floats) continue;
        const int64_t r0 = i0 / naxis1;                                         // its row of the unit, its column of the window
        const unsigned c0 = (unsigned)(i0 - r0 * naxis1);
        const int64_t slot0 = (r.row0 + j * r.snapshot_rows + r0) % a.ring_rows;   // one modulo per block
        const int64_t left = floats - i0;
        unsigned v[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const unsigned x = c0 + (unsigned)(lane + 64 * s);                  // c0 < naxis1 < 2^31 and lane + 64 s < 768
            const unsigned dr = x / naxis1;
            // a unit has at most ring_rows rows, so slot0 + dr wraps at most once where the float is the unit's; the others
            // are clamped and become the zeros of the padding
            int64_t slot = slot0 + dr;
            slot = slot >= a.ring_rows ? slot - a.ring_rows : slot;
            int64_t at = slot * a.ring_stride + r.first_col + (x - dr * naxis1);
            at = at < 0 ? 0 : (at > last ? last : at);
            v[s] = ring[at];
        }
#pragma unroll
        for (int s = 0; s < STEPS; ++s) v[s] = lane + 64 * s < left ? __builtin_bswap32(v[s]) : 0u;
        unsigned *out = reinterpret_cast<unsigned *>(a.units + b * RO_FITS_BLOCK);
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int q = lane + 64 * s;
            if (q < BF) out[q] = v[s];
        }
    }
}

}  // namespace

hipError_t launch_periodic(const PeriodicArgs &a, int cus, hipStream_t s)
{
    if (!periodic_runs_ok(a) || (a.blocks > 0 && !a.units)) return hipErrorInvalidValue;
    if (a.blocks == 0) return hipSuccess;
    // the work is known here: no more workgroups than there are blocks for their waves
    const int64_t need = (a.blocks + COPY_WAVES - 1) / COPY_WAVES;
    const unsigned grid = (unsigned)std::min<int64_t>(copy_grid(cus), need);
    hipLaunchKernelGGL(periodic_copy_kernel, dim3(grid), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
