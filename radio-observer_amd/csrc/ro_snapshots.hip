// ro_snapshots.hip -- event snapshots on the device: the rows of each event, cut from a row ring in HBM.  What
// BolidRecorder's METEOR DETECTED branch ends in (startWriting(), src/BolidRecorder.cpp:262-263: clamp to snapshotRows_ and
// reserve rows [start, start + length) of the ring, src/WaterfallBackend.cpp:107-127; the worker writes them once the ring
// holds them all, :60-104, :202-205), for up to 8 detectors (SLOTS) at once.  include/ro_stft.h states the rules candidate
// by candidate.
//
// Plain launches; no workgroup waits for another one of its launch (the rule DESIGN.md 7 drew from the one-launch FP64
// form), no atomics, so the same input gives the same bytes:
//   ring_put_kernel   rows of an image into their ring slots: cut_windows_kernel's shape, the slot (first_row + i) %
//                     ring_rows computed once per wave and row
//   snap_plan_kernel  the plan of ro_pack_plan.h over the candidates of all slots in order: what is scanned are the packed
//                     rows (an image's arena offset is its packed row x cols); besides them the directory index and the
//                     slot's pending index go from tile to tile.  It writes the directory, the new pending lists, the
//                     summary and the plan (ro_snapshots.h)
//   snap_copy_kernel  the copy of ro_pack_plan.h over the packed rows: a row's cols floats from the ring slot to the arena
#include "ro_pack_plan.h"
#include "ro_snapshots.h"

namespace ro {

namespace {

constexpr int T = RO_SNAP_TILE;
static_assert(T == PLAN_TILE, "one candidate per lane, four waves");

constexpr int PUT_WAVES = 4;                    // waves of a workgroup, each on rows of its own
constexpr int PUT_STEPS = 4;                    // runs of 64 columns per wave: a workgroup spans 256 columns ...
constexpr int PUT_PASSES = 2;                   // ... of PUT_WAVES * PUT_PASSES rows
constexpr int PUT_COLS = 64 * PUT_STEPS;
constexpr int PUT_ROWS = PUT_WAVES * PUT_PASSES;

// Workgroup b takes the `chunk`-th run of PUT_COLS columns of every group_stride-th run of PUT_ROWS rows from group b /
// chunks on.  One dword per lane, lanes of a wave on consecutive columns; all loads of a lane are issued before its first
// store.  A wave's row is wave-uniform, so its slot -- the one 64-bit modulo -- is computed once per wave and row.
__global__ __launch_bounds__(64 * PUT_WAVES) void ring_put_kernel(RingPutArgs a, unsigned chunks, unsigned group_stride,
                                                                  int64_t groups)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned group0 = blockIdx.x / chunks;
    const unsigned chunk = blockIdx.x - group0 * chunks;
    const int64_t j0 = (int64_t)chunk * PUT_COLS + lane;
    for (int64_t group = group0; group < groups; group += group_stride) {
        float v[PUT_PASSES][PUT_STEPS];
        int64_t slot[PUT_PASSES];
        const int64_t row0 = group * PUT_ROWS + wave;
#pragma unroll
        for (int p = 0; p < PUT_PASSES; ++p) {
            const int64_t row = row0 + PUT_WAVES * p;
            const bool live = row < a.rows;
            slot[p] = live ? (a.first_row + row) % a.ring_rows : 0;
            const float *in = a.image + row * a.image_stride;
#pragma unroll
            for (int k = 0; k < PUT_STEPS; ++k) v[p][k] = (live && j0 + 64 * k < a.cols) ? in[j0 + 64 * k] : 0.0f;
        }
#pragma unroll
        for (int p = 0; p < PUT_PASSES; ++p) {
            const int64_t row = row0 + PUT_WAVES * p;
            float *out = a.ring + slot[p] * a.ring_stride;
#pragma unroll
            for (int k = 0; k < PUT_STEPS; ++k)
                if (row < a.rows && j0 + 64 * k < a.cols) out[j0 + 64 * k] = v[p][k];
        }
    }
}

enum { KIND_NONE = 0, KIND_PENDING, KIND_EMPTY, KIND_LOST, KIND_CAPTURABLE };
constexpr unsigned RESOLVED = 0b0111u, PENDING = 0b1000u;    // of tile_count's classes: captured, empty, lost; pending

// The plan.  A candidate FITS when the packed rows up to and including its own are at most arena_rows; what is resolved
// goes to the directory, what stays pending to the slot's new list, both in the order of the candidates.
__global__ __launch_bounds__(T) void snap_plan_kernel(SnapArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wrows[1][PLAN_WAVES], wend[1][PLAN_WAVES];
    __shared__ int wcnt[PLAN_CLASSES][PLAN_WAVES];    // captured, empty, lost, pending of each wave
    int64_t row_base = 0;                        // packed rows of the capturable candidates in front of the tile
    int64_t packed_rows = 0;                     // ... of the captured ones: where the last captured image ends
    int dir_base = 0;
    int64_t captured = 0, empty = 0, lost = 0, pending_all = 0, dropped = 0, unlisted = 0;
#pragma unroll 1
    for (int s = 0; s < a.slots; ++s) {
        if (!((a.slot_mask >> s) & 1u)) continue;
        int snap = a.snapshot_rows[0];           // (constant indices: the table stays in the kernel arguments)
#pragma unroll
        for (int w = 1; w < SNAP_MAX_SLOTS; ++w) snap = s == w ? a.snapshot_rows[w] : snap;
        int64_t have = a.pending_count[s];       // (every lane reads it; lane 0 writes the new one behind the barrier below)
        have = have < 0 ? 0 : (have > a.pending_capacity ? a.pending_capacity : have);
        int64_t fired = a.summary ? a.summary[s].events : 0;
        fired = fired < 0 ? 0 : fired;
        const int64_t listed = fired < a.capacity ? fired : a.capacity;
        unlisted += fired - listed;
        const int64_t n = have + listed;
        const ro_event_t *old_list = a.pending + s * a.pending_capacity;
        ro_event_t *new_list = a.pending_new + s * a.pending_capacity;
        int64_t pend_base = 0;                   // still-pending candidates of the slot in front of the tile
#pragma unroll 1
        for (int64_t t0 = 0; t0 < n; t0 += T) {
            const int64_t c = t0 + threadIdx.x;
            // (lanes past the last candidate read it once more and take no part: no guarded load of a struct)
            const int64_t cc = c < n ? c : n - 1;
            const EventWords e = load_event(cc < have ? old_list + cc : a.events + (s * a.capacity + (cc - have)));
            const int64_t len = e.length() < snap ? e.length() : snap;
            const int64_t hi = e.start_row() + len;
            const int64_t lo = e.start_row() > 0 ? e.start_row() : 0;
            const int kind = c >= n ? KIND_NONE
                           : hi > a.head_row ? KIND_PENDING
                           : hi <= lo ? KIND_EMPTY
                           : lo < a.head_row - a.ring_rows ? KIND_LOST : KIND_CAPTURABLE;
            const int rows = kind == KIND_CAPTURABLE ? (int)(hi - lo) : 0;   // 1 ... snap
            const int64_t take[1] = {rows};
            const TileScan<1> scan = tile_scan(take, wrows, lane, wave);
            const int64_t first = row_base + scan.before[0];                 // packed row where this candidate's image starts
            const bool fits = kind == KIND_CAPTURABLE && first + rows <= a.arena_rows;
            const bool pend = kind == KIND_PENDING || (kind == KIND_CAPTURABLE && !fits);
            const bool is[PLAN_CLASSES] = {fits, kind == KIND_EMPTY, kind == KIND_LOST, pend};
            const int64_t end[1] = {first + rows};
            const TileCount<1> count = tile_count(is, end, wcnt, wend, lane, wave);
            captured += count.total[0];
            empty += count.total[1];
            lost += count.total[2];
            packed_rows = count.end[0] > packed_rows ? count.end[0] : packed_rows;
            if (fits || kind == KIND_EMPTY || kind == KIND_LOST) {
                const int d = dir_base + count.rank(RESOLVED, lane);
                const int status = fits ? RO_SNAP_CAPTURED : (kind == KIND_EMPTY ? RO_SNAP_EMPTY : RO_SNAP_LOST);
                store_snapshot(a.dir + d, make_snapshot(e, lo, fits ? first * a.cols : 0, fits ? rows : 0, s, status));
                a.first_packed[d] = first;
            }
            const int64_t pend_at = pend_base + count.rank(PENDING, lane);
            if (pend && pend_at < a.pending_capacity) store_event(new_list + pend_at, e);
            row_base += scan.total[0];
            dir_base += count.total[0] + count.total[1] + count.total[2];
            pend_base += count.total[3];
        }
        // the slot's new list is complete in scratch, and nobody reads the old one any more: it goes back
        __threadfence_block();
        wg_sync();
        const int64_t kept = pend_base < a.pending_capacity ? pend_base : a.pending_capacity;
        for (int64_t j = threadIdx.x; j < kept; j += T) store_event(a.pending + (s * a.pending_capacity + j), load_event(new_list + j));
        if (threadIdx.x == 0) a.pending_count[s] = kept;
        pending_all += kept;
        dropped += pend_base - kept;
    }
    if (threadIdx.x == 0) {
        ro_snap_summary_t sum;
        sum.resolved = dir_base;
        sum.captured = captured;
        sum.empty = empty;
        sum.lost = lost;
        sum.pending = pending_all;
        sum.pending_dropped = dropped;
        sum.unlisted = unlisted;
        sum.arena_floats = packed_rows * a.cols;
        *a.snap_summary = sum;
        SnapPlanHead head;
        head.resolved = dir_base;
        head.packed_rows = packed_rows;
        *a.head = head;
    }
}

constexpr int COPY_STEPS = 4;                   // loads of 64 columns each in flight before the stores

// The copy: a work item is a packed row.
__global__ __launch_bounds__(64 * COPY_WAVES) void snap_copy_kernel(SnapArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.head->packed_rows;
    const int64_t resolved = a.head->resolved;
    if (total <= 0) return;
    const CopyWave wv = copy_wave();
    for (int64_t p = wv.me; p < total; p += wv.waves) {
        const int64_t d = plan_entry(a.first_packed, resolved, p);
        if (d < 0) continue;
        const ro_snapshot_t *en = a.dir + d;
        const int64_t k = p - a.first_packed[d];
        const int64_t offset = en->offset + k * a.cols;
        if (en->status != RO_SNAP_CAPTURED || k >= en->rows || offset + a.cols > a.arena_floats) continue;
        const float *in = a.ring + ((en->first_row + k) % a.ring_rows) * a.ring_stride;
        float *out = a.arena + offset;
        for (int64_t c0 = lane; c0 < a.cols; c0 += 64 * COPY_STEPS) {
            float v[COPY_STEPS];
#pragma unroll
            for (int q = 0; q < COPY_STEPS; ++q) v[q] = c0 + 64 * q < a.cols ? in[c0 + 64 * q] : 0.0f;
#pragma unroll
            for (int q = 0; q < COPY_STEPS; ++q)
                if (c0 + 64 * q < a.cols) out[c0 + 64 * q] = v[q];
        }
    }
}

}  // namespace

size_t snap_scratch_bytes(int slots, int64_t capacity, int64_t pending_capacity)
{
    const size_t entries = (size_t)slots * (size_t)(capacity + pending_capacity);
    return sizeof(SnapPlanHead) + entries * sizeof(int64_t) + (size_t)slots * (size_t)pending_capacity * sizeof(ro_event_t);
}

void snap_scratch_layout(SnapArgs &a, void *scratch)
{
    char *p = static_cast<char *>(scratch);
    a.head = reinterpret_cast<SnapPlanHead *>(p);
    p += sizeof(SnapPlanHead);
    a.first_packed = reinterpret_cast<int64_t *>(p);
    p += (size_t)a.slots * (size_t)(a.capacity + a.pending_capacity) * sizeof(int64_t);
    a.pending_new = reinterpret_cast<ro_event_t *>(p);
}

hipError_t launch_ring_put(const RingPutArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    if (!a.image || !a.ring || a.cols < 1 || a.ring_rows < 1 || a.rows > a.ring_rows || a.first_row < 0 ||
        a.image_stride < a.cols || a.ring_stride < a.cols)
        return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)(((int64_t)a.cols + PUT_COLS - 1) / PUT_COLS);
    const int64_t groups = (a.rows + PUT_ROWS - 1) / PUT_ROWS;
    // any number of rows in one launch: the grid is one-dimensional and stays below 2^30 workgroups, which stride over the
    // row groups beyond that
    const int64_t at_once = std::max<int64_t>(1, ((int64_t)1 << 30) / chunks);
    const unsigned stride = (unsigned)std::min<int64_t>(groups, at_once);
    hipLaunchKernelGGL(ring_put_kernel, dim3(stride * chunks), dim3(64 * PUT_WAVES), 0, s, a, chunks, stride, groups);
    return hipGetLastError();
}

hipError_t launch_snapshots(const SnapArgs &a, int cus, hipStream_t s)
{
    if (a.slots < 1 || a.slots > SNAP_MAX_SLOTS || a.slot_mask == 0u || (a.slot_mask >> a.slots) != 0u || a.capacity < 0 ||
        a.pending_capacity < 0 || (a.capacity > 0 && (!a.events || !a.summary)) || !a.ring || a.ring_rows < 1 || a.cols < 1 ||
        a.ring_stride < a.cols || a.head_row < 0 || (a.pending_capacity > 0 && !a.pending) || !a.pending_count || !a.dir ||
        a.arena_floats < 0 || (a.arena_floats > 0 && !a.arena) || a.arena_rows != a.arena_floats / a.cols || !a.snap_summary ||
        !a.head || !a.first_packed || !a.pending_new ||
        (int64_t)a.slots * (a.capacity + a.pending_capacity) > SNAP_MAX_SLOTS * SNAP_MAX_CANDIDATES)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(snap_plan_kernel, dim3(1), dim3(T), 0, s, a);
    hipLaunchKernelGGL(snap_copy_kernel, dim3(copy_grid(cus)), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
