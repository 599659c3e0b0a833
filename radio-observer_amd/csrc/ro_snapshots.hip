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
//   snap_plan_kernel  ONE workgroup walks the candidates of all slots in order, RO_SNAP_TILE at a time, and carries three
//                     exclusive prefixes from tile to tile: the directory index, the packed rows (int64; an image's arena
//                     offset is its packed row x cols) and the slot's pending index.  It writes the directory, the new
//                     pending lists, the summary and the plan (ro_snapshots.h) -- the candidates are few, nobody waits for
//                     this kernel, and one workgroup needs no ordering between workgroups
//   snap_copy_kernel  a grid sized by the host from the CU count; every wave strides over the packed rows, finds a row's
//                     directory entry by binary search in the plan (the row index is wave-uniform: scalar loads, no
//                     divergent loop) and copies its cols floats from the ring slot to the arena
#include <algorithm>
#include <cstddef>

#include "ro_device_util.h"
#include "ro_snapshots.h"

namespace ro {

namespace {

constexpr int T = RO_SNAP_TILE;
constexpr int WAVES = T / 64;
static_assert(T == 256 && WAVES == 4, "one candidate per lane, four waves");

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

// An event travels as its five 64-bit words (every ABI struct here is 8-byte aligned and has no padding): copied field by
// field, its float / int tail went through a private array.
constexpr int EVENT_WORDS = sizeof(ro_event_t) / 8;
static_assert(sizeof(ro_event_t) == 40 && sizeof(ro_snapshot_t) == 72 && offsetof(ro_event_t, start_row) == 8 &&
                  offsetof(ro_event_t, length) == 16 && offsetof(ro_snapshot_t, first_row) == 40 &&
                  offsetof(ro_snapshot_t, offset) == 48 && offsetof(ro_snapshot_t, rows) == 56 &&
                  offsetof(ro_snapshot_t, slot) == 60 && offsetof(ro_snapshot_t, status) == 64,
              "the words below are these fields");
struct EventWords {
    int64_t w[EVENT_WORDS];
    __device__ __forceinline__ int64_t start_row() const { return w[1]; }
    __device__ __forceinline__ int64_t length() const { return w[2]; }
};
__device__ __forceinline__ EventWords load_event(const ro_event_t *p)
{
    EventWords e;
    const int64_t *q = reinterpret_cast<const int64_t *>(p);
#pragma unroll
    for (int w = 0; w < EVENT_WORDS; ++w) e.w[w] = q[w];
    return e;
}
__device__ __forceinline__ void store_event(ro_event_t *p, const EventWords &e)
{
    int64_t *q = reinterpret_cast<int64_t *>(p);
#pragma unroll
    for (int w = 0; w < EVENT_WORDS; ++w) q[w] = e.w[w];
}

__device__ __forceinline__ int popc_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// One workgroup.  Per tile: every lane classifies its candidate; the rows of the capturable ones are scanned (two runs of
// wave_inclusive_sum, on the low 16 bits and on the rest of a count below 2^31, put together as int64; the waves' totals
// meet in LDS) -- a candidate FITS when the packed rows up to and including its own are at most arena_rows, and since the
// scan runs over every capturable candidate, fitting or not, nothing behind the first that does not fit can fit either.
// What is resolved and what stays pending is known after that; both are ranked with ballots.
__global__ __launch_bounds__(T) void snap_plan_kernel(SnapArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wrows[WAVES], wend[WAVES];
    __shared__ int wcnt[4][WAVES];               // captured, empty, lost, pending of each wave
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
            const unsigned inc_lo = wave_inclusive_sum((unsigned)rows & 0xffffu);
            const unsigned inc_hi = wave_inclusive_sum((unsigned)rows >> 16);
            const int64_t inc = ((int64_t)inc_hi << 16) + (int64_t)inc_lo;
            if (lane == 63) wrows[wave] = inc;
            wg_sync();
            int64_t first = row_base + inc - rows, tile_rows = 0;          // packed row where this candidate's image starts
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                if (w < wave) first += wrows[w];
                tile_rows += wrows[w];
            }
            const bool fits = kind == KIND_CAPTURABLE && first + rows <= a.arena_rows;
            const bool pend = kind == KIND_PENDING || (kind == KIND_CAPTURABLE && !fits);
            const unsigned long long mc = __ballot(fits), me = __ballot(kind == KIND_EMPTY), ml = __ballot(kind == KIND_LOST),
                                     mp = __ballot(pend);
            if (lane == 0) {
                wcnt[0][wave] = __popcll(mc);
                wcnt[1][wave] = __popcll(me);
                wcnt[2][wave] = __popcll(ml);
                wcnt[3][wave] = __popcll(mp);
            }
            // the captured candidates are a prefix of the capturable ones: the wave's last one ends its packed rows
            if (mc == 0ull ? lane == 0 : lane == 63 - __clzll((long long)mc)) wend[wave] = mc == 0ull ? 0 : first + rows;
            wg_sync();
            int res_rank = popc_below(mc | me | ml, lane), pend_rank = popc_below(mp, lane), tile_res = 0, tile_pend = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const int res = wcnt[0][w] + wcnt[1][w] + wcnt[2][w];
                if (w < wave) {
                    res_rank += res;
                    pend_rank += wcnt[3][w];
                }
                tile_res += res;
                tile_pend += wcnt[3][w];
                captured += wcnt[0][w];
                empty += wcnt[1][w];
                lost += wcnt[2][w];
                packed_rows = wend[w] > packed_rows ? wend[w] : packed_rows;
            }
            if (fits || kind == KIND_EMPTY || kind == KIND_LOST) {
                const int d = dir_base + res_rank;
                const int status = fits ? RO_SNAP_CAPTURED : (kind == KIND_EMPTY ? RO_SNAP_EMPTY : RO_SNAP_LOST);
                int64_t *out = reinterpret_cast<int64_t *>(a.dir + d);       // ro_snapshot_t, word by word
#pragma unroll
                for (int w = 0; w < EVENT_WORDS; ++w) out[w] = e.w[w];                       // event
                out[EVENT_WORDS] = lo;                                                       // first_row
                out[EVENT_WORDS + 1] = fits ? first * a.cols : 0;                            // offset
                out[EVENT_WORDS + 2] = (int64_t)(((uint64_t)(unsigned)s << 32) | (unsigned)(fits ? rows : 0));    // rows, slot
                out[EVENT_WORDS + 3] = (int64_t)(unsigned)status;                            // status, reserved = 0
                a.first_packed[d] = first;
            }
            if (pend && pend_base + pend_rank < a.pending_capacity) store_event(new_list + (pend_base + pend_rank), e);
            row_base += tile_rows;
            dir_base += tile_res;
            pend_base += tile_pend;
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

constexpr int COPY_WAVES = 4;
constexpr int COPY_STEPS = 4;                   // loads of 64 columns each in flight before the stores

// Every wave takes packed rows wave, wave + waves, ...; nothing to do when the plan's total is zero.  The entry of packed
// row p is the last one whose first packed row is at most p: the table never descends, an entry without rows in front of
// a captured one holds the same value and comes first, and every entry behind the last captured one holds at least the
// total.
__global__ __launch_bounds__(64 * COPY_WAVES) void snap_copy_kernel(SnapArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.head->packed_rows;
    const int64_t resolved = a.head->resolved;
    if (total <= 0) return;
    const unsigned waves = gridDim.x * COPY_WAVES;
    const unsigned me = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * COPY_WAVES + (threadIdx.x >> 6)));
    for (int64_t p = me; p < total; p += waves) {
        int64_t lo = 0, hi = resolved;           // the first entry whose first packed row lies beyond p
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.first_packed[mid] <= p) lo = mid + 1;
            else hi = mid;
        }
        if (lo == 0) continue;
        const ro_snapshot_t *en = a.dir + (lo - 1);
        const int64_t k = p - a.first_packed[lo - 1];
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

hipError_t launch_snapshots(const SnapArgs &a, hipStream_t s)
{
    if (a.slots < 1 || a.slots > SNAP_MAX_SLOTS || a.slot_mask == 0u || (a.slot_mask >> a.slots) != 0u || a.capacity < 0 ||
        a.pending_capacity < 0 || (a.capacity > 0 && (!a.events || !a.summary)) || !a.ring || a.ring_rows < 1 || a.cols < 1 ||
        a.ring_stride < a.cols || a.head_row < 0 || (a.pending_capacity > 0 && !a.pending) || !a.pending_count || !a.dir ||
        a.arena_floats < 0 || (a.arena_floats > 0 && !a.arena) || a.arena_rows != a.arena_floats / a.cols || !a.snap_summary ||
        !a.head || !a.first_packed || !a.pending_new ||
        (int64_t)a.slots * (a.capacity + a.pending_capacity) > SNAP_MAX_SLOTS * SNAP_MAX_CANDIDATES)
        return hipErrorInvalidValue;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    hipLaunchKernelGGL(snap_plan_kernel, dim3(1), dim3(T), 0, s, a);
    // the work is known on the device only: four workgroups per CU, every wave strides over the packed rows
    hipLaunchKernelGGL(snap_copy_kernel, dim3((unsigned)(4 * std::max(cus, 1))), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
