// ro_raw.hip -- the raw I/Q of each event on the device: the samples behind every captured snapshot, cut straight out of
// the sample buffers the transform read (up to RO_MAX_IQ_SPANS of them, in their wire formats) and packed as (float)re,
// (float)im pairs into an arena with a directory.  What writeRaw() writes for a snapshot with includeRawData
// (src/BolidRecorder.cpp:262, src/WaterfallBackend.cpp:77-81, :214-267; FFTBackend::floatToInt, src/FFTBackend.h:250-254).
// include/ro_stft.h states the rules candidate by candidate.  There is no sample ring and no put kernel: only the events'
// own samples are touched.
//
// Plain launches, as in ro_snapshots.hip; no workgroup waits for another one of its launch, no atomics, so the same input
// gives the same bytes:
//   raw_plan_kernel   the plan of ro_pack_plan.h over the candidates (the pending list, then the snapshot directory's
//                     captured entries): what is scanned are the packed pairs (a run's arena offset is twice its packed
//                     pair) and, with them, the packed blocks; besides them the raw directory index and the pending index
//                     go from tile to tile.  It writes the raw directory, the new pending list (in place: a kept
//                     candidate lands at or in front of where it was read, and a tile is in registers before any of it is
//                     stored), the summary and the plan (ro_raw.h)
//   raw_copy_kernel   the copy of ro_pack_plan.h over the blocks (RO_RAW_BLOCK pairs of ONE entry): it converts a block's
//                     pairs, lanes on consecutive pairs, one pair per lane and load: f is odd for every even hop, so a
//                     16-byte load of two float pairs would be misaligned for almost every event (the wider form was not
//                     measured)
#include "ro_pack_plan.h"
#include "ro_raw.h"

namespace ro {

namespace {

constexpr int T = RO_RAW_TILE;
constexpr int64_t B = RO_RAW_BLOCK;
static_assert(T == PLAN_TILE, "one candidate per lane, four waves");

enum { KIND_NONE = 0, KIND_PENDING, KIND_EMPTY, KIND_LOST, KIND_CAPTURABLE };
constexpr unsigned RESOLVED = 0b0111u, PENDING = 0b1000u;    // of tile_count's classes: captured, empty, lost; pending

// The plan.  A candidate FITS when the packed pairs up to and including its own are at most arena_floats / 2; what is
// resolved goes to the raw directory, what stays pending to the front of the list, both in the order of the candidates.
// (A capturable run lies inside the spans, which are real memory: the sums stay far below 2^63.)
__global__ __launch_bounds__(T) void raw_plan_kernel(RawArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wsum[2][PLAN_WAVES], wend[2][PLAN_WAVES];     // pairs, blocks
    __shared__ int wcnt[PLAN_CLASSES][PLAN_WAVES];    // captured, empty, lost, pending of each wave
    int64_t have = *a.pending_count;             // (every lane reads it; lane 0 writes the new one at the end)
    have = have < 0 ? 0 : (have > a.pending_capacity ? a.pending_capacity : have);
    int64_t listed = a.snap_summary->resolved;
    listed = listed < 0 ? 0 : (listed > a.dir_capacity ? a.dir_capacity : listed);
    wg_sync();
    const int64_t n = have + listed;
    const int64_t arena_pairs = a.arena_floats >> 1;
    int64_t pair_base = 0, block_base = 0;       // packed pairs / blocks of the capturable candidates in front of the tile
    int64_t used_pairs = 0, used_blocks = 0;     // ... of the captured ones: where the last captured run ends
    int64_t dir_base = 0, pend_base = 0;
    int64_t captured = 0, empty = 0, lost = 0;
#pragma unroll 1
    for (int64_t t0 = 0; t0 < n; t0 += T) {
        const int64_t c = t0 + threadIdx.x;
        // (lanes past the last candidate read it once more and take no part: no guarded load of a struct)
        const int64_t cc = c < n ? c : n - 1;
        const SnapWords e = load_snapshot(cc < have ? a.pending + cc : a.dir + (cc - have));
        // every entry of the pending list is a candidate; of the directory, the captured images
        const bool live = c < n && (cc < have || e.status() == RO_SNAP_CAPTURED);
        const int64_t start = e.start_row();
        const int64_t len = e.rows() + (e.first_row() - start);
        const int64_t L = raw_length(len, a.rate_r, a.sample_rate);
        const int64_t f = raw_first_sample(start, a.hop, a.z);
        const int kind = !live ? KIND_NONE
                       : f + L > a.head_sample ? KIND_PENDING
                       : L <= 0 ? KIND_EMPTY
                       : f < a.base_sample ? KIND_LOST : KIND_CAPTURABLE;
        const int64_t pairs = kind == KIND_CAPTURABLE ? L : 0;
        const int64_t blocks = (pairs + B - 1) / B;
        const int64_t take[2] = {pairs, blocks};
        const TileScan<2> scan = tile_scan(take, wsum, lane, wave);
        const int64_t first_p = pair_base + scan.before[0], first_b = block_base + scan.before[1];
        const bool fits = kind == KIND_CAPTURABLE && first_p + pairs <= arena_pairs;
        const bool pend = kind == KIND_PENDING || (kind == KIND_CAPTURABLE && !fits);
        const bool is[PLAN_CLASSES] = {fits, kind == KIND_EMPTY, kind == KIND_LOST, pend};
        const int64_t end[2] = {first_p + pairs, first_b + blocks};
        const TileCount<2> count = tile_count(is, end, wcnt, wend, lane, wave);
        captured += count.total[0];
        empty += count.total[1];
        lost += count.total[2];
        used_pairs = count.end[0] > used_pairs ? count.end[0] : used_pairs;
        used_blocks = count.end[1] > used_blocks ? count.end[1] : used_blocks;
        if (fits || kind == KIND_EMPTY || kind == KIND_LOST) {
            const int64_t d = dir_base + count.rank(RESOLVED, lane);
            const int status = fits ? RO_SNAP_CAPTURED : (kind == KIND_EMPTY ? RO_SNAP_EMPTY : RO_SNAP_LOST);
            store_raw_capture(a.raw_dir + d, make_raw_capture(e, f, fits ? L : 0, fits ? 2 * first_p : 0, status));
            a.first_block[d] = first_b;
        }
        // (every candidate up to the end of this tile is in registers or done with: the list is compacted in place)
        const int64_t pend_at = pend_base + count.rank(PENDING, lane);
        if (pend && pend_at < a.pending_capacity) store_snapshot(a.pending + pend_at, e);
        pair_base += scan.total[0];
        block_base += scan.total[1];
        dir_base += count.total[0] + count.total[1] + count.total[2];
        pend_base += count.total[3];
    }
    if (threadIdx.x == 0) {
        const int64_t kept = pend_base < a.pending_capacity ? pend_base : a.pending_capacity;
        *a.pending_count = kept;
        ro_raw_summary_t sum;
        sum.resolved = dir_base;
        sum.captured = captured;
        sum.empty = empty;
        sum.lost = lost;
        sum.pending = kept;
        sum.pending_dropped = pend_base - kept;
        sum.arena_floats = 2 * used_pairs;
        sum.reserved = 0;
        *a.raw_summary = sum;
        RawPlanHead head;
        head.resolved = dir_base;
        head.blocks = used_blocks;
        *a.head = head;
    }
}

constexpr int STEPS = RO_RAW_BLOCK / 64;         // loads of 64 pairs each in flight before the stores
static_assert(STEPS * 64 == RO_RAW_BLOCK && STEPS == 8, "a block is eight pairs per lane");

typedef unsigned int u2 __attribute__((ext_vector_type(2)));

// a sample in its wire format, and the pair of float bit patterns it becomes (src/FFTBackend.h:250-254)
template <int FMT> struct RawSample;
template <> struct RawSample<RO_IQ_F32> {        // a bit copy: NaN payloads and -0 survive
    typedef u2 raw;
    static __device__ __forceinline__ raw load(const void *iq, int64_t i) { return static_cast<const u2 *>(iq)[i]; }
    static __device__ __forceinline__ u2 pair(raw r) { return r; }
};
template <> struct RawSample<RO_IQ_I16> {
    typedef unsigned raw;
    static __device__ __forceinline__ raw load(const void *iq, int64_t i) { return static_cast<const unsigned *>(iq)[i]; }
    static __device__ __forceinline__ u2 pair(raw r)
    {
        return (u2){__float_as_uint((float)(short)(r & 0xffffu)), __float_as_uint((float)(short)(r >> 16))};
    }
};
template <> struct RawSample<RO_IQ_F64> {        // round to nearest even, like the host's (float)
    struct raw { double re, im; };
    static __device__ __forceinline__ raw load(const void *iq, int64_t i)
    {
        const double *p = static_cast<const double *>(iq) + 2 * i;
        return raw{p[0], p[1]};
    }
    static __device__ __forceinline__ u2 pair(raw r) { return (u2){__float_as_uint((float)r.re), __float_as_uint((float)r.im)}; }
};

// The lanes' samples s, s + 64, ... of one span into v, where the span owns them: [own_lo, own_hi).  Every lane loads
// every step -- its index clamped into the span, so no load is guarded and none leaves the buffer -- and all loads are
// issued before the first value is looked at.
template <int FMT>
__device__ __forceinline__ void span_pairs(const void *iq, int64_t first, int64_t count, int64_t own_lo, int64_t own_hi,
                                           int64_t s, u2 (&v)[STEPS])
{
    typename RawSample<FMT>::raw r[STEPS];
#pragma unroll
    for (int q = 0; q < STEPS; ++q) {
        int64_t i = s + 64 * q - first;
        i = i < 0 ? 0 : (i >= count ? count - 1 : i);
        r[q] = RawSample<FMT>::load(iq, i);
    }
#pragma unroll
    for (int q = 0; q < STEPS; ++q) {
        const int64_t at = s + 64 * q;
        const u2 p = RawSample<FMT>::pair(r[q]);
        v[q] = (at >= own_lo && at < own_hi) ? p : v[q];
    }
}

// The copy: a work item is a block.  A sample that several spans hold is read from the last: span i OWNS [first[i], first[i + 1]), the last one up to the
// head (no gap between spans, ends ascending: the owner holds the sample).  Which spans a block needs is wave-uniform, so
// the branches below are scalar; a block inside one span runs one of them, and only a block across a boundary runs two.
__global__ __launch_bounds__(64 * COPY_WAVES) void raw_copy_kernel(RawArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.head->blocks;
    const int64_t resolved = a.head->resolved;
    if (total <= 0) return;
    const CopyWave wv = copy_wave();
    for (int64_t b = wv.me; b < total; b += wv.waves) {
        const int64_t d = plan_entry(a.first_block, resolved, b);
        if (d < 0) continue;
        const ro_raw_capture_t *en = a.raw_dir + d;
        const int64_t p0 = (b - a.first_block[d]) * B;               // the block's first pair of the entry's run
        const int64_t L = en->samples, offset = en->offset;
        if (en->status != RO_SNAP_CAPTURED || p0 >= L || offset < 0 || offset + 2 * L > a.arena_floats) continue;
        const int64_t n = L - p0 < B ? L - p0 : B;                   // pairs of this block
        const int64_t s0 = en->first_sample + p0;                    // its first sample: [s0, s0 + n) lies inside the spans
        u2 v[STEPS];
#pragma unroll
        for (int q = 0; q < STEPS; ++q) v[q] = (u2){0u, 0u};
#pragma unroll
        for (int i = 0; i < RO_MAX_IQ_SPANS; ++i) {                  // (constant indices: the tables stay in the kernel arguments)
            if (i >= a.spans) continue;
            const int64_t own_lo = a.first[i];
            const int64_t own_hi = (i + 1 < RO_MAX_IQ_SPANS && i + 1 < a.spans) ? a.first[(i + 1) % RO_MAX_IQ_SPANS] : a.head_sample;
            if (s0 + n <= own_lo || s0 >= own_hi) continue;
            if (a.format[i] == RO_IQ_F32) span_pairs<RO_IQ_F32>(a.iq[i], a.first[i], a.count[i], own_lo, own_hi, s0 + lane, v);
            else if (a.format[i] == RO_IQ_I16) span_pairs<RO_IQ_I16>(a.iq[i], a.first[i], a.count[i], own_lo, own_hi, s0 + lane, v);
            else span_pairs<RO_IQ_F64>(a.iq[i], a.first[i], a.count[i], own_lo, own_hi, s0 + lane, v);
        }
        u2 *out = reinterpret_cast<u2 *>(a.arena + offset) + p0 + lane;
#pragma unroll
        for (int q = 0; q < STEPS; ++q)
            if (64 * q + lane < n) out[64 * q] = v[q];
    }
}

}  // namespace

size_t raw_scratch_bytes(int64_t dir_capacity, int64_t pending_capacity)
{
    return sizeof(RawPlanHead) + (size_t)(dir_capacity + pending_capacity) * sizeof(int64_t);
}

void raw_scratch_layout(RawArgs &a, void *scratch)
{
    char *p = static_cast<char *>(scratch);
    a.head = reinterpret_cast<RawPlanHead *>(p);
    a.first_block = reinterpret_cast<int64_t *>(p + sizeof(RawPlanHead));
}

hipError_t launch_raw(const RawArgs &a, int cus, hipStream_t s)
{
    if (a.dir_capacity < 0 || a.pending_capacity < 0 || a.dir_capacity + a.pending_capacity > RAW_MAX_CANDIDATES ||
        (a.dir_capacity > 0 && !a.dir) || !a.snap_summary || a.spans < 1 || a.spans > RO_MAX_IQ_SPANS || a.hop < 1 ||
        !(a.rate_r != 0.0) || (a.pending_capacity > 0 && !a.pending) || !a.pending_count || !a.raw_dir || a.arena_floats < 0 ||
        (a.arena_floats > 0 && !a.arena) || ((uintptr_t)a.arena & 7u) != 0 || !a.raw_summary || !a.head || !a.first_block)
        return hipErrorInvalidValue;
    for (int i = 0; i < a.spans; ++i) {
        const bool known = a.format[i] == RO_IQ_F32 || a.format[i] == RO_IQ_I16 || a.format[i] == RO_IQ_F64;
        if (!a.iq[i] || !known || a.first[i] < 0 || a.count[i] < 1 || ((uintptr_t)a.iq[i] & (a.format[i] == RO_IQ_I16 ? 3u : 7u)) != 0 ||
            (i > 0 && (a.first[i] <= a.first[i - 1] || a.first[i] + a.count[i] <= a.first[i - 1] + a.count[i - 1] ||
                       a.first[i] > a.first[i - 1] + a.count[i - 1])))
            return hipErrorInvalidValue;
    }
    if (a.base_sample != a.first[0] || a.head_sample != a.first[a.spans - 1] + a.count[a.spans - 1]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(raw_plan_kernel, dim3(1), dim3(T), 0, s, a);
    hipLaunchKernelGGL(raw_copy_kernel, dim3(copy_grid(cus)), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
