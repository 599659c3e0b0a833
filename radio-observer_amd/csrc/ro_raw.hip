// ro_raw.hip -- the raw I/Q of each event on the device: the samples behind every captured snapshot, cut straight out of
// the sample buffers the transform read (up to RO_MAX_IQ_SPANS of them, in their wire formats) and packed as (float)re,
// (float)im pairs into an arena with a directory.  What writeRaw() writes for a snapshot with includeRawData
// (src/BolidRecorder.cpp:262, src/WaterfallBackend.cpp:77-81, :214-267; FFTBackend::floatToInt, src/FFTBackend.h:250-254).
// include/ro_stft.h states the rules candidate by candidate.  There is no sample ring and no put kernel: only the events'
// own samples are touched.
//
// Plain launches, as in ro_snapshots.hip; no workgroup waits for another one of its launch, no atomics, so the same input
// gives the same bytes:
//   raw_plan_kernel   ONE workgroup walks the candidates (the pending list, then the snapshot directory's captured entries)
//                     RO_RAW_TILE at a time and carries three exclusive prefixes from tile to tile, all in 64 bits: the raw
//                     directory index, the packed pairs (a run's arena offset is twice its packed pair) and the packed
//                     blocks, besides the pending index.  It writes the raw directory, the new pending list (in place: a
//                     kept candidate lands at or in front of where it was read, and a tile is in registers before any
//                     of it is stored), the summary and the plan (ro_raw.h)
//   raw_copy_kernel   a grid sized by the host from the CU count; every wave strides over the blocks (RO_RAW_BLOCK pairs
//                     of ONE entry), finds a block's entry by binary search in the plan (the block index is wave-uniform:
//                     no divergent loop), and converts its pairs, lanes on consecutive pairs, one pair per lane and load:
//                     f is odd for every even hop, so a 16-byte load of two float pairs would be misaligned for almost
//                     every event (the wider form was not measured)
#include <algorithm>
#include <cstddef>

#include "ro_device_util.h"
#include "ro_raw.h"

namespace ro {

namespace {

constexpr int T = RO_RAW_TILE;
constexpr int WAVES = T / 64;
constexpr int64_t B = RO_RAW_BLOCK;
static_assert(T == 256 && WAVES == 4, "one candidate per lane, four waves");

enum { KIND_NONE = 0, KIND_PENDING, KIND_EMPTY, KIND_LOST, KIND_CAPTURABLE };

// A directory entry travels as its nine 64-bit words (every ABI struct here is 8-byte aligned and has no padding).
constexpr int EVENT_WORDS = sizeof(ro_event_t) / 8;
constexpr int SNAP_WORDS = sizeof(ro_snapshot_t) / 8;
static_assert(sizeof(ro_event_t) == 40 && sizeof(ro_snapshot_t) == 72 && offsetof(ro_event_t, start_row) == 8 &&
                  offsetof(ro_snapshot_t, first_row) == 40 && offsetof(ro_snapshot_t, rows) == 56 &&
                  offsetof(ro_snapshot_t, slot) == 60 && offsetof(ro_snapshot_t, status) == 64 &&
                  sizeof(ro_raw_capture_t) == 72 && offsetof(ro_raw_capture_t, first_sample) == 40 &&
                  offsetof(ro_raw_capture_t, samples) == 48 && offsetof(ro_raw_capture_t, offset) == 56 &&
                  offsetof(ro_raw_capture_t, slot) == 64 && offsetof(ro_raw_capture_t, status) == 68,
              "the words below are these fields");
struct SnapWords {
    int64_t w[SNAP_WORDS];
    __device__ __forceinline__ int64_t start_row() const { return w[1]; }
    __device__ __forceinline__ int64_t first_row() const { return w[5]; }
    __device__ __forceinline__ int64_t rows() const { return (int64_t)(int32_t)(uint32_t)w[7]; }
    __device__ __forceinline__ uint32_t slot() const { return (uint32_t)((uint64_t)w[7] >> 32); }
    __device__ __forceinline__ int32_t status() const { return (int32_t)(uint32_t)w[8]; }
};
__device__ __forceinline__ SnapWords load_snapshot(const ro_snapshot_t *p)
{
    SnapWords e;
    const int64_t *q = reinterpret_cast<const int64_t *>(p);
#pragma unroll
    for (int w = 0; w < SNAP_WORDS; ++w) e.w[w] = q[w];
    return e;
}
__device__ __forceinline__ void store_snapshot(ro_snapshot_t *p, const SnapWords &e)
{
    int64_t *q = reinterpret_cast<int64_t *>(p);
#pragma unroll
    for (int w = 0; w < SNAP_WORDS; ++w) q[w] = e.w[w];
}

__device__ __forceinline__ int popc_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// inclusive prefix sum of a 64-bit count over the 64 lanes: four runs of wave_inclusive_sum, on 16 bits each (64 x 65535
// fits a run with room to spare), put together modulo 2^64.  A run of up to 2^31 pairs and a tile of 256 of them need more
// than the two runs snap_plan_kernel makes for its rows.
__device__ __forceinline__ int64_t wave_inclusive_sum64(int64_t x)
{
    const uint64_t u = (uint64_t)x;
    uint64_t sum = 0;
#pragma unroll
    for (int limb = 0; limb < 4; ++limb)
        sum += (uint64_t)wave_inclusive_sum((unsigned)(u >> (16 * limb)) & 0xffffu) << (16 * limb);
    return (int64_t)sum;
}

// One workgroup.  Per tile: every lane classifies its candidate; the pairs and the blocks of the capturable ones are
// scanned (the waves' totals meet in LDS) -- a candidate FITS when the packed pairs up to and including its own are at most
// arena_floats / 2, and since the scan runs over every capturable candidate, fitting or not, nothing behind the first that
// does not fit can fit either.  What is resolved and what stays pending is known after that; both are ranked with ballots.
// (A capturable run lies inside the spans, which are real memory: the sums stay far below 2^63.)
__global__ __launch_bounds__(T) void raw_plan_kernel(RawArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wpairs[WAVES], wblocks[WAVES], wend_pairs[WAVES], wend_blocks[WAVES];
    __shared__ int wcnt[4][WAVES];               // captured, empty, lost, pending of each wave
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
        const int64_t inc_p = wave_inclusive_sum64(pairs), inc_b = wave_inclusive_sum64(blocks);
        if (lane == 63) {
            wpairs[wave] = inc_p;
            wblocks[wave] = inc_b;
        }
        wg_sync();
        int64_t first_p = pair_base + inc_p - pairs, first_b = block_base + inc_b - blocks, tile_p = 0, tile_b = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) {
                first_p += wpairs[w];
                first_b += wblocks[w];
            }
            tile_p += wpairs[w];
            tile_b += wblocks[w];
        }
        const bool fits = kind == KIND_CAPTURABLE && first_p + pairs <= arena_pairs;
        const bool pend = kind == KIND_PENDING || (kind == KIND_CAPTURABLE && !fits);
        const unsigned long long mc = __ballot(fits), me = __ballot(kind == KIND_EMPTY), ml = __ballot(kind == KIND_LOST),
                                 mp = __ballot(pend);
        if (lane == 0) {
            wcnt[0][wave] = __popcll(mc);
            wcnt[1][wave] = __popcll(me);
            wcnt[2][wave] = __popcll(ml);
            wcnt[3][wave] = __popcll(mp);
        }
        // the captured candidates are a prefix of the capturable ones: the wave's last one ends its packed pairs and blocks
        if (mc == 0ull ? lane == 0 : lane == 63 - __clzll((long long)mc)) {
            wend_pairs[wave] = mc == 0ull ? 0 : first_p + pairs;
            wend_blocks[wave] = mc == 0ull ? 0 : first_b + blocks;
        }
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
            used_pairs = wend_pairs[w] > used_pairs ? wend_pairs[w] : used_pairs;
            used_blocks = wend_blocks[w] > used_blocks ? wend_blocks[w] : used_blocks;
        }
        if (fits || kind == KIND_EMPTY || kind == KIND_LOST) {
            const int64_t d = dir_base + res_rank;
            const int status = fits ? RO_SNAP_CAPTURED : (kind == KIND_EMPTY ? RO_SNAP_EMPTY : RO_SNAP_LOST);
            int64_t *out = reinterpret_cast<int64_t *>(a.raw_dir + d);     // ro_raw_capture_t, word by word
#pragma unroll
            for (int w = 0; w < EVENT_WORDS; ++w) out[w] = e.w[w];                         // event
            out[EVENT_WORDS] = f;                                                          // first_sample
            out[EVENT_WORDS + 1] = fits ? L : 0;                                           // samples
            out[EVENT_WORDS + 2] = fits ? 2 * first_p : 0;                                 // offset
            out[EVENT_WORDS + 3] = (int64_t)(((uint64_t)(unsigned)status << 32) | e.slot());           // slot, status
            a.first_block[d] = first_b;
        }
        // (every candidate up to the end of this tile is in registers or done with: the list is compacted in place)
        if (pend && pend_base + pend_rank < a.pending_capacity) store_snapshot(a.pending + (pend_base + pend_rank), e);
        pair_base += tile_p;
        block_base += tile_b;
        dir_base += tile_res;
        pend_base += tile_pend;
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

constexpr int COPY_WAVES = 4;
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

// Every wave takes blocks wave, wave + waves, ...; nothing to do when the plan's total is zero.  The entry of block b is
// the last one whose first block is at most b: the table never descends, an entry without samples in front of a captured
// one holds the same value and comes first, and every entry behind the last captured one holds at least the total.
// A sample that several spans hold is read from the last: span i OWNS [first[i], first[i + 1]), the last one up to the
// head (no gap between spans, ends ascending: the owner holds the sample).  Which spans a block needs is wave-uniform, so
// the branches below are scalar; a block inside one span runs one of them, and only a block across a boundary runs two.
__global__ __launch_bounds__(64 * COPY_WAVES) void raw_copy_kernel(RawArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = a.head->blocks;
    const int64_t resolved = a.head->resolved;
    if (total <= 0) return;
    const unsigned waves = gridDim.x * COPY_WAVES;
    const unsigned me = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * COPY_WAVES + (threadIdx.x >> 6)));
    for (int64_t b = me; b < total; b += waves) {
        int64_t lo = 0, hi = resolved;           // the first entry whose first block lies beyond b
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.first_block[mid] <= b) lo = mid + 1;
            else hi = mid;
        }
        if (lo == 0) continue;
        const ro_raw_capture_t *en = a.raw_dir + (lo - 1);
        const int64_t p0 = (b - a.first_block[lo - 1]) * B;          // the block's first pair of the entry's run
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

hipError_t launch_raw(const RawArgs &a, hipStream_t s)
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
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    hipLaunchKernelGGL(raw_plan_kernel, dim3(1), dim3(T), 0, s, a);
    // the work is known on the device only: four workgroups per CU, every wave strides over the blocks
    hipLaunchKernelGGL(raw_copy_kernel, dim3((unsigned)(4 * std::max(cus, 1))), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
