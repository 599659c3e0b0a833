// ro_pack_plan.h -- "plan then copy", the scheme of ro_snapshots.hip, ro_raw.hip and ro_units.hip, said once.  Device code
// only; DESIGN.md 4.7 states the scheme and its invariants.
//
// The plan: ONE workgroup of PLAN_TILE lanes walks a list of candidates a tile at a time, one candidate per lane.  Per tile,
// tile_scan gives every lane the exclusive prefix of what the candidates would take of the room -- over EVERY candidate
// that would take some, fitting or not, so that nothing behind the first misfit fits -- and tile_count counts and ranks the
// classes and finds where the last fitting candidate ends.  One barrier in each; the LDS words are the kernel's own and are
// handed in, and the barrier of the next tile's scan is what lets tile_count's words be written again.  The kernel carries
// the tile totals on as the bases of the next tile and writes first[], the prefix in front of every entry, to scratch.
// The copy: copy_grid(cus) workgroups of COPY_WAVES waves; a wave finds the entry of a work item with plan_entry.
#pragma once

#include <algorithm>
#include <cstddef>

#include "../../include/ro_stft.h"
#include "ro_device_util.h"

namespace ro {

constexpr int PLAN_TILE = 256;                   // candidates of a tile: one per lane of the plan's one workgroup
constexpr int PLAN_WAVES = PLAN_TILE / 64;
constexpr int PLAN_CLASSES = 4;                  // what tile_count counts; class 0 is "fits"
constexpr int COPY_WAVES = 4;                    // waves of a copy workgroup

// the copy's grid: the work is known on the device only, so four workgroups per CU whatever there is
inline unsigned copy_grid(int cus) { return (unsigned)(4 * std::max(cus, 1)); }

__device__ __forceinline__ int popc_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// inclusive prefix sum of a 64-bit count over the 64 lanes: four runs of wave_inclusive_sum, on 16 bits each (64 x 65535
// fits a run with room to spare), put together modulo 2^64 -- a raw run of 2^31 pairs, and a tile of 256 of them, need more
// than one run holds
__device__ __forceinline__ int64_t wave_inclusive_sum64(int64_t x)
{
    const uint64_t u = (uint64_t)x;
    uint64_t sum = 0;
#pragma unroll
    for (int limb = 0; limb < 4; ++limb)
        sum += (uint64_t)wave_inclusive_sum((unsigned)(u >> (16 * limb)) & 0xffffu) << (16 * limb);
    return (int64_t)sum;
}

// K counts scanned together over the tile: before[k] is the sum of x[k] over the lanes in front of this one, total[k] the
// tile's.  The waves' totals meet in w (LDS, the caller's) behind ONE barrier.
template <int K> struct TileScan {
    int64_t before[K], total[K];
};
template <int K>
__device__ __forceinline__ TileScan<K> tile_scan(const int64_t (&x)[K], int64_t (&w)[K][PLAN_WAVES], int lane, int wave)
{
    TileScan<K> t;
    int64_t inc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) inc[k] = wave_inclusive_sum64(x[k]);
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < K; ++k) w[k][wave] = inc[k];
    }
    wg_sync();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        t.before[k] = inc[k] - x[k];
        t.total[k] = 0;
#pragma unroll
        for (int v = 0; v < PLAN_WAVES; ++v) {
            if (v < wave) t.before[k] += w[k][v];
            t.total[k] += w[k][v];
        }
    }
    return t;
}

// The classes of a tile, counted: total[c] candidates of class c in the tile, and rank(classes, lane), this lane's place
// among the tile's candidates of the classes in `classes` (bit c: class c).  end[k]: where the tile's last candidate of
// class 0 ends, 0 without one -- they are a prefix of those that take room, so the ends only grow and a wave's last one
// ends what the wave uses.
template <int K> struct TileCount {
    unsigned long long mask[PLAN_CLASSES];       // this wave's ballots
    int front[PLAN_CLASSES];                     // ... and what the waves in front of it count
    int total[PLAN_CLASSES];
    int64_t end[K];
    __device__ __forceinline__ int rank(unsigned classes, int lane) const
    {
        unsigned long long m = 0ull;
        int r = 0;
#pragma unroll
        for (int c = 0; c < PLAN_CLASSES; ++c)
            if ((classes >> c) & 1u) {
                m |= mask[c];
                r += front[c];
            }
        return r + popc_below(m, lane);
    }
};
// is[c]: this lane's candidate is of class c (at most one); my_end[k]: where it ends, looked at for class 0 only.  The
// waves' counts and ends meet in wcnt and wend (LDS, the caller's) behind ONE barrier.
template <int K>
__device__ __forceinline__ TileCount<K> tile_count(const bool (&is)[PLAN_CLASSES], const int64_t (&my_end)[K],
                                                   int (&wcnt)[PLAN_CLASSES][PLAN_WAVES], int64_t (&wend)[K][PLAN_WAVES],
                                                   int lane, int wave)
{
    TileCount<K> t;
#pragma unroll
    for (int c = 0; c < PLAN_CLASSES; ++c) t.mask[c] = __ballot(is[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < PLAN_CLASSES; ++c) wcnt[c][wave] = __popcll(t.mask[c]);
    }
    const unsigned long long m0 = t.mask[0];
    if (m0 == 0ull ? lane == 0 : lane == 63 - __clzll((long long)m0)) {
#pragma unroll
        for (int k = 0; k < K; ++k) wend[k][wave] = m0 == 0ull ? 0 : my_end[k];
    }
    wg_sync();
#pragma unroll
    for (int c = 0; c < PLAN_CLASSES; ++c) {
        t.front[c] = t.total[c] = 0;
#pragma unroll
        for (int v = 0; v < PLAN_WAVES; ++v) {
            if (v < wave) t.front[c] += wcnt[c][v];
            t.total[c] += wcnt[c][v];
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        t.end[k] = 0;
#pragma unroll
        for (int v = 0; v < PLAN_WAVES; ++v) t.end[k] = wend[k][v] > t.end[k] ? wend[k][v] : t.end[k];
    }
    return t;
}

// The entry of work item p: the last of first[0, n) that is at most p, or -1.  first[] never descends; of entries with
// equal values only the last has work (the others are empty entries in front of it), and the entries behind the last one
// with work hold at least the total, which no item reaches.
__device__ __forceinline__ int64_t plan_entry(const int64_t *first, int64_t n, int64_t p)
{
    int64_t lo = 0, hi = n;                      // the first entry beyond p
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (first[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// The copy's gather out of an arena of rows: float x of a cut that starts in a row at arena float `base` -- x counts from
// the row's first cut column on, a row of the cut is naxis1 floats and a row of the arena `stride` (x < 2^32, naxis1 >= 1) --
// clamped into [0, last], so that no load is guarded and none leaves the buffer
__device__ __forceinline__ int64_t cut_at(int64_t base, unsigned x, unsigned naxis1, int64_t stride, int64_t last)
{
    const unsigned dr = x / naxis1;
    const int64_t at = base + (int64_t)dr * stride + (x - dr * naxis1);
    return at < 0 ? 0 : (at > last ? last : at);
}

// this wave among the waves of the copy's grid: it takes items me, me + waves, ...
struct CopyWave {
    unsigned me, waves;
};
__device__ __forceinline__ CopyWave copy_wave()
{
    return CopyWave{(unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * COPY_WAVES + (threadIdx.x >> 6))),
                    gridDim.x * COPY_WAVES};
}

// ---- the ABI structs as 64-bit words: each is 8-byte aligned and has no padding; copied field by field, an event's float /
// int tail went through a private array
constexpr int EVENT_WORDS = sizeof(ro_event_t) / 8;
constexpr int SNAP_WORDS = sizeof(ro_snapshot_t) / 8;
constexpr int RAW_CAPTURE_WORDS = sizeof(ro_raw_capture_t) / 8;
static_assert(sizeof(ro_event_t) == 40 && offsetof(ro_event_t, start_row) == 8 && offsetof(ro_event_t, length) == 16 &&
                  sizeof(ro_snapshot_t) == 72 && offsetof(ro_snapshot_t, event) == 0 && offsetof(ro_snapshot_t, first_row) == 40 &&
                  offsetof(ro_snapshot_t, offset) == 48 && offsetof(ro_snapshot_t, rows) == 56 &&
                  offsetof(ro_snapshot_t, slot) == 60 && offsetof(ro_snapshot_t, status) == 64 &&
                  offsetof(ro_snapshot_t, reserved) == 68 && sizeof(ro_raw_capture_t) == 72 &&
                  offsetof(ro_raw_capture_t, event) == 0 && offsetof(ro_raw_capture_t, first_sample) == 40 &&
                  offsetof(ro_raw_capture_t, samples) == 48 && offsetof(ro_raw_capture_t, offset) == 56 &&
                  offsetof(ro_raw_capture_t, slot) == 64 && offsetof(ro_raw_capture_t, status) == 68,
              "the words below are these fields");

template <class W, class S> __device__ __forceinline__ W load_words(const S *p)
{
    static_assert(sizeof(W) == sizeof(S), "a word view of another struct");
    W e;
    const int64_t *q = reinterpret_cast<const int64_t *>(p);
#pragma unroll
    for (int w = 0; w < (int)(sizeof(S) / 8); ++w) e.w[w] = q[w];
    return e;
}
template <class W, class S> __device__ __forceinline__ void store_words(S *p, const W &e)
{
    static_assert(sizeof(W) == sizeof(S), "a word view of another struct");
    int64_t *q = reinterpret_cast<int64_t *>(p);
#pragma unroll
    for (int w = 0; w < (int)(sizeof(S) / 8); ++w) q[w] = e.w[w];
}

__device__ __forceinline__ int64_t two_int32(int32_t lo, int32_t hi) { return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }

struct EventWords {
    int64_t w[EVENT_WORDS];
    __device__ __forceinline__ int64_t start_row() const { return w[1]; }
    __device__ __forceinline__ int64_t length() const { return w[2]; }
};
__device__ __forceinline__ EventWords load_event(const ro_event_t *p) { return load_words<EventWords>(p); }
__device__ __forceinline__ void store_event(ro_event_t *p, const EventWords &e) { store_words(p, e); }

struct SnapWords {
    int64_t w[SNAP_WORDS];                       // the event first
    __device__ __forceinline__ int64_t start_row() const { return w[1]; }
    __device__ __forceinline__ int64_t first_row() const { return w[5]; }
    __device__ __forceinline__ int64_t offset() const { return w[6]; }
    __device__ __forceinline__ int32_t rows() const { return (int32_t)(uint32_t)w[7]; }
    __device__ __forceinline__ int32_t slot() const { return (int32_t)(uint32_t)((uint64_t)w[7] >> 32); }
    __device__ __forceinline__ int32_t status() const { return (int32_t)(uint32_t)w[8]; }
};
__device__ __forceinline__ SnapWords load_snapshot(const ro_snapshot_t *p) { return load_words<SnapWords>(p); }
__device__ __forceinline__ void store_snapshot(ro_snapshot_t *p, const SnapWords &e) { store_words(p, e); }
// the directory entry of an event (reserved = 0)
__device__ __forceinline__ SnapWords make_snapshot(const EventWords &event, int64_t first_row, int64_t offset, int32_t rows,
                                                   int32_t slot, int32_t status)
{
    SnapWords e;
#pragma unroll
    for (int w = 0; w < EVENT_WORDS; ++w) e.w[w] = event.w[w];
    e.w[5] = first_row;
    e.w[6] = offset;
    e.w[7] = two_int32(rows, slot);
    e.w[8] = two_int32(status, 0);
    return e;
}

struct RawCaptureWords {
    int64_t w[RAW_CAPTURE_WORDS];                // the event first
    __device__ __forceinline__ int64_t samples() const { return w[6]; }
    __device__ __forceinline__ int64_t offset() const { return w[7]; }
    __device__ __forceinline__ int32_t status() const { return (int32_t)(uint32_t)((uint64_t)w[8] >> 32); }
};
__device__ __forceinline__ RawCaptureWords load_raw_capture(const ro_raw_capture_t *p) { return load_words<RawCaptureWords>(p); }
__device__ __forceinline__ void store_raw_capture(ro_raw_capture_t *p, const RawCaptureWords &e) { store_words(p, e); }
// the raw directory entry of a snapshot: its event and its slot go along
__device__ __forceinline__ RawCaptureWords make_raw_capture(const SnapWords &snap, int64_t first_sample, int64_t samples,
                                                            int64_t offset, int32_t status)
{
    RawCaptureWords e;
#pragma unroll
    for (int w = 0; w < EVENT_WORDS; ++w) e.w[w] = snap.w[w];
    e.w[5] = first_sample;
    e.w[6] = samples;
    e.w[7] = offset;
    e.w[8] = two_int32(snap.slot(), status);
    return e;
}

}  // namespace ro
