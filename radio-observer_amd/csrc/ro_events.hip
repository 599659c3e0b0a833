// ro_events.hip -- the detector of BolidRecorder::update on the device: the decision (src/BolidRecorder.cpp:135) and the
// three-state machine (:171-267) over scan records that are already in HBM, for up to 8 band sets (SLOTS) at once.  Events
// come out; no record travels to the host.
//
// The machine is a scan (include/ro_stft.h has its closed form).  Over a run of rows keep the SUMMARY (first, last,
// gstart): its first and last detect row and the start of the group that holds `last`, as far as the run alone can tell;
// a run without a detect row is EMPTY.  A (+) B: EMPTY is the identity; else first = A.first, last = B.last, and gstart =
// B.gstart if B.gstart != B.first (the group began inside B behind B's first detect row), else B.first if the quiet rows
// between A.last and B.first are G or more (A's group fired in between), else A.gstart.  With P the exclusive prefix of
// row r, carried state included, row r FIRES when it is quiet, P is not empty and r = P.last + G; the event is the group
// [P.gstart, P.last].
//
// Three plain launches per chunk of RO_EVENTS_CHUNK_ROWS rows; no workgroup waits for another one of its launch (the rule
// DESIGN.md 7 drew from the one-launch FP64 form), no atomics, so the same input gives the same bits:
//   1 events_reduce_kernel  a tile of RO_EVENTS_TILE_ROWS rows of one slot -> its (+) total and its counts
//   2 events_scan_kernel    one workgroup per slot: exclusive scan of the tile totals seeded with d_state; writes the new
//                           state and the summary
//   3 events_emit_kernel    a tile again: in-tile scan from its prefix, events at prefix_fires + local index, detect bytes
// Inside a wave the three integers of the summary are scanned with DPP moves (row_shr 1, 2, 4, 8, row_bcast 15 and 31: the
// ladder of wave_inclusive_sum with (+) in the place of +).  They are counted FROM 1 inside the tile (pass 1, 3) or the
// chunk (pass 2), so that EMPTY is (0, 0, 0) -- what a DPP move hands a lane whose source lies outside its row.  Stream
// rows are int64 and only appear where a prefix meets the carried state.
#include "ro_device_util.h"
#include "ro_events.h"

namespace ro {

namespace {

constexpr int T = RO_EVENTS_TILE_ROWS;
constexpr int WAVES = T / 64;
constexpr int PER = EVENTS_MAX_TILES / T;          // tiles per lane of pass 2
static_assert(T == 256 && WAVES == 4, "one row per lane, four waves");
static_assert(PER * T == EVENTS_MAX_TILES, "pass 2 scans a chunk's tiles with one workgroup");

struct Sum {
    int first, last, gstart;                       // counted from 1; (0, 0, 0): empty
};

__device__ __forceinline__ Sum combine(Sum a, Sum b, int G)
{
    Sum r;
    r.first = a.first;
    r.last = b.last;
    r.gstart = b.gstart != b.first ? b.gstart : (b.first - a.last - 1 >= G ? b.first : a.gstart);
    if (a.last == 0) r = b;
    if (b.last == 0) r = a;
    return r;
}

template <int CTRL, int ROWS> __device__ __forceinline__ Sum dpp_sum(Sum v)
{
    Sum r;                                         // lanes without a source, and rows outside ROWS, read EMPTY
    r.first = __builtin_amdgcn_update_dpp(0, v.first, CTRL, ROWS, 0xf, true);
    r.last = __builtin_amdgcn_update_dpp(0, v.last, CTRL, ROWS, 0xf, true);
    r.gstart = __builtin_amdgcn_update_dpp(0, v.gstart, CTRL, ROWS, 0xf, true);
    return r;
}

// inclusive (+) prefix over the 64 lanes; lane 63 holds the wave's total
__device__ __forceinline__ Sum wave_inclusive(Sum v, int G)
{
    v = combine(dpp_sum<0x111, 0xf>(v), v, G);     // row_shr:1
    v = combine(dpp_sum<0x112, 0xf>(v), v, G);     // row_shr:2
    v = combine(dpp_sum<0x114, 0xf>(v), v, G);     // row_shr:4
    v = combine(dpp_sum<0x118, 0xf>(v), v, G);     // row_shr:8
    v = combine(dpp_sum<0x142, 0xa>(v), v, G);     // row_bcast:15 -> rows 1 and 3
    v = combine(dpp_sum<0x143, 0xc>(v), v, G);     // row_bcast:31 -> rows 2 and 3
    return v;
}

// exclusive (+) prefix over the workgroup's 256 lanes, and their total; wtot: WAVES entries of LDS (the caller keeps a
// barrier between two uses of it)
__device__ __forceinline__ Sum block_exclusive(Sum v, int G, Sum *wtot, Sum *total)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const Sum inc = wave_inclusive(v, G);
    Sum ex;
    ex.first = __shfl_up(inc.first, 1, 64);
    ex.last = __shfl_up(inc.last, 1, 64);
    ex.gstart = __shfl_up(inc.gstart, 1, 64);
    if (lane == 0) ex = Sum{0, 0, 0};
    if (lane == 63) wtot[wave] = inc;
    wg_sync();
    Sum pre{0, 0, 0}, all{0, 0, 0};
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) pre = combine(pre, wtot[w], G);
        all = combine(all, wtot[w], G);
    }
    *total = all;
    return combine(pre, ex, G);
}

// a prefix in stream rows: what stands in front of a row once the carried state is in
struct Prefix {
    int64_t last, gstart;
    bool open;
};

// A (+) B with A in stream rows and B counted from 1 at stream row `base`
__device__ __forceinline__ Prefix with_front(Prefix a, Sum b, int64_t base, int64_t G)
{
    if (b.last == 0) return a;
    const int64_t bf = base + b.first - 1, bg = base + b.gstart - 1;
    Prefix r;
    r.open = true;
    r.last = base + b.last - 1;
    r.gstart = (!a.open || b.gstart != b.first) ? bg : (bf - a.last - 1 >= G ? bf : a.gstart);
    return r;
}

// the records of a slot: record of chunk row i at p[i * stride]; p == nullptr: the slot is not asked for
struct SlotRecords {
    const ro_scan_record_t *p;
    int64_t stride;
};
__device__ __forceinline__ SlotRecords slot_records(const EventsArgs &a, int slot)
{
    if (slot == 0) return SlotRecords{a.primary, 1};
    return SlotRecords{a.extra ? a.extra + (slot - 1) : nullptr, (int64_t)a.count};
}

// src/BolidRecorder.cpp:135, `a > (n * 2.0)` with float a and n: both sides are doubles.  *marginal: the decision is within
// 1e-5 of its threshold.
__device__ __forceinline__ bool decide(const ro_scan_record_t *rec, bool *marginal)
{
    const double n = (double)rec->noise, a = (double)rec->average;
    *marginal = fabs(a / (2.0 * n) - 1.0) <= 1e-5;
    return a > n * 2.0;
}

__device__ __forceinline__ int jitter_rows(ro_detector_t d) { return d.jitter > 2 ? d.jitter : 2; }

// exclusive count over the workgroup of the lanes with `flag`, and the workgroup's count; wcnt: WAVES words of LDS
__device__ __forceinline__ int block_rank(bool flag, int *wcnt, int *total)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wcnt[wave] = __popcll(m);
    wg_sync();
    int before = __popcll(m & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += wcnt[w];
        all += wcnt[w];
    }
    *total = all;
    return before;
}

// ---- pass 1: workgroup (tile, slot) reduces rows [tile * T, +T) of the chunk ------------------------------------------
__global__ __launch_bounds__(T) void events_reduce_kernel(EventsArgs a)
{
    const int slot = blockIdx.y;
    const SlotRecords rec = slot_records(a, slot);
    if (!rec.p) return;                            // (the whole workgroup: nothing below is reached by a part of it)
    const int G = jitter_rows(a.det[slot]);
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;         // row of the chunk
    bool marginal = false;
    const bool detect = i < a.rows && decide(rec.p + i * rec.stride, &marginal);
    const int me = (int)threadIdx.x + 1;
    __shared__ Sum wtot[WAVES];
    __shared__ int wcnt[3][WAVES];
    Sum total;
    const Sum before = block_exclusive(detect ? Sum{me, me, me} : Sum{0, 0, 0}, G, wtot, &total);
    // fire rows whose group's last detect row lies in this tile (G may exceed the tile: then there are none)
    const bool fire = i < a.rows && !detect && before.last != 0 && me - before.last == G;
    int fires, detects, marginals;
    block_rank(fire, wcnt[0], &fires);
    block_rank(detect, wcnt[1], &detects);
    block_rank(marginal, wcnt[2], &marginals);
    if (threadIdx.x == 0) {
        const int base = (int)blockIdx.x * T;      // tile-relative from 1 -> chunk-relative from 1
        EventsTileTotal t;
        t.first = total.last ? base + total.first : 0;
        t.last = total.last ? base + total.last : 0;
        t.gstart = total.last ? base + total.gstart : 0;
        t.fires = fires;
        t.detect_rows = detects;
        t.marginal_rows = marginals;
        a.totals[(size_t)slot * EVENTS_MAX_TILES + blockIdx.x] = t;
    }
}

// ---- pass 2: workgroup `slot` scans the chunk's tile totals, seeded with the carried state ----------------------------
__global__ __launch_bounds__(T) void events_scan_kernel(EventsArgs a, int tiles)
{
    const int slot = blockIdx.x;
    const SlotRecords rec = slot_records(a, slot);
    if (!rec.p) return;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int G = jitter_rows(a.det[slot]);
    const int64_t end = a.first_row + a.rows;
    // the carried state (every lane reads it; lane 0 writes the new one behind the barriers below).  A group that could
    // no longer fire -- rows were left out between two calls -- is closed silently.
    const ro_detect_state_t st = a.state[slot];
    Prefix carry;
    carry.open = st.open != 0 && st.last_detect_row + G >= a.first_row;
    carry.last = st.last_detect_row;
    carry.gstart = st.first_detect_row;
    // PER consecutive tiles per lane: serial (+) over them, the workgroup's scan over the lanes' totals
    const EventsTileTotal *totals = a.totals + (size_t)slot * EVENTS_MAX_TILES;
    const int per = (tiles + T - 1) / T;
    const int tile0 = (int)threadIdx.x * per;
    EventsTileTotal tt[PER];
    Sum ex[PER];
    Sum acc{0, 0, 0};
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const bool valid = k < per && tile0 + k < tiles;
        tt[k] = valid ? totals[tile0 + k] : EventsTileTotal{0, 0, 0, 0, 0, 0};
        ex[k] = acc;
        acc = combine(acc, Sum{tt[k].first, tt[k].last, tt[k].gstart}, G);
    }
    __shared__ Sum wtot[WAVES];
    __shared__ int wsum[3][WAVES];
    Sum chunk_total;
    const Sum lane_front = block_exclusive(acc, G, wtot, &chunk_total);
    // every tile's prefix in stream rows, and the one fire row a group from before the tile may have in it: P.last + G, if
    // it lies in the tile in front of the tile's first detect row (no row in between is a detect row, so it is quiet)
    Prefix pre[PER];
    int fires[PER];
    int my_fires = 0, my_detects = 0, my_marginals = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        pre[k] = with_front(carry, combine(lane_front, ex[k], G), a.first_row, G);
        const int64_t t0 = a.first_row + (int64_t)(tile0 + k) * T;
        const int64_t t1 = t0 + T < end ? t0 + T : end;
        const int64_t f = pre[k].last + G;
        const bool mine = k < per && tile0 + k < tiles;                 // (k >= per is the next lane's tile, and tt[k] zeros)
        const bool across = mine && pre[k].open && f >= t0 && f < t1 && (tt[k].last == 0 || f < a.first_row + tt[k].first - 1);
        fires[k] = tt[k].fires + (across ? 1 : 0);
        my_fires += fires[k];
        my_detects += tt[k].detect_rows;
        my_marginals += tt[k].marginal_rows;
    }
    const int inc_fires = (int)wave_inclusive_sum((unsigned)my_fires);
    const int inc_detects = (int)wave_inclusive_sum((unsigned)my_detects);
    const int inc_marginals = (int)wave_inclusive_sum((unsigned)my_marginals);
    if (lane == 63) {
        wsum[0][wave] = inc_fires;
        wsum[1][wave] = inc_detects;
        wsum[2][wave] = inc_marginals;
    }
    wg_sync();
    int fires_front = inc_fires - my_fires, all_fires = 0, all_detects = 0, all_marginals = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) fires_front += wsum[0][w];
        all_fires += wsum[0][w];
        all_detects += wsum[1][w];
        all_marginals += wsum[2][w];
    }
    EventsSlotHead *head = a.heads + slot;
    const int64_t call_events = a.accumulate ? head->events : 0;       // (lane 0 writes it behind the next barrier)
    const int64_t call_detects = a.accumulate ? head->detect_rows : 0;
    const int64_t call_marginals = a.accumulate ? head->marginal_rows : 0;
    EventsTilePrefix *prefix = a.prefix + (size_t)slot * EVENTS_MAX_TILES;
    int64_t fires_before = call_events + fires_front;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (k < per && tile0 + k < tiles) {
            EventsTilePrefix p;
            p.last = pre[k].open ? pre[k].last : 0;
            p.gstart = pre[k].open ? pre[k].gstart : 0;
            p.fires_before = fires_before;
            p.open = pre[k].open ? 1 : 0;
            p.pad = 0;
            prefix[tile0 + k] = p;
        }
        fires_before += fires[k];
    }
    wg_sync();
    if (threadIdx.x == 0) {
        // the state behind the chunk: open exactly when the fire row of the last group lies beyond it
        const Prefix all = with_front(carry, chunk_total, a.first_row, G);
        ro_detect_state_t ns{};
        if (all.open && all.last + G >= end) {
            ns.first_detect_row = all.gstart;
            ns.last_detect_row = all.last;
            ns.open = 1;
            if (all.gstart >= a.first_row) {
                const ro_scan_record_t r = rec.p[(all.gstart - a.first_row) * rec.stride];
                ns.noise = r.noise;
                ns.peak = r.peak;
                ns.magnitude = r.average;
            } else {
                ns.noise = st.noise;
                ns.peak = st.peak;
                ns.magnitude = st.magnitude;
            }
        }
        a.state[slot] = ns;
        EventsSlotHead nh;
        nh.noise = st.noise;                       // pass 3 reads the record of a group that began before the chunk here
        nh.peak = st.peak;
        nh.magnitude = st.magnitude;
        nh.pad = 0;
        nh.events = call_events + all_fires;
        nh.detect_rows = call_detects + all_detects;
        nh.marginal_rows = call_marginals + all_marginals;
        *head = nh;
        if (a.summary) {
            ro_detect_summary_t s;
            s.events = nh.events;
            s.detect_rows = nh.detect_rows;
            s.marginal_rows = nh.marginal_rows;
            a.summary[slot] = s;
        }
    }
}

// ---- pass 3: workgroup (tile, slot) redoes its scan from the tile's prefix and writes what fires ----------------------
__global__ __launch_bounds__(T) void events_emit_kernel(EventsArgs a)
{
    const int slot = blockIdx.y;
    const SlotRecords rec = slot_records(a, slot);
    if (!rec.p) return;
    const ro_detector_t det = a.det[slot];
    const int G = jitter_rows(det);
    const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;         // row of the chunk
    const int64_t row = a.first_row + i;
    bool marginal = false;
    const bool detect = i < a.rows && decide(rec.p + i * rec.stride, &marginal);
    const int me = (int)threadIdx.x + 1;
    __shared__ Sum wtot[WAVES];
    __shared__ int wcnt[WAVES];
    Sum total;
    const Sum before = block_exclusive(detect ? Sum{me, me, me} : Sum{0, 0, 0}, G, wtot, &total);
    const EventsTilePrefix tp = a.prefix[(size_t)slot * EVENTS_MAX_TILES + blockIdx.x];
    const Prefix front{tp.last, tp.gstart, tp.open != 0};
    const Prefix p = with_front(front, before, a.first_row + (int64_t)blockIdx.x * T, G);
    const bool fire = i < a.rows && !detect && p.open && row == p.last + G;
    int fires;
    const int64_t at = tp.fires_before + block_rank(fire, wcnt, &fires);
    if (fire && at < a.capacity) {
        ro_event_t e;
        e.fire_row = row;
        e.start_row = p.gstart + 1 - det.advance;
        e.length = 2 * (int64_t)det.advance + (p.last - p.gstart + 1);
        if (p.gstart >= a.first_row) {
            const ro_scan_record_t r = rec.p[(p.gstart - a.first_row) * rec.stride];
            e.noise = r.noise;
            e.peak = r.peak;
            e.magnitude = r.average;
        } else {
            const EventsSlotHead h = a.heads[slot];
            e.noise = h.noise;
            e.peak = h.peak;
            e.magnitude = h.magnitude;
        }
        e.reserved = 0;
        a.events[(int64_t)slot * a.capacity + at] = e;
    }
    if (a.detect && i < a.rows) a.detect[i * (1 + a.count) + slot] = detect ? 1 : 0;
}

}  // namespace

void events_scratch_layout(EventsArgs &a, void *scratch)
{
    char *p = static_cast<char *>(scratch);
    a.heads = reinterpret_cast<EventsSlotHead *>(p);
    p += EVENTS_MAX_SLOTS * sizeof(EventsSlotHead);
    a.prefix = reinterpret_cast<EventsTilePrefix *>(p);
    p += (size_t)EVENTS_MAX_SLOTS * EVENTS_MAX_TILES * sizeof(EventsTilePrefix);
    a.totals = reinterpret_cast<EventsTileTotal *>(p);
}

hipError_t launch_events(const EventsArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    if (a.rows > RO_EVENTS_CHUNK_ROWS || a.count < 0 || a.count > RO_MAX_EXTRA_BANDS || (!a.primary && !a.extra) ||
        !a.state || !a.heads || !a.totals || !a.prefix || a.capacity < 0 || (a.capacity > 0 && !a.events))
        return hipErrorInvalidValue;
    const int tiles = (int)((a.rows + T - 1) / T);
    const int slots = 1 + a.count;
    hipLaunchKernelGGL(events_reduce_kernel, dim3(tiles, slots), dim3(T), 0, s, a);
    hipLaunchKernelGGL(events_scan_kernel, dim3(slots), dim3(T), 0, s, a, tiles);
    hipLaunchKernelGGL(events_emit_kernel, dim3(tiles, slots), dim3(T), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
