#!/usr/bin/env python3
"""The event snapshots of include/ro_stft.h (ro_snapshots_host, ro_stft_snapshots_resident) restated in numpy, twice:

  snapshots        the rules candidate by candidate, literally: a slot's candidates are its pending list followed by the
                   call's events; still pending / EMPTY / LOST / capturable in that order; `offset` the exclusive prefix
                   sum of the capturable sizes, fitting or not; CAPTURED where offset + size <= arena_floats
  snapshots_plan   the kernels of csrc/ro_snapshots.hip: one workgroup walks the candidates TILE at a time and carries the
                   directory index, the packed rows and the slot's pending index; the new pending list is written to a
                   second copy and goes back behind the slot; the copy kernel finds each packed row's entry by binary
                   search in the plan's table of first packed rows
Neither looks at the library.  tests/test_snapshots_cpu.py holds ro_snapshots_host to `snapshots`; main() holds the two
against each other on random cases with a tile of a few candidates, so that most cases cross tile seams.

Run it: python tools/snapshots/emu_snapshots.py [cases]     (exit status 0 and a line "ok ..." when everything agrees)
"""
import sys

import numpy as np

EVENT_DTYPE = np.dtype([("fire_row", np.int64), ("start_row", np.int64), ("length", np.int64), ("noise", np.float32),
                        ("peak", np.int32), ("magnitude", np.float32), ("reserved", np.int32)])
SNAPSHOT_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_row", np.int64), ("offset", np.int64), ("rows", np.int32),
                           ("slot", np.int32), ("status", np.int32), ("reserved", np.int32)])
SNAP_SUMMARY_DTYPE = np.dtype([("resolved", np.int64), ("captured", np.int64), ("empty", np.int64), ("lost", np.int64),
                               ("pending", np.int64), ("pending_dropped", np.int64), ("unlisted", np.int64),
                               ("arena_floats", np.int64)])
CAPTURED, EMPTY, LOST = 0, 1, 2
PENDING, CAPTURABLE = -1, -2                             # (not statuses: what a candidate is before the arena is asked)


def classify(e, snapshot_rows, head_row, ring_rows):
    """(kind, lo, hi) of one candidate"""
    length = min(int(e["length"]), int(snapshot_rows))
    lo = max(int(e["start_row"]), 0)
    hi = int(e["start_row"]) + length
    if hi > head_row:
        return PENDING, lo, hi
    if hi <= lo:
        return EMPTY, lo, hi
    if lo < head_row - ring_rows:
        return LOST, lo, hi
    return CAPTURABLE, lo, hi


def candidates(events, summary, capacity, pending, pending_count, s):
    pcap = pending.shape[1]
    have = min(max(int(pending_count[s]), 0), pcap)
    fired = max(int(summary[s]["events"]), 0) if summary is not None else 0
    listed = min(fired, capacity)
    cand = [pending[s, i].copy() for i in range(have)] + [events[s, i].copy() for i in range(listed)]
    return cand, fired - listed


def entry(e, lo, offset, rows, slot, status):
    out = np.zeros(1, SNAPSHOT_DTYPE)
    out[0] = (e, lo, offset, rows, slot, status, 0)
    return out[0]


def snapshots(events, summary, slot_mask, snapshot_rows, ring, cols, head_row, pending, pending_count, arena_floats):
    """events [slots, capacity] / summary [slots] (None, None: no events); ring float32 [ring_rows, stride]; pending [slots,
    pending_capacity] and pending_count [slots] are updated in place.  Returns (directory, arena, summary): the resolved
    entries, arena_floats floats (NaN where nothing was written), a SNAP_SUMMARY_DTYPE scalar."""
    slots = int(slot_mask).bit_length()
    capacity = 0 if events is None else events.shape[1]
    pcap = pending.shape[1]
    ring_rows = ring.shape[0]
    directory = []
    arena = np.full(arena_floats, np.nan, np.float32)
    sm = np.zeros(1, SNAP_SUMMARY_DTYPE)[0]
    offset = 0
    for s in range(slots):
        if not (slot_mask >> s) & 1:
            continue
        cand, unlisted = candidates(events, summary, capacity, pending, pending_count, s)
        sm["unlisted"] += unlisted
        still = []
        for e in cand:
            kind, lo, hi = classify(e, snapshot_rows[s], head_row, ring_rows)
            if kind == PENDING:
                still.append(e)
            elif kind in (EMPTY, LOST):
                directory.append(entry(e, lo, 0, 0, s, kind))
                sm["empty" if kind == EMPTY else "lost"] += 1
            else:
                size = (hi - lo) * cols
                if offset + size <= arena_floats:
                    for k in range(hi - lo):
                        arena[offset + k * cols:offset + (k + 1) * cols] = ring[(lo + k) % ring_rows, :cols]
                    directory.append(entry(e, lo, offset, hi - lo, s, CAPTURED))
                    sm["captured"] += 1
                    sm["arena_floats"] = offset + size
                else:
                    still.append(e)
                offset += size
        kept = still[:pcap]
        for i, e in enumerate(kept):
            pending[s, i] = e
        pending_count[s] = len(kept)
        sm["pending"] += len(kept)
        sm["pending_dropped"] += len(still) - len(kept)
    sm["resolved"] = len(directory)
    out = np.zeros(len(directory), SNAPSHOT_DTYPE)
    for i, d in enumerate(directory):
        out[i] = d
    return out, arena, sm


def snapshots_plan(events, summary, slot_mask, snapshot_rows, ring, cols, head_row, pending, pending_count, arena_floats,
                   tile=256, waves=7):
    """the same outputs the way the kernels get them"""
    slots = int(slot_mask).bit_length()
    capacity = 0 if events is None else events.shape[1]
    pcap = pending.shape[1]
    ring_rows = ring.shape[0]
    arena_rows = arena_floats // cols
    directory = np.zeros(slots * (capacity + pcap), SNAPSHOT_DTYPE)
    first_packed = np.zeros(slots * (capacity + pcap), np.int64)
    pending_new = np.zeros_like(pending)
    sm = np.zeros(1, SNAP_SUMMARY_DTYPE)[0]
    row_base, packed_rows, dir_base = 0, 0, 0
    # ---- snap_plan_kernel
    for s in range(slots):
        if not (slot_mask >> s) & 1:
            continue
        cand, unlisted = candidates(events, summary, capacity, pending, pending_count, s)
        sm["unlisted"] += unlisted
        pend_base = 0
        for t0 in range(0, len(cand), tile):
            lanes = cand[t0:t0 + tile]
            kinds = [classify(e, snapshot_rows[s], head_row, ring_rows) for e in lanes]
            rows = np.array([hi - lo if k == CAPTURABLE else 0 for k, lo, hi in kinds], np.int64)
            lo16, hi16 = rows & 0xffff, rows >> 16               # two 32-bit ladders put together as int64
            inc = (np.cumsum(hi16) << 16) + np.cumsum(lo16)
            first = row_base + inc - rows
            capturable = np.array([k == CAPTURABLE for k, _, _ in kinds])
            fits = capturable & (first + rows <= arena_rows)
            resolved = fits | np.array([k in (EMPTY, LOST) for k, _, _ in kinds])
            pend = np.array([k == PENDING for k, _, _ in kinds]) | (capturable & ~fits)
            res_rank = np.cumsum(resolved) - resolved
            pend_rank = np.cumsum(pend) - pend
            for i, e in enumerate(lanes):
                kind, lo, hi = kinds[i]
                if resolved[i]:
                    d = dir_base + int(res_rank[i])
                    status = CAPTURED if fits[i] else kind
                    directory[d] = entry(e, lo, int(first[i]) * cols if fits[i] else 0, int(rows[i]) if fits[i] else 0, s, status)
                    first_packed[d] = first[i]
                    sm[("captured", "empty", "lost")[status]] += 1
                if pend[i] and pend_base + int(pend_rank[i]) < pcap:
                    pending_new[s, pend_base + int(pend_rank[i])] = e
            if fits.any():
                last = int(np.flatnonzero(fits)[-1])
                packed_rows = max(packed_rows, int(first[last] + rows[last]))
            row_base += int(rows.sum())
            dir_base += int(resolved.sum())
            pend_base += int(pend.sum())
        kept = min(pend_base, pcap)
        pending[s, :kept] = pending_new[s, :kept]
        pending_count[s] = kept
        sm["pending"] += kept
        sm["pending_dropped"] += pend_base - kept
    sm["resolved"] = dir_base
    sm["arena_floats"] = packed_rows * cols
    # ---- snap_copy_kernel: wave w takes packed rows w, w + waves, ...
    arena = np.full(arena_floats, np.nan, np.float32)
    for w in range(waves):
        for p in range(w, packed_rows, waves):
            lo, hi = 0, dir_base
            while lo < hi:
                mid = (lo + hi) >> 1
                if first_packed[mid] <= p:
                    lo = mid + 1
                else:
                    hi = mid
            assert lo > 0
            en = directory[lo - 1]
            k = p - int(first_packed[lo - 1])
            assert en["status"] == CAPTURED and k < en["rows"], (p, lo - 1, en)
            at = int(en["offset"]) + k * cols
            assert at + cols <= arena_floats
            arena[at:at + cols] = ring[(int(en["first_row"]) + k) % ring_rows, :cols]
    return directory[:dir_base].copy(), arena, sm


def random_case(rng):
    """arguments of one call: events around the head row, so that every outcome turns up"""
    slots = int(rng.integers(1, 9))
    mask = int(rng.integers(1, 1 << slots)) | (1 << (slots - 1))
    capacity, pcap = int(rng.integers(0, 41)), int(rng.integers(0, 9))
    ring_rows, cols = int(rng.integers(1, 65)), int(rng.integers(1, 71))
    stride = cols + int(rng.integers(0, 4))
    head = int(rng.integers(0, 200))
    ring = np.zeros((ring_rows, stride), np.float32)
    for r in range(max(0, head - ring_rows), head):
        ring[r % ring_rows] = r * 1000 + np.arange(stride)
    snapshot_rows = rng.integers(1, 30, slots).astype(np.int32)

    def some(n):
        e = np.zeros(n, EVENT_DTYPE)
        e["start_row"] = head - rng.integers(-10, ring_rows + 25, n)
        e["length"] = rng.integers(-2, 40, n)
        e["fire_row"] = e["start_row"] + e["length"]
        e["peak"] = rng.integers(0, 400, n)
        e["noise"] = rng.random(n)
        e["magnitude"] = rng.random(n)
        return e
    events = np.stack([some(capacity) for _ in range(slots)]) if capacity else None
    summary = None
    if capacity or rng.integers(2):
        summary = np.zeros(slots, np.dtype([("events", np.int64), ("detect_rows", np.int64), ("marginal_rows", np.int64)]))
        summary["events"] = rng.integers(0, capacity + 4, slots)
    pending = np.stack([some(pcap) for _ in range(slots)]) if pcap else np.zeros((slots, 0), EVENT_DTYPE)
    count = rng.integers(0, pcap + 1, slots).astype(np.int64)
    arena_floats = int(rng.choice([0, 1, cols * 5, cols * 40 + 3, cols * 4000]))
    return dict(events=events, summary=summary, slot_mask=mask, snapshot_rows=snapshot_rows, ring=ring, cols=cols,
                head_row=head, pending=pending, pending_count=count, arena_floats=arena_floats)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main(cases=200):
    rng = np.random.default_rng(20)
    seen = np.zeros(5, np.int64)
    for case in range(cases):
        args = random_case(rng)
        a = dict(args, pending=args["pending"].copy(), pending_count=args["pending_count"].copy())
        b = dict(args, pending=args["pending"].copy(), pending_count=args["pending_count"].copy())
        d1, arena1, s1 = snapshots(**a)
        d2, arena2, s2 = snapshots_plan(tile=int(rng.choice([3, 5, 64])), waves=int(rng.choice([1, 7])), **b)
        ok = (same(d1, d2) and same(arena1, arena2) and s1 == s2 and same(a["pending"], b["pending"]) and
              same(a["pending_count"], b["pending_count"]))
        if not ok:
            print("case %d: the plan and the rules disagree\n%s\n%s\n%s\n%s" % (case, s1, s2, d1, d2))
            return 1
        seen += (int(s1["captured"]), int(s1["empty"]), int(s1["lost"]), int(s1["pending"]), int(s1["pending_dropped"]))
    if not seen.all():
        print("the cases leave an outcome out: captured, empty, lost, pending, dropped = %s" % seen.tolist())
        return 1
    print("ok: %d cases; captured %d, empty %d, lost %d, pending %d, dropped %d" % ((cases,) + tuple(seen.tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 200))
