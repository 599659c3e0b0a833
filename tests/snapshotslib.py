"""What tests/test_snapshots_cpu.py and tests/test_gpu_snapshots.py share (test infrastructure): a synthetic ring whose slot
of stream row r holds r * 1000 + column, so that a wrong row or column names itself; synthetic events; one call's
arguments as a Case; the raw ro_snapshots_host call with guard entries behind every output; the numpy emulator
(tools/snapshots/emu_snapshots.py) on the same Case; and the decision table of the snapshot rules, written against a
`call` so that the host twin (against the emulator) and the device (against the host twin) walk the very same lines."""
import ctypes as C
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5                                              # every byte of a guard entry
NGUARD = 3                                                # guard entries (floats: 3 x 16) behind every output
PAD = np.float32(-7.0)                                    # floats [cols, stride) of a ring slot
CAPTURED, EMPTY, LOST = 0, 1, 2


def load_emu():
    spec = importlib.util.spec_from_file_location("emu_snapshots", os.path.join(ROOT, "tools", "snapshots", "emu_snapshots.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    return emu


def header_constant(name):
    """an integer #define of csrc/ro_snapshots.h"""
    import re
    text = open(os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_snapshots.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)\b" % name, text).group(1))


def row_values(r, cols):
    return (r * 1000 + np.arange(cols)).astype(np.float32)


def ring_for(ring_rows, cols, stride, head_row):
    """the ring after rows [0, head_row) have been put: slot r % ring_rows holds row r's r * 1000 + column"""
    ring = np.full((ring_rows, stride), PAD, np.float32)
    ring[:, :cols] = -1.0
    for r in range(max(0, head_row - ring_rows), head_row):
        ring[r % ring_rows, :cols] = row_values(r, cols)
    return ring


def image_of(lo, rows, cols):
    """what a captured snapshot of rows [lo, lo + rows) holds"""
    return np.concatenate([row_values(lo + k, cols) for k in range(rows)]) if rows else np.zeros(0, np.float32)


_serial = [0]


def events_of(ro, spans):
    """[(start_row, length), ...] -> EVENT_DTYPE; the peak numbers the events, so that each is recognisable"""
    out = np.zeros(len(spans), ro.capi.EVENT_DTYPE)
    for i, (start, length) in enumerate(spans):
        _serial[0] += 1
        out[i] = (start + length + 3, start, length, 1.5, _serial[0], 3.0 + _serial[0], 0)
    return out


class Case:
    """the arguments of one call; pending / pending_count are the lists BEFORE the call (every voice gets a copy)"""

    def __init__(self, ro, slot_events, snapshot_rows, ring_rows, cols, head_row, arena_floats, pending=None, pcap=4,
                 capacity=None, fired=None, mask=None, stride=None, with_summary=True):
        slots = 1 + max(list(slot_events) + list(pending or {}) + [(mask or 1).bit_length() - 1])
        self.mask = mask if mask is not None else sum(1 << s for s in set(slot_events) | set(pending or {}))
        self.slots = slots
        self.capacity = max([len(v) for v in slot_events.values()] + [0]) if capacity is None else capacity
        self.events = np.zeros((slots, self.capacity), ro.capi.EVENT_DTYPE)
        self.summary = np.zeros(slots, ro.capi.DETECT_SUMMARY_DTYPE) if with_summary else None
        for s, spans in slot_events.items():
            ev = spans if isinstance(spans, np.ndarray) else events_of(ro, spans)
            n = min(len(ev), self.capacity)
            self.events[s, :n] = ev[:n]
            if with_summary:
                self.summary["events"][s] = len(ev) if fired is None or s not in fired else fired[s]
        self.snapshot_rows = np.full(slots, snapshot_rows, np.int32) if np.isscalar(snapshot_rows) else \
            np.asarray(snapshot_rows, np.int32)
        self.cols, self.stride = cols, cols + 3 if stride is None else stride
        self.ring = ring_for(ring_rows, cols, self.stride, head_row)
        self.head_row, self.arena_floats, self.pcap = head_row, arena_floats, pcap
        self.pending = np.zeros((slots, pcap), ro.capi.EVENT_DTYPE)
        self.pending_count = np.zeros(slots, np.int64)
        for s, spans in (pending or {}).items():
            ev = spans if isinstance(spans, np.ndarray) else events_of(ro, spans)
            self.pending[s, :len(ev)] = ev
            self.pending_count[s] = len(ev)

    def carry(self, result):
        """the lists a call left behind become this call's"""
        self.pending, self.pending_count = result.pending.copy(), result.pending_count.copy()
        return self

    @property
    def dir_entries(self):
        return self.slots * (self.capacity + self.pcap)


class Result:
    """everything a call writes, guards included, as bytes; and the parts in use, typed"""

    def __init__(self, ro, case, dir_bytes, arena_bytes, pending_bytes, count_bytes, summary_bytes):
        self.raw = (dir_bytes, arena_bytes, pending_bytes, count_bytes, summary_bytes)
        self.summary = summary_bytes[:64].view(ro.capi.SNAP_SUMMARY_DTYPE)[0]
        n, used = int(self.summary["resolved"]), int(self.summary["arena_floats"])
        assert 0 <= n <= case.dir_entries and 0 <= used <= case.arena_floats, self.summary
        self.dir = dir_bytes[:n * 72].view(ro.capi.SNAPSHOT_DTYPE)
        self.arena = arena_bytes[:used * 4].view(np.float32)
        self.pending = pending_bytes[:case.slots * case.pcap * 40].view(ro.capi.EVENT_DTYPE).reshape(case.slots, case.pcap)
        self.pending_count = count_bytes[:case.slots * 8].view(np.int64)
        assert np.all(dir_bytes[n * 72:] == GUARD), "directory entries past `resolved` were touched"
        assert np.all(arena_bytes[used * 4:] == GUARD), "arena floats past the ones in use were touched"
        assert np.all(pending_bytes[case.slots * case.pcap * 40:] == GUARD) and np.all(count_bytes[case.slots * 8:] == GUARD)
        assert np.all(summary_bytes[64:] == GUARD)

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw))

    def image(self, i, cols):
        e = self.dir[i]
        return self.arena[int(e["offset"]):int(e["offset"]) + int(e["rows"]) * cols]

    def by_peak(self, event):
        """the directory entry of one event (its peak numbers it), or None"""
        hit = np.flatnonzero(self.dir["event"]["peak"] == event["peak"])
        return self.dir[int(hit[0])] if hit.size else None


def guarded(entries, itemsize):
    return np.full((entries + NGUARD) * itemsize, GUARD, np.uint8)


def outputs_for(case):
    """(dir, arena, pending, count, summary) byte arrays with the case's lists in and guards behind"""
    d_dir = guarded(case.dir_entries, 72)
    d_arena = guarded(case.arena_floats + 13 * NGUARD, 4)
    d_pending = guarded(case.slots * case.pcap, 40)
    d_pending[:case.slots * case.pcap * 40] = case.pending.view(np.uint8).reshape(-1)
    d_count = guarded(case.slots, 8)
    d_count[:case.slots * 8] = case.pending_count.view(np.uint8)
    d_summary = guarded(1, 64)
    return d_dir, d_arena, d_pending, d_count, d_summary


def ring_desc(ro, case, address):
    return ro.capi.RowRing(address, case.stride, case.ring.shape[0], case.cols, 0)


def host_call(ro, case):
    """ro_snapshots_host through ctypes; the ring must come back unchanged"""
    outs = outputs_for(case)
    ring = case.ring.copy()
    events, summary = case.events.copy(), None if case.summary is None else case.summary.copy()
    p = lambda a: C.c_void_p(a.ctypes.data)
    desc = ring_desc(ro, case, ring.ctypes.data)
    rows = (C.c_int32 * case.slots)(*case.snapshot_rows.tolist())
    rc = ro.library().ro_snapshots_host(p(events) if case.capacity else None, case.capacity,
                                        p(summary) if summary is not None else None, case.mask, rows, C.byref(desc),
                                        case.head_row, p(outs[2]) if case.pcap else None, p(outs[3]), case.pcap, p(outs[0]),
                                        p(outs[1]) if case.arena_floats else None, case.arena_floats, p(outs[4]))
    assert rc == 0, ro.library().ro_last_error()
    assert ring.tobytes() == case.ring.tobytes() and events.tobytes() == case.events.tobytes()
    return Result(ro, case, *outs)


def emu_check(ro, emu, case, got):
    """the emulator's rules on the same case against a Result"""
    pending = case.pending.copy().view(emu.EVENT_DTYPE)
    count = case.pending_count.copy()
    events = case.events.view(emu.EVENT_DTYPE) if case.capacity else None
    d, arena, sm = emu.snapshots(events, case.summary, case.mask, case.snapshot_rows, case.ring, case.cols, case.head_row,
                                 pending, count, case.arena_floats)
    assert got.summary.tobytes() == sm.tobytes(), (got.summary, sm)
    assert got.dir.tobytes() == d.tobytes(), (got.dir, d)
    used = int(sm["arena_floats"])
    assert not np.isnan(arena[:used]).any() and got.arena.tobytes() == arena[:used].tobytes()
    assert np.array_equal(got.pending_count, count)
    for s in range(case.slots):
        if (case.mask >> s) & 1:
            assert got.pending[s, :count[s]].tobytes() == pending[s, :count[s]].tobytes(), s
            assert got.pending[s, count[s]:].tobytes() == case.pending[s, count[s]:].tobytes(), "entries past the count moved"
        else:
            assert got.pending[s].tobytes() == case.pending[s].tobytes() and count[s] == case.pending_count[s]


def host_vs_emu(ro, emu):
    def call(case):
        got = host_call(ro, case)
        emu_check(ro, emu, case, got)
        return got
    return call


def statuses(result):
    return result.dir["status"].tolist()


# ---- the decision table: one case per function, each asserted by status and by bytes ------------------------------------
R, COLS, SNAP = 16, 5, 10                                 # ring rows, columns, snapshot_rows of the table


def captured_ok(result, i, lo, rows, cols=COLS):
    e = result.dir[i]
    assert (int(e["status"]), int(e["first_row"]), int(e["rows"])) == (CAPTURED, lo, rows), e
    assert np.array_equal(result.image(i, cols), image_of(lo, rows, cols)), (i, result.image(i, cols))


def case_head_edge(ro, call):
    """hi == head_row captured; hi == head_row + 1 pending"""
    case = Case(ro, {0: [(30, 10), (31, 10)]}, SNAP, R, COLS, 40, 1000)
    r = call(case)
    assert statuses(r) == [CAPTURED] and int(r.summary["pending"]) == 1 and r.pending_count[0] == 1
    captured_ok(r, 0, 30, 10)
    assert r.pending[0, 0].tobytes() == case.events[0, 1].tobytes() and int(r.summary["arena_floats"]) == 50


def case_ring_edge(ro, call):
    """lo == head_row - ring_rows captured; one row earlier LOST"""
    r = call(Case(ro, {0: [(24, 6), (23, 6)]}, SNAP, R, COLS, 40, 1000))
    assert statuses(r) == [CAPTURED, LOST]
    captured_ok(r, 0, 24, 6)
    assert (int(r.dir[1]["first_row"]), int(r.dir[1]["rows"]), int(r.dir[1]["offset"])) == (23, 0, 0)
    assert (int(r.summary["captured"]), int(r.summary["lost"]), int(r.summary["arena_floats"])) == (1, 1, 30)


def case_negative_start(ro, call):
    """a negative start_row with hi > 0 is captured from row 0; with hi <= 0 it is EMPTY"""
    r = call(Case(ro, {0: [(-3, 7), (-5, 5), (-9, 4), (2, 0), (3, -2)]}, SNAP, R, COLS, 8, 1000))
    assert statuses(r) == [CAPTURED, EMPTY, EMPTY, EMPTY, EMPTY] and int(r.summary["empty"]) == 4
    captured_ok(r, 0, 0, 4)
    assert r.dir["first_row"].tolist() == [0, 0, 0, 2, 3] and int(r.summary["arena_floats"]) == 20


def case_length_clamp(ro, call):
    """length > snapshot_rows keeps the first snapshot_rows rows (per slot)"""
    r = call(Case(ro, {0: [(28, 25)], 1: [(28, 25)]}, [SNAP, 3], R, COLS, 40, 1000))
    assert statuses(r) == [CAPTURED, CAPTURED] and r.dir["slot"].tolist() == [0, 1]
    captured_ok(r, 0, 28, 10)
    captured_ok(r, 1, 28, 3)
    assert int(r.dir[1]["offset"]) == 50


def case_wrap(ro, call):
    """a snapshot that wraps the ring's end: rows 29 ... 34 live in slots 13, 14, 15, 0, 1, 2"""
    r = call(Case(ro, {0: [(29, 6)]}, SNAP, R, COLS, 40, 1000))
    assert statuses(r) == [CAPTURED]
    captured_ok(r, 0, 29, 6)


def arena_case(ro, arena_floats):
    return Case(ro, {0: [(26, 4), (30, 4), (-4, 2), (34, 4)], 1: [(10, 3), (35, 2), (25, 20)]}, SNAP, R, COLS, 40, arena_floats)


def case_arena_exact(ro, call):
    """an arena that fits exactly"""
    r = call(arena_case(ro, 70))
    assert statuses(r) == [CAPTURED, CAPTURED, EMPTY, CAPTURED, LOST, CAPTURED] and int(r.summary["pending"]) == 1
    assert r.dir["offset"].tolist() == [0, 20, 0, 40, 0, 60] and int(r.summary["arena_floats"]) == 70
    for i, (lo, n) in ((0, (26, 4)), (1, (30, 4)), (3, (34, 4)), (5, (35, 2))):
        captured_ok(r, i, lo, n)


def case_arena_short(ro, call):
    """one float short: that candidate and every capturable one behind it stay pending, EMPTY and LOST behind it resolve"""
    case = arena_case(ro, 59)
    r = call(case)
    assert statuses(r) == [CAPTURED, CAPTURED, EMPTY, LOST] and r.dir["slot"].tolist() == [0, 0, 0, 1]
    assert int(r.summary["arena_floats"]) == 40 and r.pending_count.tolist() == [1, 2]
    assert r.pending[0, 0].tobytes() == case.events[0, 3].tobytes()
    assert r.pending[1, :2].tobytes() == case.events[1, 1:3].tobytes()          # (35, 2) would have fitted by itself
    # the next call, with room, takes them in order ahead of its own events
    nxt = Case(ro, {0: [(36, 3)], 1: []}, SNAP, R, COLS, 45, 1000, mask=3).carry(r)
    r2 = call(nxt)
    # (row 25 has left the ring by head 45: the candidate that waited for room is LOST)
    assert statuses(r2) == [CAPTURED, CAPTURED, CAPTURED, LOST] and r2.dir["slot"].tolist() == [0, 0, 1, 1]
    assert r2.dir["event"]["peak"].tolist() == [case.events[0, 3]["peak"], nxt.events[0, 0]["peak"], case.events[1, 1]["peak"],
                                                case.events[1, 2]["peak"]]
    captured_ok(r2, 0, 34, 4)
    captured_ok(r2, 1, 36, 3)
    captured_ok(r2, 2, 35, 2)


def case_pending_overflow(ro, call):
    """a pending list that overflows: pending_dropped counts the rest"""
    case = Case(ro, {0: [(35, 10), (36, 10), (30, 5), (37, 10), (38, 10)]}, SNAP, R, COLS, 40, 1000,
                pending={0: [(33, 10)]}, pcap=3)
    r = call(case)
    assert statuses(r) == [CAPTURED] and int(r.summary["pending"]) == 3 and int(r.summary["pending_dropped"]) == 2
    assert r.pending[0, 0].tobytes() == case.pending[0, 0].tobytes()            # the old entry first
    assert r.pending[0, 1:3].tobytes() == case.events[0, 0:2].tobytes()


def case_unlisted(ro, call):
    """summary.events > capacity: only `capacity` events are read, `unlisted` counts the rest"""
    r = call(Case(ro, {0: [(30, 2), (31, 2), (32, 2), (33, 2), (34, 2)], 1: [(30, 1)]}, SNAP, R, COLS, 40, 1000, capacity=3,
                  fired={0: 7, 1: 1}))
    assert statuses(r) == [CAPTURED] * 4 and r.dir["first_row"].tolist() == [30, 31, 32, 30]
    assert int(r.summary["unlisted"]) == 4 and int(r.summary["resolved"]) == 4


def case_zero_events(ro, call):
    """zero events give a zero summary"""
    r = call(Case(ro, {0: [], 2: []}, SNAP, R, COLS, 40, 1000, capacity=4))
    assert r.summary.tobytes() == bytes(64) and r.dir.size == 0 and r.arena.size == 0
    r = call(Case(ro, {0: []}, SNAP, R, COLS, 0, 0, capacity=0, pcap=0, with_summary=False))
    assert r.summary.tobytes() == bytes(64)


def case_two_calls(ro, call):
    """the first call's pending candidates resolve in the second, ahead of the second call's own events, in order"""
    first = Case(ro, {0: [(35, 10), (28, 4), (38, 4)], 1: [(39, 2)]}, SNAP, R, COLS, 40, 1000)
    r1 = call(first)
    assert statuses(r1) == [CAPTURED] and r1.pending_count.tolist() == [2, 1]
    second = Case(ro, {0: [(41, 5), (47, 9)], 1: [(44, 1)]}, SNAP, R, COLS, 50, 1000).carry(r1)
    r2 = call(second)
    assert statuses(r2) == [CAPTURED] * 5 and r2.dir["slot"].tolist() == [0, 0, 0, 1, 1]
    assert r2.dir["first_row"].tolist() == [35, 38, 41, 39, 44] and r2.pending_count.tolist() == [1, 0]
    for i, (lo, n) in enumerate(((35, 10), (38, 4), (41, 5), (39, 2), (44, 1))):
        captured_ok(r2, i, lo, n)
    assert r2.pending[0, 0].tobytes() == second.events[0, 1].tobytes()


def case_lost_after_waiting(ro, call):
    """a candidate that waited too long: pending at head 40, LOST at head 60 (its first row left the ring)"""
    r1 = call(Case(ro, {0: [(35, 10)]}, SNAP, R, COLS, 40, 1000))
    assert r1.dir.size == 0 and r1.pending_count[0] == 1
    r2 = call(Case(ro, {0: []}, SNAP, R, COLS, 60, 1000, capacity=0, with_summary=False).carry(r1))
    assert statuses(r2) == [LOST] and r2.pending_count[0] == 0 and int(r2.summary["lost"]) == 1


TABLE = [case_head_edge, case_ring_edge, case_negative_start, case_length_clamp, case_wrap, case_arena_exact, case_arena_short,
         case_pending_overflow, case_unlisted, case_zero_events, case_two_calls, case_lost_after_waiting]


def case_from_emu(ro, args):
    """emu_snapshots.random_case's arguments as a Case"""
    case = Case.__new__(Case)
    case.mask = args["slot_mask"]
    case.slots = case.mask.bit_length()
    case.events = (np.zeros((case.slots, 0), ro.capi.EVENT_DTYPE) if args["events"] is None
                   else np.ascontiguousarray(args["events"]).view(ro.capi.EVENT_DTYPE))
    case.capacity = case.events.shape[1]
    case.summary = None if args["summary"] is None else args["summary"].view(ro.capi.DETECT_SUMMARY_DTYPE)
    case.snapshot_rows = args["snapshot_rows"]
    case.ring, case.cols, case.stride = args["ring"], args["cols"], args["ring"].shape[1]
    case.head_row, case.arena_floats = args["head_row"], args["arena_floats"]
    case.pending = np.ascontiguousarray(args["pending"]).view(ro.capi.EVENT_DTYPE)
    case.pcap = case.pending.shape[1]
    case.pending_count = args["pending_count"]
    return case
