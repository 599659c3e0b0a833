"""What tests/test_raw_cpu.py and tests/test_gpu_raw.py share (test infrastructure): synthetic samples -- stream sample s is
(s, -s - 0.5) in F32 and F64 and (s % 30011 - 15000, -(s % 29989)) in I16, so that a wrong sample names itself, and where
a later span owns a sample the earlier spans hold 7777 instead, so that a read from the wrong span names itself too; one
call's arguments as a Case; the raw ro_raw_host call with guard entries behind every output; the numpy emulator
(tools/raw/emu_raw.py) on the same Case; and the decision table of the raw capture's rules, written against a `call` so
that the host twin (against the emulator) and the device (against the host twin) walk the very same lines."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5                                              # every byte of a guard entry
NGUARD = 3                                                # guard entries (floats: 3 x 13) behind every output
CAPTURED, EMPTY, LOST = 0, 1, 2
F32, I16, F64 = 0, 1, 2


def load_emu():
    spec = importlib.util.spec_from_file_location("emu_raw", os.path.join(ROOT, "tools", "raw", "emu_raw.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    return emu


EMU = load_emu()


def header_constant(name):
    """an integer #define of csrc/ro_raw.h"""
    text = open(os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_raw.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)\b" % name, text).group(1))


def f_of(shape, start):
    return EMU.first_sample(start, shape[0], shape[1])


def L_of(shape, length):
    return EMU.raw_length(length, EMU.int_rate(*shape), shape[2])


def expected_run(layout, f, L):
    """the float32 pairs of stream samples [f, f + L), each in the format of the LAST span of the layout that holds it; from
    the closed form, not from the spans' arrays"""
    out = np.zeros((L, 2), np.float32)
    s = f
    while s < f + L:
        i = max(j for j, (first, count, _) in enumerate(layout) if first <= s < first + count)
        end = min(f + L, layout[i + 1][0] if i + 1 < len(layout) else layout[i][0] + layout[i][1])
        out[s - f:end - f] = EMU.samples_of(s, end - s, layout[i][2]).astype(np.float32)
        s = end
    return out.reshape(-1)


_serial = [0]


def snaps_of(ro, items):
    """[(start_row, length) or (start_row, length, status), ...] -> SNAPSHOT_DTYPE entries as the snapshots call writes them
    for a ring that held every row: first_row = max(start, 0), rows = what is left of `length`; the peak numbers them"""
    out = np.zeros(len(items), ro.capi.SNAPSHOT_DTYPE)
    for i, item in enumerate(items):
        start, length = item[0], item[1]
        status = item[2] if len(item) > 2 else CAPTURED
        _serial[0] += 1
        lo = max(start, 0)
        out[i]["event"] = (start + length + 3, start, length + 2, 1.5, _serial[0], 3.0 + _serial[0], 0)
        out[i]["first_row"], out[i]["rows"] = lo, max(length - (lo - start), 0) if status == CAPTURED else 0
        out[i]["offset"], out[i]["slot"], out[i]["status"] = 1000 + i, _serial[0] % 8, status
    return out


class Case:
    """the arguments of one call; pending / pending_count are the list BEFORE the call (every voice gets a copy)"""

    def __init__(self, ro, shape, items, layout, arena_floats, pending=None, pcap=4, dcap=None, resolved=None):
        self.shape = shape
        self.directory = items if isinstance(items, np.ndarray) else snaps_of(ro, items)
        self.dcap = len(self.directory) if dcap is None else dcap
        self.snap_summary = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
        self.snap_summary["resolved"] = len(self.directory) if resolved is None else resolved
        self.layout = list(layout)
        self.spans = EMU.spans_of(self.layout)
        self.arena_floats, self.pcap = arena_floats, pcap
        self.pending = np.zeros(pcap, ro.capi.SNAPSHOT_DTYPE)
        self.pending_count = np.zeros(1, np.int64)
        if pending is not None:
            p = pending if isinstance(pending, np.ndarray) else snaps_of(ro, pending)
            self.pending[:len(p)] = p
            self.pending_count[0] = len(p)

    def carry(self, result):
        """the list a call left behind becomes this call's"""
        self.pending, self.pending_count = result.pending.copy(), result.pending_count.copy()
        return self

    @property
    def dir_entries(self):
        return self.pcap + self.dcap

    @property
    def head(self):
        return self.layout[-1][0] + self.layout[-1][1]


class Result:
    """everything a call writes, guards included, as bytes; and the parts in use, typed"""

    def __init__(self, ro, case, dir_bytes, arena_bytes, pending_bytes, count_bytes, summary_bytes):
        self.raw = (dir_bytes, arena_bytes, pending_bytes, count_bytes, summary_bytes)
        self.summary = summary_bytes[:64].view(ro.capi.RAW_SUMMARY_DTYPE)[0]
        n, used = int(self.summary["resolved"]), int(self.summary["arena_floats"])
        assert 0 <= n <= case.dir_entries and 0 <= used <= case.arena_floats and int(self.summary["reserved"]) == 0, self.summary
        self.dir = dir_bytes[:n * 72].view(ro.capi.RAW_CAPTURE_DTYPE)
        self.arena = arena_bytes[:used * 4].view(np.float32)
        self.pending = pending_bytes[:case.pcap * 72].view(ro.capi.SNAPSHOT_DTYPE)
        self.pending_count = count_bytes[:8].view(np.int64)
        assert np.all(dir_bytes[n * 72:] == GUARD), "directory entries past `resolved` were touched"
        assert np.all(arena_bytes[used * 4:] == GUARD), "arena floats past the ones in use were touched"
        assert np.all(pending_bytes[case.pcap * 72:] == GUARD) and np.all(count_bytes[8:] == GUARD)
        assert np.all(summary_bytes[64:] == GUARD)
        kept = int(self.pending_count[0])
        assert 0 <= kept <= case.pcap and kept == int(self.summary["pending"])
        assert self.pending[kept:].tobytes() == case.pending[kept:].tobytes(), "pending entries past the new count moved"
        sizes = [int(e["samples"]) for e in self.dir if e["status"] == CAPTURED]
        assert [int(e["offset"]) for e in self.dir if e["status"] == CAPTURED] == [2 * sum(sizes[:i]) for i in range(len(sizes))]
        assert used == 2 * sum(sizes) and all(int(e["samples"]) == 0 and int(e["offset"]) == 0 for e in self.dir
                                              if e["status"] != CAPTURED)

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw))

    def run(self, i):
        e = self.dir[i]
        return self.arena[int(e["offset"]):int(e["offset"]) + 2 * int(e["samples"])]

    def by_peak(self, entry):
        hit = np.flatnonzero(self.dir["event"]["peak"] == entry["event"]["peak"])
        return self.dir[int(hit[0])] if hit.size else None


def guarded(entries, itemsize):
    return np.full((entries + NGUARD) * itemsize, GUARD, np.uint8)


def outputs_for(case):
    """(raw_dir, arena, pending, count, summary) byte arrays with the case's list in and guards behind"""
    d_dir = guarded(case.dir_entries, 72)
    d_arena = guarded(case.arena_floats + 13 * NGUARD, 4)
    d_pending = guarded(case.pcap, 72)
    d_pending[:case.pcap * 72] = case.pending.view(np.uint8).reshape(-1)
    d_count = guarded(1, 8)
    d_count[:8] = case.pending_count.view(np.uint8)
    d_summary = guarded(1, 64)
    return d_dir, d_arena, d_pending, d_count, d_summary


def span_structs(ro, case, addresses):
    arr = (ro.capi.IqSpan * 4)()
    for i, ((a, first, fmt), address) in enumerate(zip(case.spans, addresses)):
        arr[i] = ro.capi.IqSpan(address, first, len(a), fmt, 0)
    return arr


def host_call(ro, case):
    """ro_raw_host through ctypes; the samples and the directory must come back unchanged"""
    outs = outputs_for(case)
    arrays = [a.copy() for a, _, _ in case.spans]
    directory, snap_summary = case.directory.copy(), case.snap_summary.copy()
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = ro.library().ro_raw_host(*case.shape, p(directory) if case.dcap else None, case.dcap, p(snap_summary),
                                  span_structs(ro, case, [a.ctypes.data for a in arrays]), len(arrays),
                                  p(outs[2]) if case.pcap else None, p(outs[3]), case.pcap, p(outs[0]),
                                  p(outs[1]) if case.arena_floats else None, case.arena_floats, p(outs[4]))
    assert rc == 0, ro.library().ro_last_error()
    assert all(a.tobytes() == b.tobytes() for a, (b, _, _) in zip(arrays, case.spans)), "the samples were written"
    assert directory.tobytes() == case.directory.tobytes() and snap_summary.tobytes() == case.snap_summary.tobytes()
    return Result(ro, case, *outs)


def emu_check(ro, case, got):
    """the emulator's rules on the same case against a Result"""
    pending = case.pending.copy().view(EMU.SNAPSHOT_DTYPE)
    count = case.pending_count.copy()
    d, arena, sm = EMU.raw(*case.shape, case.directory[:case.dcap].view(EMU.SNAPSHOT_DTYPE), int(case.snap_summary["resolved"][0]),
                           case.spans, pending, count, case.arena_floats)
    assert got.summary.tobytes() == sm.tobytes(), (got.summary, sm)
    assert got.dir.tobytes() == d.tobytes(), (got.dir, d)
    used = int(sm["arena_floats"])
    assert not np.isnan(arena[:used]).any() and got.arena.tobytes() == arena[:used].tobytes()
    assert np.array_equal(got.pending_count, count)
    assert got.pending[:count[0]].tobytes() == pending[:count[0]].tobytes()


def host_vs_emu(ro):
    def call(case):
        got = host_call(ro, case)
        emu_check(ro, case, got)
        return got
    return call


def statuses(result):
    return result.dir["status"].tolist()


def captured_ok(case, result, i, start, length):
    """entry i is the captured run of a snapshot (start, length): f, L and every float from the closed form"""
    e = result.dir[i]
    f, L = f_of(case.shape, start), L_of(case.shape, length)
    assert (int(e["status"]), int(e["first_sample"]), int(e["samples"])) == (CAPTURED, f, L), (e, f, L)
    assert result.run(i).tobytes() == expected_run(case.layout, f, L).tobytes(), (i, result.run(i)[:8])


# ---- the decision table: one case per function, each asserted by status and by bytes ------------------------------------
S = (256, 240, 1000)      # hop 16, R = (int)62.5 = 62: L(10) = 161, one more than 10 hops; f(20) = 321
Z = (256, 0, 4000)        # no overlap: hop 256, R = 15: L(10) = 2666; f(20) = 19 * 256 + 1


def case_head_edge(ro, call):
    """f + L == head_sample captured; one sample fewer and it is still pending"""
    assert (f_of(S, 20), L_of(S, 10), f_of(Z, 20), L_of(Z, 10)) == (321, 161, 4865, 2666)
    for shape, fmt in ((S, F32), (Z, I16)):
        end = f_of(shape, 20) + L_of(shape, 10)
        case = Case(ro, shape, [(20, 10)], [(300, end - 300, fmt)], 6000)
        r = call(case)
        assert statuses(r) == [CAPTURED] and int(r.summary["pending"]) == 0
        captured_ok(case, r, 0, 20, 10)
        case = Case(ro, shape, [(20, 10)], [(300, end - 301, fmt)], 6000)
        r = call(case)
        assert statuses(r) == [] and r.pending_count[0] == 1 and r.pending[0].tobytes() == case.directory[0].tobytes()
        assert int(r.summary["arena_floats"]) == 0


def case_empty(ro, call):
    """L == 0 is EMPTY, also where its first sample has left the spans; still pending while f lies beyond the head"""
    case = Case(ro, S, [(20, 0), (10, 0), (40, 0)], [(300, 200, F32)], 4000)
    r = call(case)
    assert statuses(r) == [EMPTY, EMPTY] and r.dir["first_sample"].tolist() == [321, 161] and r.pending_count[0] == 1
    assert (int(r.summary["empty"]), int(r.summary["lost"]), int(r.summary["arena_floats"])) == (2, 0, 0)


def case_base_edge(ro, call):
    """f == base_sample captured; a base one sample later and it is LOST: nothing is written"""
    case = Case(ro, S, [(20, 10)], [(321, 400, F64)], 4000)
    captured_ok(case, call(case), 0, 20, 10)
    case = Case(ro, S, [(20, 10)], [(322, 400, F64)], 4000)
    r = call(case)
    assert statuses(r) == [LOST] and int(r.dir[0]["first_sample"]) == 321 and int(r.summary["lost"]) == 1


def case_first_sample(ro, call):
    """f for start in {-3, 0, 1, 2, 57} with and without overlap; the image of start -3 was clipped at row 0 (rows 4 of a
    length 7), the raw run is the whole length's"""
    for shape, want in ((S, [0, 0, 17, 33, 913]), (Z, [0, 0, 1, 257, 14337])):
        hop = shape[0] - shape[1]
        starts = [-3, 0, 1, 2, 57]
        assert [f_of(shape, s) for s in starts] == want == [0 if s < 1 else (s - (shape[1] == 0)) * hop + 1 for s in starts]
        case = Case(ro, shape, [(s, 7) for s in starts], [(0, want[-1] + L_of(shape, 7) + 10, F32)], 100000)
        assert case.directory["rows"].tolist() == [4, 7, 7, 7, 7] and case.directory["first_row"].tolist() == [0, 0, 1, 2, 57]
        r = call(case)
        assert statuses(r) == [CAPTURED] * 5 and r.dir["first_sample"].tolist() == want
        for i, s in enumerate(starts):
            captured_ok(case, r, i, s, 7)


def arena_case(ro, arena_floats):
    # L(4) = 64, L(5) = 80, L(6) = 96; (2, 4) is LOST at base 100, (9, 0) EMPTY
    return Case(ro, S, [(10, 4), (12, 5), (2, 4), (14, 6), (9, 0), (16, 4)], [(100, 500, F32)], arena_floats, pcap=6)


def case_arena_exact(ro, call):
    """an arena that fits exactly"""
    assert [L_of(S, n) for n in (4, 5, 6)] == [64, 80, 96]
    case = arena_case(ro, 2 * (64 + 80 + 96 + 64))
    r = call(case)
    assert statuses(r) == [CAPTURED, CAPTURED, LOST, CAPTURED, EMPTY, CAPTURED] and int(r.summary["pending"]) == 0
    assert r.dir["offset"].tolist() == [0, 128, 0, 288, 0, 480] and int(r.summary["arena_floats"]) == 608
    for i, (s, n) in ((0, (10, 4)), (1, (12, 5)), (3, (14, 6)), (5, (16, 4))):
        captured_ok(case, r, i, s, n)


def case_arena_short(ro, call):
    """one float short at the first, a middle and the last candidate: that one and every capturable one behind it stay
    pending, EMPTY and LOST behind it resolve; the next call, with room, takes them in order ahead of its own"""
    for floats, want, kept in ((127, [LOST, EMPTY], [0, 1, 3, 5]), (479, [CAPTURED, CAPTURED, LOST, EMPTY], [3, 5]),
                               (607, [CAPTURED, CAPTURED, LOST, CAPTURED, EMPTY], [5])):
        case = arena_case(ro, floats)
        r = call(case)
        assert statuses(r) == want and r.pending_count[0] == len(kept), (floats, statuses(r))
        assert r.pending[:len(kept)].tobytes() == case.directory[kept].tobytes()
        nxt = Case(ro, S, [(18, 4)], [(100, 500, F32)], 4000, pcap=6).carry(r)
        r2 = call(nxt)
        assert statuses(r2) == [CAPTURED] * (len(kept) + 1) and r2.pending_count[0] == 0
        assert r2.dir["event"]["peak"].tolist() == case.directory[kept]["event"]["peak"].tolist() + [nxt.directory[0]["event"]["peak"]]
        for i, k in enumerate(kept):
            captured_ok(nxt, r2, i, int(case.directory[k]["event"]["start_row"]), int(case.directory[k]["rows"]))
    # (14, 6) does not fit and (16, 4) behind it would have: the prefix rule keeps it waiting
    r = call(arena_case(ro, 2 * (64 + 80) + 2 * 64))
    assert statuses(r) == [CAPTURED, CAPTURED, LOST, EMPTY] and r.pending_count[0] == 2


def case_three_calls(ro, call):
    """a run that waits for its samples over three calls, the spans sliding: pending, pending, captured -- ahead of the
    third call's own candidates; and one that waited too long is LOST"""
    first = Case(ro, S, [(30, 10), (20, 4), (33, 2)], [(300, 250, F32)], 4000)          # f 481 + 161 and 529 + 32
    r1 = call(first)
    assert statuses(r1) == [CAPTURED] and r1.pending_count[0] == 2
    second = Case(ro, S, [(31, 1)], [(400, 230, F32)], 4000).carry(r1)                    # head 630: 561 needed, 642 not yet
    r2 = call(second)
    assert [int(e["first_sample"]) for e in r2.dir] == [529, 497] and statuses(r2) == [CAPTURED] * 2 and r2.pending_count[0] == 1
    third = Case(ro, S, [(34, 1)], [(470, 180, F32), (600, 100, I16)], 4000).carry(r2)    # head 700
    r3 = call(third)
    assert statuses(r3) == [CAPTURED, CAPTURED] and r3.dir["first_sample"].tolist() == [481, 545] and r3.pending_count[0] == 0
    captured_ok(third, r3, 0, 30, 10)                                                     # straddles the two formats
    late = Case(ro, S, [], [(482, 300, F32)], 4000).carry(r2)
    r4 = call(late)
    assert statuses(r4) == [LOST] and r4.pending_count[0] == 0


def case_pending_overflow(ro, call):
    """a pending list that overflows: pending_dropped counts the rest"""
    case = Case(ro, S, [(35, 10), (36, 10), (20, 5), (37, 10), (38, 10)], [(300, 300, F32)], 4000, pending=[(33, 10)], pcap=3)
    r = call(case)
    assert statuses(r) == [CAPTURED] and int(r.summary["pending"]) == 3 and int(r.summary["pending_dropped"]) == 2
    assert r.pending[0].tobytes() == case.pending[0].tobytes()                            # the old entry first
    assert r.pending[1:3].tobytes() == case.directory[0:2].tobytes()


def case_counts_out_of_range(ro, call):
    """a pending count and a `resolved` outside their ranges read as the nearer bound"""
    pend = [(20, 4), (21, 4), (22, 4)]
    for count, resolved, want in ((-3, -1, 0), (99, 99, 5), (2, 1, 3)):
        case = Case(ro, S, [(23, 4), (24, 4)], [(300, 300, F32)], 4000, pending=pend, pcap=3, resolved=resolved)
        case.pending_count[0] = count
        r = call(case)
        assert statuses(r) == [CAPTURED] * want and r.pending_count[0] == 0, (count, resolved, statuses(r))


def case_skipped_entries(ro, call):
    """EMPTY and LOST directory entries have no image and get no raw run: skipped, not resolved, not pending"""
    case = Case(ro, S, [(20, 4, EMPTY), (21, 4), (22, 4, LOST), (50, 4, LOST), (23, 4)], [(300, 300, F32)], 4000)
    r = call(case)
    assert statuses(r) == [CAPTURED] * 2 and int(r.summary["resolved"]) == 2 and r.pending_count[0] == 0
    assert r.dir["event"]["peak"].tolist() == case.directory[[1, 4]]["event"]["peak"].tolist()


def case_dir_capacity(ro, call):
    """dir_capacity below `resolved`: only dir_capacity entries are read"""
    case = Case(ro, S, [(20, 4), (21, 4), (22, 4), (23, 4)], [(300, 300, F32)], 4000, dcap=2)
    r = call(case)
    assert statuses(r) == [CAPTURED] * 2 and r.dir["first_sample"].tolist() == [321, 337]


def case_flush_only(ro, call):
    """dir_capacity 0: a call that only flushes the pending list; and one with no room for anything"""
    case = Case(ro, S, [], [(300, 300, F32)], 4000, pending=[(20, 4), (40, 4)], dcap=0)
    r = call(case)
    assert statuses(r) == [CAPTURED] and r.pending_count[0] == 1
    r = call(Case(ro, S, [], [(300, 300, F32)], 0, pcap=0, dcap=0))
    assert r.summary.tobytes() == bytes(64)
    r = call(Case(ro, S, [(20, 4)], [(300, 300, F32)], 0, pcap=0))
    assert statuses(r) == [] and int(r.summary["pending_dropped"]) == 1


def case_spans(ro, call):
    """one to four spans, overlapping, in mixed formats; runs inside one span, across two and across three; a sample that
    several spans hold comes from the last one (the earlier ones hold 7777 there)"""
    layouts = [[(300, 700, F64)],
               [(300, 300, F32), (560, 440, I16)],
               [(300, 200, I16), (480, 150, F64), (600, 400, F32)],
               [(300, 120, F32), (400, 140, I16), (520, 100, F64), (619, 381, F32)]]
    for layout in layouts:
        # f 321 + 161 = 482, f 481 + 161 = 642, f 401 + 323 = 724 (across three of three and of four), f 833 + 161 = 994
        items = [(20, 10), (30, 10), (25, 20), (52, 10)]
        assert L_of(S, 20) == 322 and f_of(S, 25) == 401
        case = Case(ro, S, items, layout, 10000)
        r = call(case)
        assert statuses(r) == [CAPTURED] * 4
        for i, (s, n) in enumerate(items):
            captured_ok(case, r, i, s, n)
        assert not np.any(r.arena == 7777)


TABLE = [case_head_edge, case_empty, case_base_edge, case_first_sample, case_arena_exact, case_arena_short, case_three_calls,
         case_pending_overflow, case_counts_out_of_range, case_skipped_entries, case_dir_capacity, case_flush_only, case_spans]


def refusals(ro, d):
    """(changed arguments, word the text must hold); d: "d_" for the resident call's argument names"""
    one = lambda **kw: dict(spans=[dict(kw)])

    def two(second, first=(300, 200)):
        return dict(spans=[dict(first_sample=first[0], samples=first[1]), dict(first_sample=second[0], samples=second[1])])
    return [(dict(snap_summary=None), "null %ssnap_summary" % d), (dict(spans=None), "null spans"),
            (dict(count=None), "null %spending_count" % d), (dict(raw_dir=None), "null %sraw_dir" % d),
            (dict(out=None), "null %sraw_summary" % d), (dict(dir=None), "null %sdir" % d),
            (dict(pending=None), "null %spending with" % d), (dict(arena=None), "null %sarena" % d),
            (dict(dcap=-1), "dir_capacity"), (dict(pcap=-1), "pending_capacity"), (dict(arena_floats=-1), "arena_floats"),
            (dict(span_count=0), "span_count"), (dict(span_count=5), "span_count"),
            (one(d_iq=None), "spans[0]: null d_iq"), (one(first_sample=-1), "first_sample"), (one(samples=0), "samples"),
            (one(format=3), "format"), (one(format=-1), "format"), (one(reserved=1), "reserved"),
            (two((300, 250)), "spans[1] is out of order"), (two((250, 300)), "spans[1] is out of order"),
            (two((320, 180)), "spans[1] is out of order"), (two((320, 100)), "spans[1] is out of order"),
            (two((501, 100)), "spans[1] leaves a gap"),
            (dict(dcap=(1 << 24) + 1), "candidates"), (dict(dcap=1 << 23, pcap=(1 << 23) + 1), "candidates")]


def apply_refusal(ro, base_spans, kw):
    """the spans of a refusal: `spans` is None, or a list of field changes on top of copies of base_spans[0]"""
    kw = dict(kw)
    if "spans" in kw and kw["spans"] is not None:
        arr = (ro.capi.IqSpan * 4)()
        for i, change in enumerate(kw["spans"]):
            b = base_spans[0]
            fields = dict(d_iq=b.d_iq, first_sample=b.first_sample, samples=b.samples, format=b.format, reserved=b.reserved)
            fields.update(change)
            arr[i] = ro.capi.IqSpan(fields["d_iq"], fields["first_sample"], fields["samples"], fields["format"], fields["reserved"])
        kw.setdefault("span_count", len(kw["spans"]))
        kw["spans"] = arr
    return kw


def case_from_emu(ro, args):
    """emu_raw.random_case's arguments as a Case"""
    case = Case.__new__(Case)
    case.shape = (args["bins"], args["overlap"], args["sample_rate"])
    case.directory = np.ascontiguousarray(args["directory"]).view(ro.capi.SNAPSHOT_DTYPE)
    case.dcap = len(case.directory)
    case.snap_summary = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
    case.snap_summary["resolved"] = args["resolved"]
    case.spans = args["spans"]
    case.layout = [(first, len(a), fmt) for a, first, fmt in case.spans]
    case.arena_floats = args["arena_floats"]
    case.pending = np.ascontiguousarray(args["pending"]).view(ro.capi.SNAPSHOT_DTYPE)
    case.pcap = len(case.pending)
    case.pending_count = args["pending_count"].copy()
    return case
