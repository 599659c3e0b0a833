"""What tests/test_periodic_cpu.py and tests/test_gpu_periodic.py share (test infrastructure): synthetic rings whose floats
name their (row, column), so that a wrong float names itself; one call's arguments as a Case; ro_periodic_plan through ctypes
with guard bytes behind the directory and the summary; ro_periodic_units_host with guard bytes behind the units; the numpy
emulator (tools/periodic/emu_periodic.py) on the same Case; and the decision table, written against a `call` so that the
host twin (against the emulator) and the device (against the host twin) walk the very same lines."""
import ctypes as C
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5                                              # every guard byte
NGUARD = 3                                                # guard entries behind the directory; 3 x 64 bytes behind the units
WRITTEN, LOST, NO_ROOM = 0, 1, 2
BLOCK = 2880
PAD = -1.0                                                # floats [cols, stride) of a slot, and slots no row has reached
COLS_STEP = 2048                                          # ring float (row, col) is (row - row_base) * 2048 + col + 0.5


def load_emu():
    spec = importlib.util.spec_from_file_location("emu_periodic", os.path.join(ROOT, "tools", "periodic", "emu_periodic.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    return emu


EMU = load_emu()


def blocks_of(naxis1, rows):
    return -(-4 * naxis1 * rows // BLOCK)


def ring_at(head_row, ring_rows, cols, stride=None, row_base=0):
    """the ring after rows [0, head_row): slot s holds the last row r < head_row with r % ring_rows == s"""
    stride = cols if stride is None else stride
    ring = np.full((ring_rows, stride), PAD, np.float32)
    for r in range(max(head_row - ring_rows, 0), head_row):
        ring[r % ring_rows, :cols] = (r - row_base) * COLS_STEP + np.arange(cols) + 0.5
    assert (head_row - row_base) * COLS_STEP < 1 << 24 and cols <= COLS_STEP
    return ring


class Case:
    """the arguments of one plan and its units.  recorders: [(snapshot_rows, first_col, cols), ...]"""

    def __init__(self, recorders, head_row, ring_rows, cols, units_bytes, final=False, next_index=None, capacity=64, stride=None,
                 ring=None, row_base=0):
        self.recorders = [tuple(int(x) for x in r) for r in recorders]
        self.head_row, self.final, self.ring_rows, self.cols = head_row, final, ring_rows, cols
        self.units_bytes, self.capacity = units_bytes, capacity
        self.next_index = np.zeros(len(recorders), np.int64) if next_index is None else np.array(next_index, np.int64)
        self.ring = ring_at(head_row, ring_rows, cols, stride, row_base) if ring is None else np.ascontiguousarray(ring, np.float32)
        self.row_base = row_base
        assert self.ring.shape[0] == ring_rows and self.ring.shape[1] >= cols

    def but(self, **kw):
        other = Case.__new__(Case)
        other.__dict__.update(self.__dict__)
        other.next_index = self.next_index.copy()
        other.__dict__.update(kw)
        return other

    def recorder_array(self, ro):
        return ro.periodic_recorders(self.recorders)

    def ring_struct(self, ro, address=None):
        return ro.capi.RowRing(self.ring.ctypes.data if address is None else address, self.ring.shape[1], self.ring_rows,
                               self.cols, 0)


def guarded(nbytes, guard_bytes):
    return np.full(nbytes + guard_bytes, GUARD, np.uint8)


def plan_call(ro, case):
    """ro_periodic_plan through ctypes, guards behind the directory and the summary.  Returns (directory, summary, the new
    next_index); the case's own next_index stays"""
    recs = case.recorder_array(ro)
    nxt = np.concatenate([case.next_index, np.full(NGUARD, 0x5a5a5a5a5a5a5a5a, np.int64)])
    d, sm = guarded(case.capacity * 56, NGUARD * 56), guarded(64, NGUARD * 64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    lib = ro.library()
    rc = lib.ro_periodic_plan(p(recs), len(recs), p(nxt), case.head_row, int(case.final), case.ring_rows, case.cols,
                              case.units_bytes, p(d) if case.capacity else None, case.capacity, p(sm))
    assert rc == 0, lib.ro_last_error()
    summary = sm[:64].view(ro.capi.PERIODIC_SUMMARY_DTYPE)[0]
    n = int(summary["entries"])
    assert 0 <= n <= case.capacity and np.all(d[n * 56:] == GUARD) and np.all(sm[64:] == GUARD)
    assert np.all(nxt[len(recs):] == 0x5a5a5a5a5a5a5a5a)
    return d[:n * 56].view(ro.capi.PERIODIC_ENTRY_DTYPE).copy(), summary.copy(), nxt[:len(recs)].copy()


class Result:
    """what a plan and its units leave: the directory, the summary, the new next_index, and the units with their guards"""

    def __init__(self, case, directory, summary, next_index, units_bytes):
        self.dir, self.summary, self.next_index, self.raw = directory, summary, next_index, units_bytes
        s, st = summary, directory["status"]
        used = int(s["units_bytes"])
        assert used % BLOCK == 0 and used <= case.units_bytes and int(s["reserved"]) == 0
        assert [int(s[k]) for k in ("written", "lost", "no_room")] == [int((st == k).sum()) for k in range(3)]
        sizes = [blocks_of(int(e["naxis1"]), int(e["rows"])) for e in directory if e["status"] != LOST]
        written = int(s["written"])
        assert int(s["needed_bytes"]) == BLOCK * sum(sizes) and used == BLOCK * sum(sizes[:written])
        assert directory["offset"][st == WRITTEN].tolist() == [BLOCK * sum(sizes[:i]) for i in range(written)]
        assert not directory["offset"][st != WRITTEN].any() and not directory["bytes"][st == LOST].any()
        self.units = units_bytes[:used]
        assert np.all(units_bytes[used:] == GUARD), "bytes of the units behind the last written unit were touched"

    def unit(self, d):
        e = self.dir[d]
        assert e["status"] == WRITTEN, e
        return self.units[int(e["offset"]):int(e["offset"]) + BLOCK * blocks_of(int(e["naxis1"]), int(e["rows"]))]

    def shape(self):
        """[(recorder, index, first_row, rows, due_row, status), ...]"""
        return [tuple(int(e[k]) for k in ("recorder", "index", "first_row", "rows", "due_row", "status")) for e in self.dir]


def host_units(ro, case, directory):
    """ro_periodic_units_host through ctypes with guards behind the units; the ring must come back unchanged"""
    units = guarded(case.units_bytes, NGUARD * 64)
    ring = case.ring.copy()
    recs = case.recorder_array(ro)
    p = lambda a: C.c_void_p(a.ctypes.data)
    lib = ro.library()
    desc = case.ring_struct(ro, ring.ctypes.data)
    rc = lib.ro_periodic_units_host(C.byref(desc), p(recs), len(recs), p(directory) if len(directory) else None, len(directory),
                                    p(units) if case.units_bytes else None, case.units_bytes)
    assert rc == 0, lib.ro_last_error()
    assert ring.tobytes() == case.ring.tobytes(), "the ring was written"
    return units


def host_call(ro, case):
    directory, summary, nxt = plan_call(ro, case)
    return Result(case, directory, summary, nxt, host_units(ro, case, directory))


def emu_check(case, got):
    """the emulator's replay and rules on the same case against a Result"""
    nxt = [int(x) for x in case.next_index]
    d, sm = EMU.plan(case.recorders, nxt, case.head_row, case.final, case.ring_rows, case.units_bytes, case.capacity)
    assert got.summary.tobytes() == sm.tobytes(), (got.summary, sm)
    assert got.dir.tobytes() == d.tobytes(), (got.dir, d)
    assert got.next_index.tolist() == nxt
    assert got.units.tobytes() == EMU.units(case.ring, case.cols, case.recorders, d, case.units_bytes).tobytes()


def host_vs_emu(ro):
    def call(case):
        got = host_call(ro, case)
        emu_check(case, got)
        return got
    return call


def statuses(result):
    return result.dir["status"].tolist()


def cut_bytes(case, e):
    """the unit of directory entry e from the closed form of ring_at"""
    _, first_col, naxis1 = case.recorders[int(e["recorder"])]
    rows = int(e["first_row"]) - case.row_base + np.arange(int(e["rows"]), dtype=np.int64)
    data = (rows[:, None] * COLS_STEP + first_col + np.arange(naxis1)[None, :] + 0.5).astype(">f4").tobytes()
    return data + bytes(-len(data) % BLOCK)


def check_cuts(case, result):
    for i, e in enumerate(result.dir):
        if e["status"] == WRITTEN:
            assert result.unit(i).tobytes() == cut_bytes(case, e), (i, e)


# ---- the decision table: one case per function, each asserted by status and by bytes ------------------------------------
def case_rooms(ro, call):
    """exactly needed_bytes; one block less; not a multiple of 2880; none at all, the units NULL.  The first entry that does
    not fit and every writable one behind it, of any recorder, are NO_ROOM with their shape and offset 0; next_index stays in
    front of them, and a second call with needed_bytes from there writes the rest"""
    recorders = [(7, 1, 200), (5, 0, 33), (11, 100, 150)]   # blocks of a unit: 2, 1, 3
    case = Case(recorders, 25, 40, 256, 0, stride=259)      # due: 3, 4, 2 snapshots -> 6 + 4 + 6 blocks
    need = 16 * BLOCK
    full = call(case.but(units_bytes=need))
    assert statuses(full) == [WRITTEN] * 9 and full.next_index.tolist() == [3, 4, 2]
    assert int(full.summary["needed_bytes"]) == int(full.summary["units_bytes"]) == need
    check_cuts(case, full)
    for room, written in ((need - 1, 8), (need - BLOCK, 8), (need - 3 * BLOCK - 1, 7), (7 * BLOCK + 17, 4), (6 * BLOCK, 3),
                          (2 * BLOCK, 1), (BLOCK, 0), (0, 0)):
        r = call(case.but(units_bytes=room))
        assert statuses(r) == [WRITTEN] * written + [NO_ROOM] * (9 - written), (room, statuses(r))
        assert int(r.summary["needed_bytes"]) == need and r.dir["rows"].tolist() == [7] * 3 + [5] * 4 + [11] * 2
        assert r.units.tobytes() == full.units[:len(r.units)].tobytes()
        want_next = [min(written, 3), min(max(written - 3, 0), 4), max(written - 7, 0)]
        assert r.next_index.tolist() == want_next, (room, r.next_index)
        rest = call(case.but(next_index=r.next_index, units_bytes=int(r.summary["needed_bytes"])))
        assert statuses(rest) == [WRITTEN] * (9 - written) and rest.next_index.tolist() == [3, 4, 2]
        assert rest.shape() == [x[:5] + (WRITTEN,) for x in full.shape()[written:]]
        check_cuts(case, rest)
    # the prefix rule: room for recorder 1's one-block units, but recorder 0's second unit does not fit in front of them
    r = call(case.but(units_bytes=3 * BLOCK))
    assert statuses(r) == [WRITTEN] + [NO_ROOM] * 8


def case_lost_and_captured(ro, call):
    """a snapshot is due at row (k + 1) S + 1, with H = (k + 1) S + 2: a ring of S + 1 rows has lost its first row by then, a
    ring of S + 2 holds it.  LOST resolves: next_index passes it, nothing is written, bytes 0"""
    S = 7
    for k in (0, 3):
        H = (k + 1) * S + 2
        lost = call(Case([(S, 2, 9)], H, S + 1, 12, 4 * BLOCK, next_index=[k]))
        assert lost.shape() == [(0, k, k * S, S, H - 1, LOST)] and lost.next_index.tolist() == [k + 1] and len(lost.units) == 0
        case = Case([(S, 2, 9)], H, S + 2, 12, 4 * BLOCK, next_index=[k])
        held = call(case)
        assert held.shape() == [(0, k, k * S, S, H - 1, WRITTEN)] and held.next_index.tolist() == [k + 1]
        check_cuts(case, held)
        assert call(case.but(head_row=H - 1)).shape() == []          # a row earlier it is not due
    # a late call: the older snapshots are lost, the younger ones held -- LOST entries lead a recorder's list
    case = Case([(S, 0, 12), (3, 4, 5)], 40, 20, 12, 64 * BLOCK)
    r = call(case)
    assert [x[5] for x in r.shape()] == [LOST] * 3 + [WRITTEN] * 2 + [LOST] * 7 + [WRITTEN] * 5
    assert r.next_index.tolist() == [5, 12]
    check_cuts(case, r)


def case_capacity(ro, call):
    """`capacity` below the due count: the candidates beyond it are not listed and not advanced, the summary counts them, and
    the next call lists them"""
    case = Case([(2, 0, 4), (3, 1, 2)], 14, 16, 4, 64 * BLOCK)     # due: 6 and 4
    r = call(case.but(capacity=7))
    assert [x[:2] for x in r.shape()] == [(0, k) for k in range(6)] + [(1, 0)]
    assert int(r.summary["unlisted"]) == 3 and r.next_index.tolist() == [6, 1]
    rest = call(case.but(next_index=r.next_index))
    assert [x[:2] for x in rest.shape()] == [(1, 1), (1, 2), (1, 3)] and int(rest.summary["unlisted"]) == 0
    none = call(case.but(capacity=0))
    assert none.shape() == [] and int(none.summary["unlisted"]) == 10 and none.next_index.tolist() == [0, 0]
    check_cuts(case, r)
    check_cuts(case, rest)


def case_final(ro, call):
    """stop(): one more snapshot, [k' S, min((k' + 1) S, H)) for the first k' that is not due, due_row H - 1 -- with one row,
    with S rows (the row behind them is dropped, as the reference drops it), and none without rows; answered once"""
    S = 5
    for H, want in ((0, []), (1, [(0, 0, 0, 1, 0, WRITTEN)]), (5, [(0, 0, 0, 5, 4, WRITTEN)]), (6, [(0, 0, 0, 5, 5, WRITTEN)]),
                    (7, [(0, 0, 0, 5, 6, WRITTEN), (0, 1, 5, 2, 6, WRITTEN)]),
                    (11, [(0, 0, 0, 5, 6, WRITTEN), (0, 1, 5, 5, 10, WRITTEN)]),
                    (13, [(0, 0, 0, 5, 6, WRITTEN), (0, 1, 5, 5, 11, WRITTEN), (0, 2, 10, 3, 12, WRITTEN)])):
        case = Case([(S, 1, 3)], H, 16, 5, 8 * BLOCK, final=True)
        r = call(case)
        assert r.shape() == want, (H, r.shape())
        check_cuts(case, r)
        again = call(case.but(next_index=r.next_index))
        assert again.shape() == [], (H, again.shape())
    # a final one that finds no room comes back
    case = Case([(S, 1, 3)], 8, 16, 5, BLOCK, final=True)
    r = call(case)
    assert statuses(r) == [WRITTEN, NO_ROOM] and r.next_index.tolist() == [1] and r.dir["rows"].tolist() == [5, 3]
    rest = call(case.but(next_index=r.next_index))
    assert rest.shape() == [(0, 1, 5, 3, 7, WRITTEN)]
    check_cuts(case, rest)


def case_wrap(ro, call):
    """snapshots that straddle the ring's last slot, in rings of S + 2, 2 S + 3 and 23 rows"""
    S = 9
    for ring_rows in (S + 2, 2 * S + 3, 23):
        for k in range(6):
            H = (k + 1) * S + 2
            case = Case([(S, 3, 70)], H, ring_rows, 77, 4 * BLOCK, next_index=[k], stride=80)
            r = call(case)
            assert r.shape() == [(0, k, k * S, S, H - 1, WRITTEN)], (ring_rows, k)
            check_cuts(case, r)
    straddles = [(ring_rows, k) for ring_rows in (S + 2, 2 * S + 3, 23) for k in range(6)
                 if (k * S) % ring_rows + S > ring_rows]
    assert len(straddles) >= 6


def case_eight(ro, call):
    """eight recorders in one plan: different S, overlapping windows, one whose next_index is ahead of its due snapshots and
    one in the middle of them"""
    recorders = [(1 + s, 3 * s, 40 - 4 * s) for s in range(8)]
    case = Case(recorders, 30, 32, 64, 64 * BLOCK, next_index=[20, 0, 50, 3, 0, 0, 1, 0], stride=67)
    r = call(case)
    per = [[x[1] for x in r.shape() if x[0] == s] for s in range(8)]
    assert per == [list(range(20, 28)), list(range(0, 14)), [], list(range(3, 7)), list(range(0, 5)), list(range(0, 4)),
                   list(range(1, 4)), list(range(0, 3))]
    assert statuses(r) == [WRITTEN] * len(r.dir) and r.next_index.tolist() == [28, 14, 50, 7, 5, 4, 4, 3]
    check_cuts(case, r)


def case_bits(ro, call):
    """a bit copy: NaN payloads, -0, denormals and infinities come out with their bytes reversed and nothing else changed"""
    bits = np.array([0x7fc12345, 0xffa00001, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000,
                     0x3f800000, 0x01020304, 0xdeadbeef, 0x00800000], np.uint32)
    ring = bits.view(np.float32).reshape(4, 3)
    r = call(Case([(2, 1, 2)], 4, 4, 3, BLOCK, ring=ring))
    want = bits.reshape(4, 3)[0:2, 1:3].reshape(-1).byteswap().tobytes()
    assert statuses(r) == [WRITTEN] and r.unit(0).tobytes() == want + bytes(BLOCK - len(want))


TABLE = [case_rooms, case_lost_and_captured, case_capacity, case_final, case_wrap, case_eight, case_bits]


def case_from_emu(args):
    """emu_periodic.random_case's arguments as a Case"""
    return Case(args["recorders"], args["head_row"], args["ring"].shape[0], args["cols"], args["units_bytes"], final=args["final"],
                next_index=args["next_index"], capacity=args["capacity"], ring=args["ring"])


def unit_refusals(d):
    """(changed arguments, word the text must hold) of the two unit calls; d: "d_" for the resident call's argument names.
    The refusal tests' case: recorders [(4, 1, 6), (3, 0, 2)] on a ring of 10 columns and 12 rows, H = 11: entries (0, 0), (0, 1),
    (1, 0), (1, 1), (1, 2), all WRITTEN, one block each"""
    return [(dict(ring=None), "null ring"), (dict(ring_rows_ptr=None), "null d_rows"), (dict(recorders=None), "null recorders"),
            (dict(dir=None), "null dir"), (dict(ring_fields=dict(ring_rows=0)), "ring_rows"),
            (dict(ring_fields=dict(stride=9)), "stride"), (dict(ring_fields=dict(reserved=1)), "reserved"),
            (dict(count=0), "count"), (dict(count=9), "count"),
            (dict(recs={0: (0, 1, 6)}), "recorders[0]: snapshot_rows"), (dict(recs={1: (3, -1, 2)}), "recorders[1]: window"),
            (dict(recs={1: (3, 0, 0)}), "recorders[1]: window"), (dict(recs={0: (4, 5, 6)}), "recorders[0]: window"),
            (dict(units=None), "null %sunits" % d), (dict(units_bytes=-1), "units_bytes"), (dict(entries=-1), "entries"),
            (dict(units="ring"), "overlaps"), (dict(units="ring end"), "overlaps"),
            (dict(entry={0: dict(recorder=2)}), "dir[0]: recorder"), (dict(entry={4: dict(recorder=0)}), "dir[4]: recorder"),
            (dict(entry={1: dict(index=2, first_row=8)}), "dir[1]: index"), (dict(entry={1: dict(first_row=5)}), "dir[1]: index"),
            (dict(entry={0: dict(rows=3, bytes=72)}), "dir[1]: rows"), (dict(entry={1: dict(rows=5, bytes=120)}), "dir[1]: rows"),
            (dict(entry={1: dict(rows=0, bytes=0)}), "dir[1]: rows"), (dict(entry={4: dict(status=3)}), "dir[4]: status"),
            (dict(entry={3: dict(naxis1=3)}), "dir[3]: naxis1"), (dict(entry={3: dict(bytes=20)}), "dir[3]: naxis1"),
            (dict(entry={2: dict(offset=3 * BLOCK)}), "dir[2]: offset"), (dict(entry={2: dict(offset=2 * BLOCK + 4)}), "dir[2]: offset"),
            (dict(entry={1: dict(status=NO_ROOM, offset=0)}), "dir[2]: offset"),
            (dict(entry={3: dict(status=LOST, offset=0, bytes=0), 4: dict(offset=3 * BLOCK)}), "dir[4]: a recorder's WRITTEN"),
            (dict(entry={4: dict(status=LOST, bytes=0)}), "dir[4]: offset"),
            (dict(units_bytes=4 * BLOCK), "dir[4]: offset"), (dict(ring_fields=dict(ring_rows=3)), "dir[0]: rows")]
