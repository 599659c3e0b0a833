"""What tests/test_units_cpu.py and tests/test_gpu_units.py share (test infrastructure): synthetic arenas -- arena float i is
i + 0.5, so that a wrong float names itself; one call's arguments as a Case (images or raw); the raw ro_snapshot_units_host /
ro_raw_units_host call with guard bytes behind every output; the numpy emulator (tools/units/emu_units.py) on the same Case;
and the decision table of the units' rules, written against a `call` so that the host twins (against the emulator) and the
device (against the host twins) walk the very same lines."""
import ctypes as C
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5                                              # every guard byte
NGUARD = 3                                                # guard entries behind the directory; 3 x 64 bytes behind the units
CAPTURED, EMPTY, LOST = 0, 1, 2
WRITTEN, SKIPPED, NO_ROOM, INVALID = 0, 1, 2, 3
BLOCK = 2880
SLOTS = 8


def load_emu():
    spec = importlib.util.spec_from_file_location("emu_units", os.path.join(ROOT, "tools", "units", "emu_units.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    return emu


EMU = load_emu()


def ramp(floats):
    return np.arange(floats, dtype=np.float32) + np.float32(0.5)


def blocks_of(naxis1, naxis2):
    return -(-4 * naxis1 * naxis2 // BLOCK)


def whole(cols):
    """every slot's window is the whole image row"""
    return [(0, cols)] * SLOTS


class Case:
    """the arguments of one call.  kind "image": directory is SNAPSHOT_DTYPE, with cols and windows (eight (first_col, cols));
    kind "raw": RAW_CAPTURE_DTYPE"""

    def __init__(self, ro, kind, directory, arena, units_bytes, cols=None, windows=None, resolved=None, dcap=None):
        self.kind = kind
        self.directory = directory
        self.dcap = len(directory) if dcap is None else dcap
        self.summary = np.zeros(1, ro.capi.RAW_SUMMARY_DTYPE if kind == "raw" else ro.capi.SNAP_SUMMARY_DTYPE)
        self.summary["resolved"] = len(directory) if resolved is None else resolved
        self.arena = np.ascontiguousarray(arena, np.float32) if not isinstance(arena, int) else ramp(arena)
        self.units_bytes = units_bytes
        self.cols, self.windows = cols, None if windows is None else list(windows)
        assert (kind == "raw") == (windows is None)

    def with_room(self, units_bytes):
        other = Case.__new__(Case)
        other.__dict__.update(self.__dict__)
        other.units_bytes = units_bytes
        return other

    def window_structs(self, ro):
        arr = (ro.capi.BandWindow * SLOTS)()
        for i, (first, cols) in enumerate(self.windows):
            arr[i] = ro.capi.BandWindow(first, cols)
        return arr


def images(ro, items, cols, pad=0):
    """[(rows, slot) or (rows, slot, status), ...] -> (SNAPSHOT_DTYPE entries packed as the snapshots call packs them, the
    arena's floats + pad); the peak numbers them"""
    d = np.zeros(len(items), ro.capi.SNAPSHOT_DTYPE)
    offset = 0
    for i, item in enumerate(items):
        status = item[2] if len(item) > 2 else CAPTURED
        d[i]["event"]["peak"] = i
        d[i]["slot"], d[i]["status"] = item[1], status
        if status == CAPTURED:
            d[i]["rows"], d[i]["offset"] = item[0], offset
            offset += item[0] * cols
    return d, offset + pad


def runs(ro, items, pad=0, gap=0):
    """[samples or (samples, status), ...] -> (RAW_CAPTURE_DTYPE entries packed as the raw call packs them, behind `gap`
    floats, the arena's floats + pad)"""
    d = np.zeros(len(items), ro.capi.RAW_CAPTURE_DTYPE)
    offset = gap
    for i, item in enumerate(items):
        samples, status = item if isinstance(item, tuple) else (item, CAPTURED)
        d[i]["event"]["peak"] = i
        d[i]["slot"], d[i]["status"] = i % SLOTS, status
        if status == CAPTURED:
            d[i]["samples"], d[i]["offset"] = samples, offset
            offset += 2 * samples
    return d, offset + pad


class Result:
    """everything a call writes, guards included, as bytes; and the parts in use, typed"""

    def __init__(self, ro, case, dir_bytes, units_bytes, summary_bytes):
        self.raw = (dir_bytes, units_bytes, summary_bytes)
        self.summary = summary_bytes[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
        s = self.summary
        n, used = int(s["entries"]), int(s["units_bytes"])
        assert 0 <= n <= case.dcap and 0 <= used <= case.units_bytes and used % BLOCK == 0 and int(s["reserved"]) == 0, s
        self.dir = dir_bytes[:n * 32].view(ro.capi.FITS_UNIT_DTYPE)
        self.units = units_bytes[:used]
        assert np.all(dir_bytes[n * 32:] == GUARD), "unit directory entries at or behind n were touched"
        assert np.all(units_bytes[used:] == GUARD), "bytes of the units past the ones in use were touched"
        assert np.all(summary_bytes[64:] == GUARD)
        st = self.dir["status"]
        assert [int(s[k]) for k in ("written", "skipped", "no_room", "invalid")] == [int((st == k).sum()) for k in range(4)]
        have = [(int(e["naxis1"]), int(e["naxis2"])) for e in self.dir if e["status"] in (WRITTEN, NO_ROOM)]
        sizes = [blocks_of(*x) for x in have]
        assert all(int(e["bytes"]) == 4 * a * b for e, (a, b) in zip(self.dir[(st == WRITTEN) | (st == NO_ROOM)], have))
        assert int(s["needed_bytes"]) == BLOCK * sum(sizes)
        written = int(s["written"])
        assert self.dir["offset"][st == WRITTEN].tolist() == [BLOCK * sum(sizes[:i]) for i in range(written)]
        assert used == BLOCK * sum(sizes[:written])
        for k in (SKIPPED, INVALID):
            assert self.dir[st == k].tobytes() == (bytes(28) + bytes([k, 0, 0, 0])) * int((st == k).sum())
        assert not self.dir["offset"][st == NO_ROOM].any()

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw))

    def unit(self, d):
        """the bytes of entry d's unit, padding included"""
        e = self.dir[d]
        assert e["status"] == WRITTEN, e
        return self.units[int(e["offset"]):int(e["offset"]) + BLOCK * blocks_of(int(e["naxis1"]), int(e["naxis2"]))]


def guarded(nbytes, guard_bytes):
    return np.full(nbytes + guard_bytes, GUARD, np.uint8)


def outputs_for(case):
    """(unit_dir, units, summary) byte arrays with guards behind"""
    return guarded(case.dcap * 32, NGUARD * 32), guarded(case.units_bytes, NGUARD * 64), guarded(64, NGUARD * 64)


def host_call(ro, case):
    """the host twin through ctypes; the sources must come back unchanged"""
    outs = outputs_for(case)
    directory, summary, arena = case.directory.copy(), case.summary.copy(), case.arena.copy()
    p = lambda a: C.c_void_p(a.ctypes.data)
    lib = ro.library()
    head = (p(directory) if case.dcap else None, case.dcap, p(summary), p(arena) if arena.size else None, arena.size)
    tail = (p(outs[0]), p(outs[1]) if case.units_bytes else None, case.units_bytes, p(outs[2]))
    if case.kind == "raw":
        rc = lib.ro_raw_units_host(*head, *tail)
    else:
        rc = lib.ro_snapshot_units_host(*head, case.cols, case.window_structs(ro), *tail)
    assert rc == 0, lib.ro_last_error()
    assert directory.tobytes() == case.directory.tobytes() and summary.tobytes() == case.summary.tobytes()
    assert arena.tobytes() == case.arena.tobytes(), "the arena was written"
    return Result(ro, case, *outs)


def emu_check(ro, case, got):
    """the emulator's rules on the same case against a Result"""
    view = EMU.RAW_CAPTURE_DTYPE if case.kind == "raw" else EMU.SNAPSHOT_DTYPE
    d, units, sm = EMU.units(case.directory[:case.dcap].view(view), int(case.summary["resolved"][0]), case.arena,
                             case.units_bytes, case.cols, case.windows)
    assert got.summary.tobytes() == sm.tobytes(), (got.summary, sm)
    assert got.dir.tobytes() == d.tobytes(), (got.dir, d)
    assert got.units.tobytes() == units.tobytes()


def host_vs_emu(ro):
    def call(case):
        got = host_call(ro, case)
        emu_check(ro, case, got)
        return got
    return call


def statuses(result):
    return result.dir["status"].tolist()


def cut_bytes(case, d):
    """the unit of directory entry d from the closed form: arena float i is i + 0.5"""
    e = case.directory[d]
    if case.kind == "raw":
        i = int(e["offset"]) + np.arange(2 * int(e["samples"]), dtype=np.int64)
    else:
        first, cols = case.windows[int(e["slot"])]
        i = (int(e["offset"]) + first + case.cols * np.arange(int(e["rows"]), dtype=np.int64)[:, None] +
             np.arange(cols, dtype=np.int64)[None, :]).reshape(-1)
    data = (i.astype(np.float32) + np.float32(0.5)).astype(">f4").tobytes()
    return data + bytes(-len(data) % BLOCK)


# ---- the decision table: one case per function, each asserted by status and by bytes ------------------------------------
def case_order_of_the_rules(ro, call):
    """1 not CAPTURED: SKIPPED, whatever else it holds; 2 INVALID, also for a slot whose window has no columns; 3 a window
    without columns: SKIPPED; 4 writable"""
    cols = 9
    d, floats = images(ro, [(3, 0), (2, 1, EMPTY), (4, 2, LOST), (2, 3), (5, 1), (1, 7)], cols)
    windows = [(1, 4), (0, 9), (2, 2), (0, 0), (0, 0), (0, 0), (0, 0), (8, 1)]
    d[1]["slot"], d[1]["rows"], d[1]["offset"] = 99, -4, -7             # not CAPTURED: nothing else is looked at
    bad = np.repeat(d[4:5], 5)                                           # slot 1, 5 rows
    bad["slot"][0], bad["slot"][1] = -1, 8
    bad["rows"][2] = 0
    bad["offset"][3] = -1
    bad["offset"][4] = floats - 5 * cols + 1                             # one float beyond the arena
    empty_window_but_invalid = d[3:4].copy()                             # slot 3 has no columns; rows < 1 comes first
    empty_window_but_invalid["rows"] = 0
    directory = np.concatenate([d, bad, empty_window_but_invalid])
    case = Case(ro, "image", directory, floats, 20 * BLOCK, cols, windows)
    r = call(case)
    assert statuses(r) == [WRITTEN, SKIPPED, SKIPPED, SKIPPED, WRITTEN, WRITTEN] + [INVALID] * 6
    assert r.dir["naxis1"].tolist()[:6] == [4, 0, 0, 0, 9, 1] and r.dir["naxis2"].tolist()[:6] == [3, 0, 0, 0, 5, 1]
    for i in (0, 4, 5):
        assert r.unit(i).tobytes() == cut_bytes(case, i), i
    # raw: the same three outcomes
    d, floats = runs(ro, [5, (7, LOST), 3, 4, 6, 2])
    d["samples"][2], d["offset"][3] = 0, -2
    d["offset"][4] = floats - 11                                         # 2 x 6 floats from there: one beyond
    case = Case(ro, "raw", d, floats, 20 * BLOCK)
    r = call(case)
    assert statuses(r) == [WRITTEN, SKIPPED, INVALID, INVALID, INVALID, WRITTEN] and r.dir["naxis1"].tolist() == [2, 0, 0, 0, 0, 2]
    assert r.unit(0).tobytes() == cut_bytes(case, 0) and r.unit(5).tobytes() == cut_bytes(case, 5)


def case_arena_edge(ro, call):
    """an entry that ends with the arena is writable; an arena one float shorter makes it INVALID, and nothing of it is read"""
    d, floats = images(ro, [(2, 0), (3, 1)], 7)
    for short, want in ((0, [WRITTEN, WRITTEN]), (1, [WRITTEN, INVALID])):
        case = Case(ro, "image", d, floats - short, 4 * BLOCK, 7, whole(7))
        assert statuses(call(case)) == want
    d, floats = runs(ro, [4, 9])
    for short, want in ((0, [WRITTEN, WRITTEN]), (1, [WRITTEN, INVALID])):
        assert statuses(call(Case(ro, "raw", d, floats - short, 4 * BLOCK))) == want
    # no arena at all: every captured entry is INVALID
    assert statuses(call(Case(ro, "raw", d, 0, 4 * BLOCK))) == [INVALID, INVALID]


def case_room(ro, call):
    """exactly the need; one block less; not a multiple of 2880; none at all.  The first entry that does not fit and every
    writable one behind it are NO_ROOM -- also a smaller one that would have fitted -- and carry their shape; SKIPPED and
    INVALID entries behind it stay what they are; a second call with needed_bytes writes all"""
    cols = 200
    d, floats = images(ro, [(3, 0), (8, 1), (4, 2, EMPTY), (1, 0), (9, 1), (1, 3), (2, 0)], cols)      # blocks 1, 3, -, 1, 3, -, 1
    d["rows"][5] = -1
    case = Case(ro, "image", d, floats, 0, cols, whole(cols))
    need = 9 * BLOCK
    full = call(case.with_room(need))
    assert statuses(full) == [WRITTEN, WRITTEN, SKIPPED, WRITTEN, WRITTEN, INVALID, WRITTEN]
    assert int(full.summary["needed_bytes"]) == int(full.summary["units_bytes"]) == need
    for room, written in ((need - 1, 4), (need - BLOCK, 4), (need - BLOCK - 1, 3), (5 * BLOCK + 17, 3), (4 * BLOCK, 2), (BLOCK, 1),
                          (BLOCK - 1, 0), (0, 0)):
        r = call(case.with_room(room))
        want = [WRITTEN if i < written else NO_ROOM for i in range(5)]
        assert statuses(r) == want[:2] + [SKIPPED] + want[2:4] + [INVALID] + want[4:], (room, statuses(r))
        assert int(r.summary["needed_bytes"]) == need and r.dir["naxis2"].tolist() == [3, 8, 0, 1, 9, 0, 2]
        assert r.units.tobytes() == full.units[:len(r.units)].tobytes()
        again = call(case.with_room(int(r.summary["needed_bytes"])))
        assert again.same_bytes(full)
    # the prefix rule: room for the first and the fourth entry's blocks, but the second does not fit
    r = call(case.with_room(2 * BLOCK))
    assert statuses(r)[:4] == [WRITTEN, NO_ROOM, SKIPPED, NO_ROOM]


def case_counts_out_of_range(ro, call):
    """`resolved` outside [0, dir_capacity] reads as the nearer bound; dir_capacity below it: only dir_capacity entries"""
    d, floats = runs(ro, [3, 4, 5, 6])
    for resolved, dcap, want in ((-3, 4, 0), (99, 4, 4), (2, 4, 2), (4, 3, 3), (0, 0, 0)):
        r = call(Case(ro, "raw", d[:dcap], floats, 8 * BLOCK, resolved=resolved))
        assert statuses(r) == [WRITTEN] * want, (resolved, dcap)
        if want == 0:
            assert r.summary.tobytes() == bytes(64)


def case_blocks(ro, call):
    """units that end just in front of, at and behind the block's end: the padding is zero, and a unit that ends with its
    block has none"""
    for naxis1, naxis2 in ((1, 719), (1, 720), (1, 721), (3, 240), (3, 241), (720, 2), (719, 1), (721, 1)):
        d, floats = images(ro, [(naxis2, 0), (naxis2, 1)], naxis1 + 2)
        case = Case(ro, "image", d, floats, 8 * BLOCK, naxis1 + 2, [(1, naxis1), (2, naxis1)] + [(0, 0)] * 6)
        r = call(case)
        assert statuses(r) == [WRITTEN, WRITTEN] and len(r.units) == 2 * BLOCK * blocks_of(naxis1, naxis2)
        assert r.unit(0).tobytes() == cut_bytes(case, 0) and r.unit(1).tobytes() == cut_bytes(case, 1), (naxis1, naxis2)
    for samples in (1, 359, 360, 361, 720, 721):
        d, floats = runs(ro, [samples, samples], gap=6)
        case = Case(ro, "raw", d, floats, 8 * BLOCK)
        r = call(case)
        assert r.unit(0).tobytes() == cut_bytes(case, 0) and r.unit(1).tobytes() == cut_bytes(case, 1), samples


def case_slots(ro, call):
    """eight recorders in one image: every slot's unit is its own columns; a recorder that is not wanted is skipped"""
    cols = 64
    windows = [(8 * s, 8 - s % 3) for s in range(SLOTS)]
    windows[5] = (0, 0)
    d, floats = images(ro, [(5 + s, s) for s in range(SLOTS)] + [(3, 6), (2, 0)], cols)
    case = Case(ro, "image", d, floats, 12 * BLOCK, cols, windows)
    r = call(case)
    assert statuses(r) == [WRITTEN] * 5 + [SKIPPED] + [WRITTEN] * 4
    assert r.dir["naxis1"].tolist() == [8, 7, 6, 8, 7, 0, 8, 7, 8, 8]
    for i in range(10):
        if i != 5:
            assert r.unit(i).tobytes() == cut_bytes(case, i), i


def case_bits(ro, call):
    """a bit copy: NaN payloads, -0, denormals and infinities come out with their bytes reversed and nothing else changed"""
    bits = np.array([0x7fc12345, 0xffa00001, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000,
                     0x3f800000, 0x01020304], np.uint32)
    d, _ = images(ro, [(2, 0)], 5)
    r = call(Case(ro, "image", d, bits.view(np.float32), BLOCK, 5, [(1, 3)] + [(0, 0)] * 7))
    want = bits.reshape(2, 5)[:, 1:4].reshape(-1).byteswap().tobytes()
    assert r.unit(0).tobytes() == want + bytes(BLOCK - len(want))
    d, _ = runs(ro, [5])
    r = call(Case(ro, "raw", d, bits.view(np.float32), BLOCK))
    assert r.unit(0).tobytes() == bits.byteswap().tobytes() + bytes(BLOCK - 40)


TABLE = [case_order_of_the_rules, case_arena_edge, case_room, case_counts_out_of_range, case_blocks, case_slots, case_bits]


def case_from_emu(ro, args):
    """emu_units.random_case's arguments as a Case"""
    raw = args["windows"] is None
    d = np.ascontiguousarray(args["directory"]).view(ro.capi.RAW_CAPTURE_DTYPE if raw else ro.capi.SNAPSHOT_DTYPE)
    return Case(ro, "raw" if raw else "image", d, args["arena"], args["units_bytes"], args["cols"], args["windows"],
                resolved=args["resolved"])


def refusals(d, raw):
    """(changed arguments, word the text must hold); d: "d_" for the resident calls' argument names"""
    out = [(dict(summary=None), "null %s%s" % (d, "raw_summary" if raw else "snap_summary")),
           (dict(unit_dir=None), "null %sunit_dir" % d), (dict(out=None), "null %sunit_summary" % d),
           (dict(dir=None), "null %s%s with" % (d, "raw_dir" if raw else "dir")), (dict(arena=None), "null %sarena" % d),
           (dict(units=None), "null %sunits" % d), (dict(dcap=-1), "dir_capacity"), (dict(arena_floats=-1), "arena_floats"),
           (dict(units_bytes=-1), "units_bytes"), (dict(dcap=(1 << 24) + 1), "dir_capacity"),
           (dict(units="arena"), "overlaps"), (dict(units="arena end"), "overlaps")]
    if not raw:
        out += [(dict(cols=0), "cols"), (dict(cols=-5), "cols"), (dict(windows=None), "null slot_windows"),
                (dict(windows={3: (-1, 2)}), "slot_windows[3]"), (dict(windows={0: (0, -1)}), "slot_windows[0]"),
                (dict(windows={7: (5, 6)}), "slot_windows[7]")]          # (the refusal tests' image has 10 columns)
    return out
