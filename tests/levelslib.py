"""What tests/test_levels_cpu.py and tests/test_gpu_levels.py share (test infrastructure): the grey-level previews' calls
through ctypes with guard bytes behind every output, over the Cases of unitslib (event snapshots; `units_bytes` of such a Case
is the room in LEVEL bytes here) and of periodiclib (periodic snapshots; the levels' room is a quarter of the case's
units_bytes); the source image of an entry, cut on the host; the checks every result goes through -- the geometry, the
directory as a quarter of the units', the oracle's fits2png restatement byte for byte -- and the decision tables, written
against a `call` so that the host twins and the device walk the very same lines."""
import ctypes as C

import numpy as np

import periodiclib as P
import unitslib as U
from unitslib import GUARD, INVALID, NGUARD, NO_ROOM, SKIPPED, SLOTS, WRITTEN
from util import add_tone, noise_iq

LBLOCK = 720                                              # RO_LEVEL_BLOCK
CAPTURED, EMPTY, LOST = U.CAPTURED, U.EMPTY, U.LOST


def blocks_of(naxis1, naxis2):
    return -(-naxis1 * naxis2 // LBLOCK)


def magnitudes(rng, n):
    """n positive float32: magnitudes of noise plus a tone (at least 512 are made: their ln spans several units)"""
    iq = add_tone(noise_iq(rng, max(n, 512)), 6000.0, 1.0)
    m = np.hypot(iq[:, 0], iq[:, 1]).astype(np.float32)
    assert np.all(m > 0) and np.log(m.max()) - np.log(m.min()) > 2.0
    return m[:n].copy()


def magnitude_ring(rng, ring_rows, cols, stride=None):
    """a ring [ring_rows, stride] whose every slot holds magnitudes in its first `cols` floats, periodiclib.PAD behind them"""
    stride = cols if stride is None else stride
    ring = np.full((ring_rows, stride), P.PAD, np.float32)
    ring[:, :cols] = magnitudes(rng, ring_rows * cols).reshape(ring_rows, cols)
    return ring


def pcase(seed, recorders, head_row, ring_rows, cols, units_bytes, stride=None, **kw):
    """periodiclib.Case over a ring of magnitudes"""
    return P.Case(recorders, head_row, ring_rows, cols, units_bytes,
                  ring=magnitude_ring(np.random.default_rng(seed), ring_rows, cols, stride), **kw)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


# ---- event snapshots -----------------------------------------------------------------------------------------------------------
class Result:
    """everything a snapshot-levels call writes, guards included, as bytes; and the parts in use, typed"""

    def __init__(self, ro, case, dir_bytes, range_bytes, level_bytes, summary_bytes):
        self.raw = (dir_bytes, range_bytes, level_bytes, summary_bytes)
        self.summary = summary_bytes[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
        s = self.summary
        n, used = int(s["entries"]), int(s["units_bytes"])
        assert 0 <= n <= case.dcap and 0 <= used <= case.units_bytes and used % LBLOCK == 0 and int(s["reserved"]) == 0, s
        self.dir = dir_bytes[:n * 32].view(ro.capi.FITS_UNIT_DTYPE)
        self.ranges = range_bytes[:n * 8].view(ro.capi.LEVEL_RANGE_DTYPE)
        self.levels = level_bytes[:used]
        assert np.all(dir_bytes[n * 32:] == GUARD), "level directory entries at or behind n were touched"
        assert np.all(range_bytes[n * 8:] == GUARD), "ranges at or behind n were touched"
        assert np.all(level_bytes[used:] == GUARD), "bytes of the levels past the ones in use were touched"
        assert np.all(summary_bytes[64:] == GUARD)
        st = self.dir["status"]
        assert [int(s[k]) for k in ("written", "skipped", "no_room", "invalid")] == [int((st == k).sum()) for k in range(4)]
        have = [(int(e["naxis1"]), int(e["naxis2"])) for e in self.dir if e["status"] in (WRITTEN, NO_ROOM)]
        sizes = [blocks_of(*x) for x in have]
        assert all(int(e["bytes"]) == a * b for e, (a, b) in zip(self.dir[(st == WRITTEN) | (st == NO_ROOM)], have))
        assert int(s["needed_bytes"]) == LBLOCK * sum(sizes)
        written = int(s["written"])
        assert self.dir["offset"][st == WRITTEN].tolist() == [LBLOCK * sum(sizes[:i]) for i in range(written)]
        assert used == LBLOCK * sum(sizes[:written])
        for k in (SKIPPED, INVALID):
            assert self.dir[st == k].tobytes() == (bytes(28) + bytes([k, 0, 0, 0])) * int((st == k).sum())
        assert not self.dir["offset"][st == NO_ROOM].any()
        assert self.ranges[st != WRITTEN].tobytes() == bytes(8 * int((st != WRITTEN).sum())), "a range of an entry that is not WRITTEN"
        for d in np.flatnonzero(st == WRITTEN):             # the padding behind every image is zero
            e = self.dir[d]
            assert not self.levels[int(e["offset"]) + int(e["bytes"]):int(e["offset"]) + LBLOCK * blocks_of(int(e["naxis1"]), int(e["naxis2"]))].any()

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw))

    def pixels(self, d):
        """the levels of entry d's image, uint8 [naxis2, naxis1]"""
        e = self.dir[d]
        assert e["status"] == WRITTEN, e
        return self.levels[int(e["offset"]):int(e["offset"]) + int(e["bytes"])].reshape(int(e["naxis2"]), int(e["naxis1"]))

    def written(self):
        return [int(d) for d in np.flatnonzero(self.dir["status"] == WRITTEN)]


def outputs_for(case):
    """(level_dir, ranges, levels, summary) byte arrays with guards behind"""
    return (U.guarded(case.dcap * 32, NGUARD * 32), U.guarded(case.dcap * 8, NGUARD * 8), U.guarded(case.units_bytes, NGUARD * 64),
            U.guarded(64, NGUARD * 64))


def host_call(ro, case):
    """ro_snapshot_levels_host through ctypes; the sources must come back unchanged"""
    outs = outputs_for(case)
    directory, summary, arena = case.directory.copy(), case.summary.copy(), case.arena.copy()
    lib = ro.library()
    rc = lib.ro_snapshot_levels_host(ptr(directory) if case.dcap else None, case.dcap, ptr(summary), ptr(arena) if arena.size else None,
                                     arena.size, case.cols, case.window_structs(ro), ptr(outs[0]), ptr(outs[1]),
                                     ptr(outs[2]) if case.units_bytes else None, case.units_bytes, ptr(outs[3]))
    assert rc == 0, lib.ro_last_error()
    assert directory.tobytes() == case.directory.tobytes() and summary.tobytes() == case.summary.tobytes()
    assert arena.tobytes() == case.arena.tobytes(), "the arena was written"
    return Result(ro, case, *outs)


def source_image(case, d):
    """the float32 image of directory entry d, cut to its slot's window: [rows, window cols]"""
    e = case.directory[d]
    first, cols = case.windows[int(e["slot"])]
    image = case.arena[int(e["offset"]):int(e["offset"]) + int(e["rows"]) * case.cols].reshape(-1, case.cols)
    return np.ascontiguousarray(image[:, first:first + cols])


def check_quarter_of_units(ro, case, r):
    """the level directory and summary are ro_snapshot_units_host's over 4 x the room, offsets and bytes divided by four"""
    want = U.host_call(ro, case.with_room(4 * case.units_bytes))
    assert len(want.dir) == len(r.dir)
    for k in ("naxis1", "naxis2", "status"):
        assert r.dir[k].tolist() == want.dir[k].tolist(), k
    assert [4 * int(x) for x in r.dir["offset"]] == want.dir["offset"].tolist()
    assert [4 * int(x) for x in r.dir["bytes"]] == want.dir["bytes"].tolist()
    for k in ("entries", "written", "skipped", "no_room", "invalid"):
        assert int(r.summary[k]) == int(want.summary[k]), k
    assert 4 * int(r.summary["units_bytes"]) == int(want.summary["units_bytes"])
    assert 4 * int(r.summary["needed_bytes"]) == int(want.summary["needed_bytes"])


def check_oracle(oracle, case, r):
    """every WRITTEN image is the oracle's grey image of the cut, byte for byte, and its range exactly"""
    for d in r.written():
        _, u8, (mn, mx) = oracle.ln_levels(source_image(case, d))
        assert r.ranges[d].tobytes() == np.array([mn, mx], np.float32).tobytes(), (d, r.ranges[d], mn, mx)
        assert np.array_equal(r.pixels(d), u8), d


def host_vs_oracle(ro, oracle):
    def call(case):
        r = host_call(ro, case)
        check_quarter_of_units(ro, case, r)
        check_oracle(oracle, case, r)
        return r
    return call


def statuses(r):
    return r.dir["status"].tolist()


# the decision table: one case per function
def case_order_of_the_rules(ro, call):
    """all four statuses in one call: rules 1 - 4 in order (unitslib.case_order_of_the_rules' directory), room for all but the
    last writable entry"""
    cols = 9
    d, floats = U.images(ro, [(3, 0), (2, 1, EMPTY), (4, 2, LOST), (2, 3), (5, 1), (1, 7), (200, 1)], cols)
    windows = [(1, 4), (0, 9), (2, 2), (0, 0), (0, 0), (0, 0), (0, 0), (8, 1)]
    bad = np.repeat(d[4:5], 3)
    bad["slot"][0], bad["rows"][1], bad["offset"][2] = 8, 0, floats - 5 * cols + 1
    directory = np.concatenate([d, bad])
    case = U.Case(ro, "image", directory, magnitudes(np.random.default_rng(3), floats), 3 * LBLOCK, cols, windows)
    r = call(case)
    assert statuses(r) == [WRITTEN, SKIPPED, SKIPPED, SKIPPED, WRITTEN, WRITTEN, NO_ROOM] + [INVALID] * 3
    assert r.dir["naxis1"].tolist()[:7] == [4, 0, 0, 0, 9, 1, 9] and r.dir["bytes"].tolist()[:7] == [12, 0, 0, 0, 45, 1, 1800]
    # a one-pixel image is flat: range min == max, level 0
    assert r.ranges[5]["ln_min"] == r.ranges[5]["ln_max"] and r.pixels(5).tolist() == [[0]]


def case_room(ro, call):
    """exactly needed_bytes; one block less; not a multiple of 720; none at all, the levels NULL; the prefix rule; a second
    call with needed_bytes writes all"""
    cols = 200
    d, floats = U.images(ro, [(3, 0), (8, 1), (4, 2, EMPTY), (1, 0), (9, 1), (1, 3), (2, 0)], cols)      # blocks 1, 3, -, 1, 3, -, 1
    d["rows"][5] = -1
    case = U.Case(ro, "image", d, magnitudes(np.random.default_rng(4), floats), 0, cols, U.whole(cols))
    need = 9 * LBLOCK
    full = call(case.with_room(need))
    assert statuses(full) == [WRITTEN, WRITTEN, SKIPPED, WRITTEN, WRITTEN, INVALID, WRITTEN]
    assert int(full.summary["needed_bytes"]) == int(full.summary["units_bytes"]) == need
    for room, written in ((need - 1, 4), (need - LBLOCK, 4), (need - LBLOCK - 1, 3), (5 * LBLOCK + 17, 3), (LBLOCK, 1),
                          (LBLOCK - 1, 0), (0, 0)):
        r = call(case.with_room(room))
        want = [WRITTEN if i < written else NO_ROOM for i in range(5)]
        assert statuses(r) == want[:2] + [SKIPPED] + want[2:4] + [INVALID] + want[4:], (room, statuses(r))
        assert int(r.summary["needed_bytes"]) == need and r.dir["naxis2"].tolist() == [3, 8, 0, 1, 9, 0, 2]
        assert r.levels.tobytes() == full.levels[:len(r.levels)].tobytes()           # an image's levels do not depend on the room
        assert call(case.with_room(int(r.summary["needed_bytes"]))).same_bytes(full)
    r = call(case.with_room(2 * LBLOCK))
    assert statuses(r)[:4] == [WRITTEN, NO_ROOM, SKIPPED, NO_ROOM]


def case_zero_and_flat(ro, call):
    """an all-zero image: range {+inf, -inf}, all levels 0; a flat image: min == max, all levels 0; an image with zero
    pixels: they take no part in the range and are level 0"""
    cols = 40
    d, floats = U.images(ro, [(20, 0), (20, 0), (20, 0), (20, 0)], cols)
    arena = magnitudes(np.random.default_rng(5), floats).reshape(-1, cols)
    arena[0:20] = 0.0
    arena[20:40] = 2.5
    arena[40:60, 3:9] = 0.0
    arena[45] = 0.0
    case = U.Case(ro, "image", d, arena.reshape(-1), 8 * LBLOCK, cols, [(1, 38)] + [(0, 0)] * 7)
    r = call(case)
    assert statuses(r) == [WRITTEN] * 4
    assert r.ranges[0]["ln_min"] == np.inf and r.ranges[0]["ln_max"] == -np.inf and not r.pixels(0).any()
    assert r.ranges[1]["ln_min"] == r.ranges[1]["ln_max"] and abs(r.ranges[1]["ln_min"] - np.log(2.5)) < 1e-6 and not r.pixels(1).any()
    px = r.pixels(2)
    assert not px[:, 2:8].any() and not px[5].any() and px.max() == 255 and np.isfinite(r.ranges[2]["ln_min"])
    assert r.pixels(3).max() == 255 and (r.pixels(3) == 0).sum() >= 1


def case_ranges_do_not_leak(ro, call):
    """two images in one call whose values differ by 10^6: each is quantised against its own range"""
    cols = 30
    d, floats = U.images(ro, [(25, 0), (25, 1)], cols)
    arena = magnitudes(np.random.default_rng(6), floats)
    arena[25 * cols:] *= np.float32(1e6)
    case = U.Case(ro, "image", d, arena, 4 * LBLOCK, cols, [(0, 30), (2, 27)] + [(0, 0)] * 6)
    r = call(case)
    assert statuses(r) == [WRITTEN, WRITTEN]
    assert r.ranges[1]["ln_min"] - r.ranges[0]["ln_max"] > 5.0
    for i in range(2):
        assert r.pixels(i).max() == 255 and r.pixels(i).min() == 0, i            # (a leaked range leaves one image without either)


def case_blocks(ro, call):
    """images that end just in front of, at and behind the block's end, two per call"""
    for naxis1, naxis2 in ((1, 719), (1, 720), (1, 721), (3, 241), (720, 2), (719, 1), (721, 1)):
        d, floats = U.images(ro, [(naxis2, 0), (naxis2, 1)], naxis1 + 2)
        case = U.Case(ro, "image", d, magnitudes(np.random.default_rng(naxis1 + naxis2), floats), 2 * LBLOCK * blocks_of(naxis1, naxis2),
                      naxis1 + 2, [(1, naxis1), (2, naxis1)] + [(0, 0)] * 6)
        r = call(case)
        assert statuses(r) == [WRITTEN, WRITTEN] and len(r.levels) == 2 * LBLOCK * blocks_of(naxis1, naxis2)


def case_slots(ro, call):
    """eight recorders in one image: every slot's preview is of its own columns"""
    cols = 64
    windows = [(8 * s, 8 - s % 3) for s in range(SLOTS)]
    windows[5] = (0, 0)
    d, floats = U.images(ro, [(5 + s, s) for s in range(SLOTS)] + [(3, 6), (2, 0)], cols)
    arena = magnitudes(np.random.default_rng(8), floats)
    r = call(U.Case(ro, "image", d, arena, 12 * LBLOCK, cols, windows))
    assert statuses(r) == [WRITTEN] * 5 + [SKIPPED] + [WRITTEN] * 4 and r.dir["naxis1"].tolist() == [8, 7, 6, 8, 7, 0, 8, 7, 8, 8]


TABLE = [case_order_of_the_rules, case_room, case_zero_and_flat, case_ranges_do_not_leak, case_blocks, case_slots]


def snapshot_refusals(d):
    """(changed arguments, word the text must hold); d: "d_" for the resident call's argument names.  The refusal tests'
    image has 10 columns"""
    return [(dict(summary=None), "null %ssnap_summary" % d), (dict(level_dir=None), "null %slevel_dir" % d),
            (dict(out=None), "null %slevel_summary" % d), (dict(dir=None), "null %sdir with" % d), (dict(arena=None), "null %sarena" % d),
            (dict(levels=None), "null %slevels" % d), (dict(ranges=None), "null %sranges" % d), (dict(dcap=-1), "dir_capacity"),
            (dict(arena_floats=-1), "arena_floats"), (dict(levels_bytes=-1), "levels_bytes"), (dict(dcap=(1 << 24) + 1), "dir_capacity"),
            (dict(levels="arena"), "overlaps"), (dict(levels="arena end"), "overlaps"), (dict(cols=0), "cols"), (dict(cols=-5), "cols"),
            (dict(windows=None), "null slot_windows"), (dict(windows={3: (-1, 2)}), "slot_windows[3]"),
            (dict(windows={0: (0, -1)}), "slot_windows[0]"), (dict(windows={7: (5, 6)}), "slot_windows[7]")]


# ---- periodic snapshots --------------------------------------------------------------------------------------------------------
def room_of(case):
    return case.units_bytes // 4


class PeriodicResult:
    """what a periodic-levels call leaves over a plan's directory: the ranges and the levels with their guards"""

    def __init__(self, ro, case, directory, range_bytes, level_bytes):
        self.dir, self.raw = directory, (range_bytes, level_bytes)
        n = len(directory)
        st = directory["status"]
        assert np.all(range_bytes[n * 8:] == GUARD), "ranges behind the directory were touched"
        self.ranges = range_bytes[:n * 8].view(ro.capi.LEVEL_RANGE_DTYPE)
        assert np.all(range_bytes[:n * 8].reshape(n, 8)[st != P.WRITTEN] == GUARD), "a range of an entry that is not WRITTEN was touched"
        written = directory[st == P.WRITTEN]
        used = 0 if not len(written) else int(written[-1]["offset"]) // 4 + LBLOCK * blocks_of(int(written[-1]["naxis1"]), int(written[-1]["rows"]))
        self.levels = level_bytes[:used]
        assert np.all(level_bytes[used:] == GUARD), "bytes of the levels behind the last written image were touched"
        for e in written:
            at, px = int(e["offset"]) // 4, int(e["naxis1"]) * int(e["rows"])
            assert int(e["offset"]) % 4 == 0 and not self.levels[at + px:at + LBLOCK * blocks_of(int(e["naxis1"]), int(e["rows"]))].any()

    def pixels(self, d):
        e = self.dir[d]
        assert e["status"] == P.WRITTEN, e
        at = int(e["offset"]) // 4
        return self.levels[at:at + int(e["naxis1"]) * int(e["rows"])].reshape(int(e["rows"]), int(e["naxis1"]))

    def written(self):
        return [int(d) for d in np.flatnonzero(self.dir["status"] == P.WRITTEN)]

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw))


def periodic_outputs_for(case, directory):
    return U.guarded(len(directory) * 8, NGUARD * 8), U.guarded(room_of(case), NGUARD * 64)


def periodic_host_call(ro, case, directory):
    """ro_periodic_levels_host through ctypes with guards; the ring must come back unchanged"""
    outs = periodic_outputs_for(case, directory)
    ring = case.ring.copy()
    recs = case.recorder_array(ro)
    lib = ro.library()
    desc = case.ring_struct(ro, ring.ctypes.data)
    rc = lib.ro_periodic_levels_host(C.byref(desc), ptr(recs), len(recs), ptr(directory) if len(directory) else None, len(directory),
                                     ptr(outs[0]), ptr(outs[1]) if room_of(case) else None, room_of(case))
    assert rc == 0, lib.ro_last_error()
    assert ring.tobytes() == case.ring.tobytes(), "the ring was written"
    return PeriodicResult(ro, case, directory, *outs)


def ring_image(case, e):
    """the float32 image of directory entry e, un-wrapped from the ring: [rows, naxis1]"""
    _, first_col, naxis1 = case.recorders[int(e["recorder"])]
    slots = (int(e["first_row"]) + np.arange(int(e["rows"]), dtype=np.int64)) % case.ring_rows
    return np.ascontiguousarray(case.ring[slots, first_col:first_col + naxis1])


def check_periodic_oracle(oracle, case, r):
    for d in r.written():
        _, u8, (mn, mx) = oracle.ln_levels(ring_image(case, r.dir[d]))
        assert r.ranges[d].tobytes() == np.array([mn, mx], np.float32).tobytes(), (d, r.ranges[d], mn, mx)
        assert np.array_equal(r.pixels(d), u8), d


def periodic_host_vs_oracle(ro, oracle):
    def call(case):
        directory, summary, _ = P.plan_call(ro, case)
        r = periodic_host_call(ro, case, directory)
        assert len(r.levels) == int(summary["units_bytes"]) // 4
        check_periodic_oracle(oracle, case, r)
        return r
    return call


def pcase_wrap_lost_and_no_room(ro, call):
    """the ring's wrap (snapshots that straddle the last slot of rings of S + 2, 2 S + 3 and 23 rows); a late call whose older
    snapshots are LOST; a room that leaves NO_ROOM entries: their ranges and bytes are not touched"""
    S = 9
    for ring_rows in (S + 2, 2 * S + 3, 23):
        for k in range(6):
            r = call(pcase(ring_rows + k, [(S, 3, 70)], (k + 1) * S + 2, ring_rows, 77, 4 * P.BLOCK, next_index=[k], stride=80))
            assert r.dir["status"].tolist() == [P.WRITTEN]
    r = call(pcase(1, [(7, 0, 12), (3, 4, 5)], 40, 20, 12, 64 * P.BLOCK))
    assert r.dir["status"].tolist() == [P.LOST] * 3 + [P.WRITTEN] * 2 + [P.LOST] * 7 + [P.WRITTEN] * 5
    r = call(pcase(2, [(7, 1, 200), (5, 0, 33), (11, 100, 150)], 25, 40, 256, 7 * P.BLOCK + 68, stride=259))
    assert r.dir["status"].tolist() == [P.WRITTEN] * 4 + [P.NO_ROOM] * 5
    r = call(pcase(3, [(7, 1, 200)], 25, 40, 256, 0, stride=259))
    assert r.dir["status"].tolist() == [P.NO_ROOM] * 3 and len(r.levels) == 0


def pcase_final(ro, call):
    """`final` with 1 row and with S rows"""
    for H, rows in ((1, [1]), (5, [5]), (7, [5, 2]), (13, [5, 5, 3])):
        r = call(pcase(H, [(5, 1, 3)], H, 16, 5, 8 * P.BLOCK, final=True))
        assert r.dir["rows"].tolist() == rows and r.dir["status"].tolist() == [P.WRITTEN] * len(rows)


def pcase_eight(ro, call):
    """eight recorders in one call: different S, overlapping windows"""
    recorders = [(1 + s, 3 * s, 40 - 4 * s) for s in range(8)]
    r = call(pcase(8, recorders, 30, 32, 64, 64 * P.BLOCK, next_index=[20, 0, 50, 3, 0, 0, 1, 0], stride=67))
    assert sorted(set(r.dir["recorder"].tolist())) == [0, 1, 3, 4, 5, 6, 7] and r.dir["status"].tolist() == [P.WRITTEN] * len(r.dir)


def pcase_odd_first_column(ro, call):
    """stride = cols + 3 with an odd first column, around the block (1 x 719, 720, 721 and 65 x 11, 12)"""
    for naxis1, S in ((1, 719), (1, 720), (1, 721), (65, 11), (65, 12), (721, 1)):
        r = call(pcase(naxis1 + S, [(S, 1, naxis1)], 2 * S + 2, 2 * S + 3, naxis1 + 1, 2 * P.BLOCK * P.blocks_of(naxis1, S), stride=naxis1 + 4))
        assert r.dir["status"].tolist() == [P.WRITTEN] * 2 and r.dir["offset"].tolist() == [0, P.BLOCK * P.blocks_of(naxis1, S)]


PERIODIC_TABLE = [pcase_wrap_lost_and_no_room, pcase_final, pcase_eight, pcase_odd_first_column]


def periodic_refusals(d):
    """periodiclib.unit_refusals in the levels' argument names -- the same cases the units' calls refuse, the room a quarter
    -- and what the levels' calls add"""
    out = []
    for kw, word in P.unit_refusals(d):
        kw = dict(kw)
        if "units" in kw:
            kw["levels"] = kw.pop("units")
        if "units_bytes" in kw:
            v = kw.pop("units_bytes")
            kw["levels_bytes"] = v if v < 0 else v // 4
        out.append((kw, word.replace("units", "levels")))
    return out + [(dict(ranges=None), "null %sranges" % d), (dict(levels_bytes=5 * LBLOCK - 1), "dir[4]: offset")]
