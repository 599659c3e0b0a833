"""What tests/test_resize_cpu.py and tests/test_gpu_resize.py share (test infrastructure): the restatement of Pillow's 8-bit
Lanczos resize in numpy and math -- math.sin, the C library's, never numpy's -- which knows nothing of the code under test
and is itself held to Pillow byte for byte; the shape, content and case tables; the plan and the resize through ctypes with
guard bytes behind every output and every buffer at its exact size; the checks every result goes through; the decision table,
written against a `call` so that the host twin and the device walk the very same lines.  Every comparison is exact."""
import ctypes as C
import functools
import math

import numpy as np

from pnglib import LBLOCK, guarded, images, ptr
from unitslib import GUARD, INVALID, NGUARD, NO_ROOM, SKIPPED, WRITTEN

BITS = 22

# (W, H, width): the smallest image that is still resized; a small general one; output width 1; the vertical pass dominates; a
# tall image with the scale just above 1; scale about 1 (9 taps, xmin clamps); an odd width at a scale of about 2; H' = 1;
# Bolidozor's columns; the headline image; the VLF width (31 taps across tile seams); 1641 taps, a span longer than any tile
SHAPES = [(2, 2, 1), (7, 5, 3), (19, 40, 1), (3, 300, 2), (33, 100, 32), (1000, 64, 999), (257, 131, 129), (721, 9, 100),
          (410, 37, 128), (615, 352, 200), (5120, 219, 1024), (70000, 300, 256)]
LONG = (70000, 300, 256)
CONTENTS = ["random", "ones", "zeros", "checker", "bell"]


def shape_id(s):
    return "%dx%d-w%d" % s


def pixels_of(content, w, h, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    if content == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if content == "checker":                                 # 0 / 255 in both axes: both clamps
        return (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    if content == "bell":
        return np.clip(rng.normal(150.0, 30.0, (h, w)), 0, 255).astype(np.uint8)
    return np.full((h, w), 0xFF if content == "ones" else 0, np.uint8)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def out_shape(w, h, width):
    """fits2png:510-514"""
    if 0 < width < w:
        return width, int(float(h) * (float(width) / float(w)))
    return w, h


def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos(t):
    return _sinc(t) * _sinc(t / 3) if -3.0 <= t < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def coeffs(n_in, n_out):
    """[(xmin, int32 taps [xmax])] of every output pixel of one axis"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        k = [v / ww if ww != 0.0 else v for v in w]
        out.append((xmin, np.array([int(v * (1 << BITS) + 0.5) if v >= 0 else int(v * (1 << BITS) - 0.5) for v in k], np.int64)))
    return out


def one_pass(a, n_out):
    """the last axis of a [lines, n_in] uint8 to n_out"""
    lines, n_in = a.shape
    if n_in == n_out:
        return a
    wide = a.astype(np.int64)
    out = np.zeros((lines, n_out), np.uint8)
    for xx, (xmin, taps) in enumerate(coeffs(n_in, n_out)):
        s = (1 << (BITS - 1)) + wide[:, xmin:xmin + len(taps)] @ taps
        assert np.all(np.abs(s) < 1 << 31), "an int32 sum would wrap"
        out[:, xx] = np.clip(s >> BITS, 0, 255)
    return out


def resize(pixels, width):
    """what fits2png's --width makes of a level image [H, W] uint8: the horizontal pass rounded to uint8, then the vertical one;
    None where the height becomes 0"""
    h, w = pixels.shape
    w2, h2 = out_shape(w, h, width)
    if h2 == 0:
        return None
    mid = one_pass(np.ascontiguousarray(pixels), w2)
    return np.ascontiguousarray(one_pass(np.ascontiguousarray(mid.T), h2).T)


@functools.lru_cache(maxsize=None)
def reference(content, shape, seed=0):
    """(the source, its resize by the restatement), computed once and shared; read only"""
    w, h, width = shape
    px = pixels_of(content, w, h, seed)
    out = resize(px, width)
    px.setflags(write=False)
    if out is not None:
        out.setflags(write=False)
    return px, out


def room_of(w, h, width):
    w2, h2 = out_shape(w, h, width)
    return -(-w2 * h2 // LBLOCK) * LBLOCK


# ---- the calls -------------------------------------------------------------------------------------------------------------------
class Case:
    """the arguments of one plan and one resize: a level directory (FITS_UNIT_DTYPE), its summary, the levels, the width, the
    room of the out levels"""

    def __init__(self, ro, level_dir, levels, width, out_bytes, entries=None, dcap=None):
        self.level_dir = np.ascontiguousarray(level_dir)
        assert self.level_dir.dtype == ro.capi.FITS_UNIT_DTYPE
        self.dcap = len(level_dir) if dcap is None else dcap
        self.summary = np.zeros(1, ro.capi.UNIT_SUMMARY_DTYPE)
        self.summary["entries"] = len(level_dir) if entries is None else entries
        self.levels = np.ascontiguousarray(levels, np.uint8)
        self.width = width
        self.out_bytes = out_bytes

    def with_room(self, out_bytes):
        other = Case.__new__(Case)
        other.__dict__.update(self.__dict__)
        other.out_bytes = out_bytes
        return other


class Plan:
    """what ro_resize_plan writes, guards included: the sizing form first, then the blob at its exact size"""

    def __init__(self, ro, case):
        lib = ro.library()
        self.dir_bytes, self.summary_bytes = guarded(case.dcap * 32, NGUARD * 32), guarded(64, NGUARD * 64)
        self.info = np.zeros(1, ro.capi.RESIZE_INFO_DTYPE)
        level_dir, summary = case.level_dir.copy(), case.summary.copy()
        args = (ptr(level_dir) if case.dcap else None, case.dcap, ptr(summary), case.levels.size, case.width, ptr(self.dir_bytes),
                case.out_bytes, ptr(self.summary_bytes))
        assert lib.ro_resize_plan(*args, None, 0, ptr(self.info)) == 0, lib.ro_last_error()
        sized = (self.dir_bytes.copy(), self.summary_bytes.copy(), self.info.copy())
        n = int(self.info["plan_bytes"][0])
        assert n >= 64 and n % 16 == 0
        self.blob = np.full(n // 8 + 8, GUARD * 0x0101010101010101, np.uint64).view(np.uint8)      # (8-byte aligned)
        assert lib.ro_resize_plan(*args, ptr(self.blob), n, ptr(self.info)) == 0, lib.ro_last_error()
        assert np.all(self.blob[n:] == GUARD), "bytes behind the plan were touched"
        self.blob = self.blob[:n]
        for a, b in zip(sized, (self.dir_bytes, self.summary_bytes, self.info)):
            assert a.tobytes() == b.tobytes(), "the sizing form differs from the writing one"
        assert level_dir.tobytes() == case.level_dir.tobytes() and summary.tobytes() == case.summary.tobytes()
        assert not self.info["reserved"].any() and all(int(self.info[k][0]) >= 0 for k in ("jobs", "h_items", "v_items", "mid_bytes"))


class Result:
    """everything a plan and a resize write, guards included, as bytes; and the parts in use, typed"""

    def __init__(self, ro, case, plan, out_levels):
        self.plan = plan
        self.raw = (plan.dir_bytes, plan.summary_bytes, out_levels)
        self.summary = plan.summary_bytes[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
        s = self.summary
        n, used = int(s["entries"]), int(s["units_bytes"])
        assert 0 <= n <= case.dcap and 0 <= used <= case.out_bytes and used % LBLOCK == 0 and int(s["reserved"]) == 0, s
        self.dir = plan.dir_bytes[:n * 32].view(ro.capi.FITS_UNIT_DTYPE)
        self.levels = out_levels[:used]
        assert np.all(plan.dir_bytes[n * 32:] == GUARD), "directory entries at or behind n were touched"
        assert np.all(out_levels[used:] == GUARD), "bytes of the out levels past the ones in use were touched"
        assert np.all(plan.summary_bytes[64:] == GUARD)
        st = self.dir["status"]
        assert [int(s[k]) for k in ("written", "skipped", "no_room", "invalid")] == [int((st == k).sum()) for k in range(4)]
        assert int(plan.info["jobs"][0]) == int(s["written"])
        have = self.dir[(st == WRITTEN) | (st == NO_ROOM)]
        assert all(int(e["bytes"]) == int(e["naxis1"]) * int(e["naxis2"]) > 0 for e in have)
        rooms = [-(-int(e["bytes"]) // LBLOCK) * LBLOCK for e in have]
        assert int(s["needed_bytes"]) == sum(rooms)
        written = int(s["written"])
        assert self.dir["offset"][st == WRITTEN].tolist() == [sum(rooms[:i]) for i in range(written)]      # the prefix rule
        assert used == sum(rooms[:written])
        for k in (SKIPPED, INVALID):
            assert self.dir[st == k].tobytes() == (bytes(28) + bytes([k, 0, 0, 0])) * int((st == k).sum())
        assert not self.dir["offset"][st == NO_ROOM].any()
        for e, room in zip(self.dir[st == WRITTEN], rooms):     # the pad behind every image is zero
            assert not self.levels[int(e["offset"]) + int(e["bytes"]):int(e["offset"]) + room].any()

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw)) and self.plan.blob.tobytes() == other.plan.blob.tobytes()

    def image(self, d):
        e = self.dir[d]
        assert e["status"] == WRITTEN, e
        return self.levels[int(e["offset"]):int(e["offset"]) + int(e["bytes"])].reshape(int(e["naxis2"]), int(e["naxis1"]))

    def written(self):
        return [int(d) for d in np.flatnonzero(self.dir["status"] == WRITTEN)]


def host_call(ro, case, plan=None):
    """ro_resize_plan and ro_levels_resize_host through ctypes; the sources must come back unchanged"""
    plan = plan or Plan(ro, case)
    out = guarded(case.out_bytes, NGUARD * 64)
    levels, blob, info = case.levels.copy(), plan.blob.copy(), plan.info.copy()
    lib = ro.library()
    rc = lib.ro_levels_resize_host(ptr(info), ptr(blob), ptr(levels) if levels.size else None, levels.size,
                                   ptr(out) if case.out_bytes else None, case.out_bytes)
    assert rc == 0, lib.ro_last_error()
    assert levels.tobytes() == case.levels.tobytes(), "the levels were written"
    assert blob.tobytes() == plan.blob.tobytes() and info.tobytes() == plan.info.tobytes(), "the plan was written"
    return Result(ro, case, plan, out)


def source_pixels(case, d):
    e = case.level_dir[d]
    return case.levels[int(e["offset"]):int(e["offset"]) + int(e["bytes"])].reshape(int(e["naxis2"]), int(e["naxis1"]))


def check_images(case, r, want=None):
    """every WRITTEN image is the restatement's resize of its level image, byte for byte; want: {entry: the resize}, where the
    caller has it already"""
    for d in r.written():
        px = source_pixels(case, d)
        expect = want[d] if want and d in want else resize(px, case.width)
        assert r.image(d).shape == expect.shape and np.array_equal(r.image(d), expect), "entry %d differs from the restatement" % d


def host_vs_python(ro):
    def call(case):
        r = host_call(ro, case)
        check_images(case, r)
        return r
    return call


def statuses(r):
    return r.dir["status"].tolist()


# ---- the shape table -------------------------------------------------------------------------------------------------------------
def shape_case(ro, shape, content):
    """the image behind a one-pixel one, so that nothing starts at level byte 0; -> (case, {1: the expected resize})"""
    w, h, width = shape
    px, want = reference(content, shape)
    d, levels = images(ro, [pixels_of("random", 1, 1), px], pad=64)
    return Case(ro, d, levels, width, LBLOCK + room_of(w, h, width)), {1: want}


def one_call_shapes(width):
    """the shapes that go in one call under `width`: all of them at the long shape's own width, the others elsewhere"""
    return [s for s in SHAPES if s != LONG or width == LONG[2]]


def all_shapes_case(ro, shapes, width):
    """the shapes as one directory under ONE width, each with another content"""
    items = [pixels_of(CONTENTS[i % len(CONTENTS)], w, h, 3) for i, (w, h, _) in enumerate(shapes)]
    d, levels = images(ro, items, pad=64)
    return Case(ro, d, levels, width, sum(room_of(w, h, width) for w, h, _ in shapes))


# ---- the decision table: one case per function -----------------------------------------------------------------------------------
def small(seed, w, h):
    return pixels_of("random", w, h, seed)


def case_skipped_and_invalid(ro, call):
    """rule 1, one entry per clause of rule 2, and rule 3 (H' = 0: 9 x 2 at width 4), between two writable ones"""
    d, levels = images(ro, [small(1, 15, 6), (None, SKIPPED), (None, NO_ROOM), (None, INVALID)] + [small(2, 14, 4)] * 7 +
                       [small(3, 9, 2), small(4, 12, 8)])
    bad = d[4:11]
    bad["naxis1"][0] = 0
    bad["naxis2"][1] = 0
    bad["bytes"][2] += 1                                    # not naxis1 naxis2
    bad["offset"][3] = -LBLOCK
    bad["offset"][4] += 16                                  # not a multiple of 720
    bad["offset"][5] = len(levels) // LBLOCK * LBLOCK       # offset + bytes beyond the levels
    bad["naxis1"][6], bad["naxis2"][6], bad["bytes"][6] = 1 << 30, 4, 1 << 32       # no image of fewer than 2^31 pixels
    r = call(Case(ro, d, levels, 4, 4096))
    assert statuses(r) == [WRITTEN] + [SKIPPED] * 3 + [INVALID] * 7 + [SKIPPED, WRITTEN]
    assert r.dir["naxis1"].tolist()[0::12] == [4, 4] and r.dir["naxis2"].tolist()[0::12] == [1, 2]
    assert r.dir["offset"].tolist()[-1] == LBLOCK


def case_copy(ro, call):
    """width >= W: the image is a job too, a plain copy -- of one block, of several, of one that ends a block exactly"""
    items = [small(5, 8, 3), small(6, 16, 45), small(7, 9, 2000), small(8, 30, 7)]
    d, levels = images(ro, items)
    for width in (30, 31, 1 << 30):
        r = call(Case(ro, d, levels, width, len(levels)))
        assert statuses(r) == [WRITTEN] * 4 and r.dir.tobytes() == d.tobytes()
        assert r.levels.tobytes() == levels.tobytes()
    r = call(Case(ro, d, levels, 9, len(levels)))            # two copies, two resized
    assert [tuple(x) for x in zip(r.dir["naxis1"].tolist(), r.dir["naxis2"].tolist())] == [(8, 3), (9, 25), (9, 2000), (9, 2)]
    assert np.array_equal(r.image(0), items[0]) and np.array_equal(r.image(2), items[2])


def case_room(ro, call):
    """exactly needed_bytes; one byte short; the prefix rule: nothing behind the first misfit fits; none at all, out levels NULL;
    a second call with needed_bytes writes all"""
    d, levels = images(ro, [small(9, 90, 40), small(10, 300, 20), (None, SKIPPED), small(11, 12, 5), small(12, 200, 150), small(13, 20, 10)])
    width = 50
    rooms = [room_of(90, 40, width), room_of(300, 20, width), room_of(12, 5, width), room_of(200, 150, width), room_of(20, 10, width)]
    assert rooms == [2 * LBLOCK, LBLOCK, LBLOCK, 3 * LBLOCK, LBLOCK]
    need = sum(rooms)
    case = Case(ro, d, levels, width, 0)
    full = call(case.with_room(need))
    assert statuses(full) == [WRITTEN, WRITTEN, SKIPPED, WRITTEN, WRITTEN, WRITTEN]
    assert int(full.summary["needed_bytes"]) == int(full.summary["units_bytes"]) == need
    for room, written in ((need - 1, 4), (need - rooms[4], 4), (need - rooms[4] - 1, 3), (sum(rooms[:2]) + 17, 2), (rooms[0], 1),
                          (rooms[0] - 1, 0), (0, 0)):
        r = call(case.with_room(room))
        want = [WRITTEN if i < written else NO_ROOM for i in range(5)]
        assert statuses(r) == want[:2] + [SKIPPED] + want[2:], (room, statuses(r))
        assert int(r.summary["needed_bytes"]) == need and r.dir["naxis1"].tolist() == [50, 50, 0, 12, 50, 20]
        assert r.levels.tobytes() == full.levels[:len(r.levels)].tobytes()           # an image does not depend on the room
        assert call(case.with_room(int(r.summary["needed_bytes"]))).same_bytes(full)
    # the last image would fit behind the third, but the fourth does not: nothing behind it fits
    r = call(case.with_room(sum(rooms[:3]) + rooms[4]))
    assert statuses(r) == [WRITTEN, WRITTEN, SKIPPED, WRITTEN, NO_ROOM, NO_ROOM]


def case_entries_clamped(ro, call):
    """n = min(max(entries, 0), dir_capacity): beyond the capacity, inside it (entries behind n untouched), negative, zero"""
    d, levels = images(ro, [small(14, 13, 9), small(15, 18, 4), small(16, 12, 6)])
    room = 3 * LBLOCK
    assert len(call(Case(ro, d, levels, 6, room, entries=1 << 40)).dir) == 3
    assert len(call(Case(ro, d, levels, 6, room, entries=7, dcap=2)).dir) == 2
    r = call(Case(ro, d, levels, 6, room, entries=2))
    assert statuses(r) == [WRITTEN, WRITTEN] and int(r.summary["units_bytes"]) == 2 * LBLOCK
    for n in (0, -5):
        r = call(Case(ro, d, levels, 6, room, entries=n))
        assert r.summary.tobytes() == bytes(64) and len(r.levels) == 0 and int(r.plan.info["plan_bytes"][0]) == 64
    r = call(Case(ro, d[:0], levels[:0], 6, 0))
    assert r.summary.tobytes() == bytes(64)


def table_bytes(n_in, n_out):
    """what one tap table may take: 16 bytes, xmin and xmax, and no more than ksize taps per output pixel, rounded up to 16"""
    ksize = int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1
    return -(-(16 + 8 * n_out + 4 * n_out * ksize) // 16) * 16


def case_many_entries(ro, call):
    """600 small entries of few distinct shapes, every third one skipped, room for 350 images: the taps are shared between
    entries and axes, not repeated -- the plan is bounded by the distinct (in, out) pairs"""
    shapes = [(16 + i % 5, 8 + i % 3) for i in range(600)]
    px = [small(100 + i, w, h) for i, (w, h) in enumerate(shapes)]
    d, levels = images(ro, [(p, SKIPPED) if i % 3 == 1 else p for i, p in enumerate(px)])
    r = call(Case(ro, d, levels, 8, 350 * LBLOCK + 700))
    assert int(r.summary["written"]) == 350 and int(r.summary["no_room"]) == 50 and int(r.summary["skipped"]) == 200
    assert int(r.summary["needed_bytes"]) == 400 * LBLOCK
    pairs = set()
    for w, h in shapes:
        w2, h2 = out_shape(w, h, 8)
        pairs |= {(w, w2), (h, h2)}
    pairs = {p for p in pairs if p[0] != p[1]}
    assert int(r.plan.info["plan_bytes"][0]) <= 64 + 350 * 80 + sum(table_bytes(*p) for p in pairs)


TABLE = [case_skipped_and_invalid, case_copy, case_room, case_entries_clamped, case_many_entries]


def plan_refusals():
    """[(what to change in ro_resize_plan's call, a word of the message)]"""
    return [(dict(dcap=-1), "dir_capacity"), (dict(levels_bytes=-1), "levels_bytes"), (dict(out_bytes=-1), "out_levels_bytes"),
            (dict(plan_bytes=-1), "plan_bytes"), (dict(width=0), "width"), (dict(width=-3), "width"), (dict(summary=None), "level_summary"),
            (dict(level_dir=None), "level_dir"), (dict(dcap=(1 << 24) + 1), "2^24"), (dict(out_dir=None), "out_level_dir"),
            (dict(out=None), "out_level_summary"), (dict(info=None), "info"), (dict(plan=None), "null plan"),
            (dict(plan="odd"), "aligned"), (dict(plan_bytes=64), "plan_bytes")]


def resize_refusals(d):
    """[(what to change in a resize call, a word of the message)]: d is "d_" for the resident call's argument names"""
    return [(dict(info=None), "info"), (dict(info="negative"), "info"), (dict(plan=None), d + "plan"), (dict(levels_bytes=-1), "levels_bytes"),
            (dict(out_bytes=-1), "out_levels_bytes"), (dict(levels=None), d + "levels"), (dict(out=None), d + "out_levels"),
            (dict(out="levels"), "overlaps " + d + "levels"), (dict(out="levels end"), "overlaps " + d + "levels"),
            (dict(out="plan"), "overlaps " + d + "plan")]
