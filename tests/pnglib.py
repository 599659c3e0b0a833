"""What tests/test_png_cpu.py and tests/test_gpu_png.py share (test infrastructure): the checker of the preview files, which
knows nothing of the code under test -- the expected file of a level image built with struct, zlib.crc32 and zlib.adler32,
and a walk over a produced file chunk by chunk (every chunk's CRC, zlib.decompress of the IDAT data against the raw
scanlines, the stored blocks' headers) and through Pillow; the PNG call through ctypes with guard bytes behind every output;
the checks every result goes through; the shape table and the decision table, written against a `call` so that the host twin
and the device walk the very same lines.  Every comparison is exact."""
import ctypes as C
import io
import struct
import zlib

import numpy as np

from unitslib import GUARD, INVALID, NGUARD, NO_ROOM, SKIPPED, WRITTEN

LBLOCK = 720                                              # RO_LEVEL_BLOCK
ALIGN = 16                                                # RO_PNG_ALIGN
STORED = 65535
SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
IEND = bytes([0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82])

# W x H: the smallest shapes at which the layout can go wrong
SHAPES = [(1, 1), (4368, 15), (255, 256), (4368, 30), (65534, 2), (1, 70000), (615, 352)]
CONTENTS = ["random", "ones", "zeros"]


def file_bytes(w, h):
    raw = h * (w + 1)
    return 63 + 5 * -(-raw // STORED) + raw


def room_of(w, h):
    return -(-file_bytes(w, h) // ALIGN) * ALIGN


def pixels_of(content, w, h, seed=0):
    if content == "random":
        return np.random.default_rng(1000 * seed + w + h).integers(0, 256, (h, w), dtype=np.uint8)
    return np.full((h, w), 0xFF if content == "ones" else 0, np.uint8)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def scanlines(pixels):
    h, w = pixels.shape
    raw = np.zeros((h, w + 1), np.uint8)
    raw[:, 1:] = pixels
    return raw.tobytes()


def expected_file(pixels):
    """the file of a level image [H, W] uint8, to the byte"""
    h, w = pixels.shape
    raw = scanlines(pixels)
    z = b"\x78\x01"
    for at in range(0, len(raw), STORED):
        part = raw[at:at + STORED]
        z += struct.pack("<BHH", 1 if at + STORED >= len(raw) else 0, len(part), len(part) ^ 0xFFFF) + part
    z += struct.pack(">I", zlib.adler32(raw))
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", z) + IEND
    assert len(out) == file_bytes(w, h)
    return out


def walk(data, pixels):
    """a produced file against the level image it was made of, with no help from the code under test"""
    data = bytes(data)
    h, w = pixels.shape
    assert data[:8] == SIGNATURE
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n, "a chunk runs past the file"
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0) and chunks[2][1] == b""
    z = chunks[1][1]
    raw = scanlines(pixels)
    assert zlib.decompress(z) == raw                         # (validates the Adler-32)
    assert z[:2] == b"\x78\x01"
    at, left = 2, len(raw)
    while left:
        final, n, nn = struct.unpack("<BHH", z[at:at + 5])
        assert n == min(left, STORED) and nn == n ^ 0xFFFF and final == (1 if left <= STORED else 0), (at, final, n, nn)
        at += 5 + n
        left -= n
    assert at + 4 == len(z)
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "L" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), pixels)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def guarded(nbytes, guard_bytes):
    return np.full(nbytes + guard_bytes, GUARD, np.uint8)


class Case:
    """the arguments of one call: a level directory (FITS_UNIT_DTYPE), its summary, the levels, the room"""

    def __init__(self, ro, level_dir, levels, png_bytes, entries=None, dcap=None):
        self.level_dir = np.ascontiguousarray(level_dir)
        assert self.level_dir.dtype == ro.capi.FITS_UNIT_DTYPE
        self.dcap = len(level_dir) if dcap is None else dcap
        self.summary = np.zeros(1, ro.capi.UNIT_SUMMARY_DTYPE)
        self.summary["entries"] = len(level_dir) if entries is None else entries
        self.levels = np.ascontiguousarray(levels, np.uint8)
        self.png_bytes = png_bytes

    def with_room(self, png_bytes):
        other = Case.__new__(Case)
        other.__dict__.update(self.__dict__)
        other.png_bytes = png_bytes
        return other


def images(ro, items, pad=0):
    """[pixels [H, W] uint8 or (pixels, status), ...] -> (FITS_UNIT_DTYPE entries in level terms, packed in 720-byte blocks as
    the levels' calls pack them, and the levels + pad bytes of GUARD)"""
    d = np.zeros(len(items), ro.capi.FITS_UNIT_DTYPE)
    parts, offset = [], 0
    for i, item in enumerate(items):
        px, status = item if isinstance(item, tuple) else (item, WRITTEN)
        d[i]["status"] = status
        if status == WRITTEN:
            h, w = px.shape
            d[i]["offset"], d[i]["bytes"], d[i]["naxis2"], d[i]["naxis1"] = offset, w * h, h, w
            room = -(-w * h // LBLOCK) * LBLOCK
            parts.append(np.concatenate([px.reshape(-1), np.zeros(room - w * h, np.uint8)]))
            offset += room
    parts.append(np.full(pad, GUARD, np.uint8))
    return d, np.concatenate(parts)


class Result:
    """everything a call writes, guards included, as bytes; and the parts in use, typed"""

    def __init__(self, ro, case, dir_bytes, png, summary_bytes):
        self.raw = (dir_bytes, png, summary_bytes)
        self.summary = summary_bytes[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
        s = self.summary
        n, used = int(s["entries"]), int(s["units_bytes"])
        assert 0 <= n <= case.dcap and 0 <= used <= case.png_bytes and used % ALIGN == 0 and int(s["reserved"]) == 0, s
        self.dir = dir_bytes[:n * 32].view(ro.capi.FITS_UNIT_DTYPE)
        self.png = png[:used]
        assert np.all(dir_bytes[n * 32:] == GUARD), "directory entries at or behind n were touched"
        assert np.all(png[used:] == GUARD), "bytes of the files past the ones in use were touched"
        assert np.all(summary_bytes[64:] == GUARD)
        st = self.dir["status"]
        assert [int(s[k]) for k in ("written", "skipped", "no_room", "invalid")] == [int((st == k).sum()) for k in range(4)]
        have = self.dir[(st == WRITTEN) | (st == NO_ROOM)]
        assert all(int(e["bytes"]) == file_bytes(int(e["naxis1"]), int(e["naxis2"])) for e in have)
        rooms = [room_of(int(e["naxis1"]), int(e["naxis2"])) for e in have]
        assert int(s["needed_bytes"]) == sum(rooms)
        written = int(s["written"])
        assert self.dir["offset"][st == WRITTEN].tolist() == [sum(rooms[:i]) for i in range(written)]
        assert used == sum(rooms[:written])
        for k in (SKIPPED, INVALID):
            assert self.dir[st == k].tobytes() == (bytes(28) + bytes([k, 0, 0, 0])) * int((st == k).sum())
        assert not self.dir["offset"][st == NO_ROOM].any()
        for e in self.dir[st == WRITTEN]:                   # the pad behind every file is zero
            assert not self.png[int(e["offset"]) + int(e["bytes"]):int(e["offset"]) + room_of(int(e["naxis1"]), int(e["naxis2"]))].any()

    def same_bytes(self, other):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.raw, other.raw))

    def file(self, d):
        e = self.dir[d]
        assert e["status"] == WRITTEN, e
        return self.png[int(e["offset"]):int(e["offset"]) + int(e["bytes"])]

    def written(self):
        return [int(d) for d in np.flatnonzero(self.dir["status"] == WRITTEN)]


def outputs_for(case):
    """(png_dir, png, summary) byte arrays with guards behind"""
    return guarded(case.dcap * 32, NGUARD * 32), guarded(case.png_bytes, NGUARD * 64), guarded(64, NGUARD * 64)


def host_call(ro, case):
    """ro_levels_png_host through ctypes; the sources must come back unchanged"""
    outs = outputs_for(case)
    level_dir, summary, levels = case.level_dir.copy(), case.summary.copy(), case.levels.copy()
    lib = ro.library()
    rc = lib.ro_levels_png_host(ptr(level_dir) if case.dcap else None, case.dcap, ptr(summary), ptr(levels) if levels.size else None,
                                levels.size, ptr(outs[0]), ptr(outs[1]) if case.png_bytes else None, case.png_bytes, ptr(outs[2]))
    assert rc == 0, lib.ro_last_error()
    assert level_dir.tobytes() == case.level_dir.tobytes() and summary.tobytes() == case.summary.tobytes()
    assert levels.tobytes() == case.levels.tobytes(), "the levels were written"
    return Result(ro, case, *outs)


def source_pixels(case, d):
    e = case.level_dir[d]
    return case.levels[int(e["offset"]):int(e["offset"]) + int(e["bytes"])].reshape(int(e["naxis2"]), int(e["naxis1"]))


def check_files(case, r, walk_them=True):
    """every WRITTEN file is the expected file of its level image, byte for byte, and walks"""
    for d in r.written():
        px = source_pixels(case, d)
        assert r.file(d).tobytes() == expected_file(px), d
        if walk_them:
            walk(r.file(d), px)


def host_vs_python(ro):
    def call(case):
        r = host_call(ro, case)
        check_files(case, r)
        return r
    return call


def statuses(r):
    return r.dir["status"].tolist()


# ---- the shape table -------------------------------------------------------------------------------------------------------------
def shape_case(ro, w, h, content):
    """the image behind a one-pixel one, so that it does not start at level byte 0"""
    d, levels = images(ro, [pixels_of("random", 1, 1), pixels_of(content, w, h)], pad=64)
    return Case(ro, d, levels, room_of(1, 1) + room_of(w, h))


# ---- the decision table: one case per function -----------------------------------------------------------------------------------
def small(seed, w, h):
    return pixels_of("random", w, h, seed)


def case_skipped_and_invalid(ro, call):
    """rule 1, and one entry per clause of rule 2, between two writable ones"""
    d, levels = images(ro, [small(1, 5, 3), (None, SKIPPED), (None, NO_ROOM), (None, INVALID)] + [small(2, 7, 2)] * 9 + [small(3, 4, 4)])
    bad = d[4:13]
    bad["naxis1"][0] = 0
    bad["naxis2"][1] = 0
    bad["bytes"][2] += 1                                    # not naxis1 naxis2
    bad["offset"][3] = -LBLOCK
    bad["offset"][4] += 16                                  # not a multiple of 720
    bad["offset"][5] = len(levels) // LBLOCK * LBLOCK       # offset + bytes beyond the levels
    bad["naxis1"][6], bad["naxis2"][6], bad["bytes"][6] = 1, 1 << 30, 1 << 30       # an IDAT beyond 2^31 - 1
    bad["naxis1"][7], bad["naxis2"][7], bad["bytes"][7] = 1 << 30, 4, 1 << 32
    bad["naxis1"][8], bad["bytes"][8] = -7, -14
    case = Case(ro, d, levels, 4096)
    r = call(case)
    assert statuses(r) == [WRITTEN] + [SKIPPED] * 3 + [INVALID] * 9 + [WRITTEN]
    assert r.dir["offset"].tolist()[-1] == room_of(5, 3) and r.dir["bytes"].tolist()[-1] == file_bytes(4, 4)


def case_room(ro, call):
    """exactly needed_bytes; one byte short; the prefix rule: nothing behind the first misfit fits; none at all, png NULL; a
    second call with needed_bytes writes all"""
    d, levels = images(ro, [small(4, 9, 9), small(5, 300, 2), (None, SKIPPED), small(6, 1, 1), small(7, 40, 30), small(8, 2, 1)])
    rooms = [room_of(9, 9), room_of(300, 2), room_of(1, 1), room_of(40, 30), room_of(2, 1)]
    need = sum(rooms)
    case = Case(ro, d, levels, 0)
    full = call(case.with_room(need))
    assert statuses(full) == [WRITTEN, WRITTEN, SKIPPED, WRITTEN, WRITTEN, WRITTEN]
    assert int(full.summary["needed_bytes"]) == int(full.summary["units_bytes"]) == need
    for room, written in ((need - 1, 4), (need - rooms[4], 4), (need - rooms[4] - 1, 3), (sum(rooms[:2]) + 17, 2), (rooms[0], 1),
                          (rooms[0] - 1, 0), (0, 0)):
        r = call(case.with_room(room))
        want = [WRITTEN if i < written else NO_ROOM for i in range(5)]
        assert statuses(r) == want[:2] + [SKIPPED] + want[2:], (room, statuses(r))
        assert int(r.summary["needed_bytes"]) == need and r.dir["naxis1"].tolist() == [9, 300, 0, 1, 40, 2]
        assert r.png.tobytes() == full.png[:len(r.png)].tobytes()                    # a file does not depend on the room
        assert call(case.with_room(int(r.summary["needed_bytes"]))).same_bytes(full)
    # the one-pixel file would fit behind the first, but the second does not: nothing behind it fits
    r = call(case.with_room(rooms[0] + rooms[2]))
    assert statuses(r) == [WRITTEN, NO_ROOM, SKIPPED, NO_ROOM, NO_ROOM, NO_ROOM]


def case_entries_clamped(ro, call):
    """n = min(max(entries, 0), dir_capacity): beyond the capacity, inside it (entries behind n untouched), negative, zero"""
    d, levels = images(ro, [small(9, 3, 3), small(10, 8, 1), small(11, 2, 6)])
    room = 3 * 128
    assert len(call(Case(ro, d, levels, room, entries=1 << 40)).dir) == 3
    assert len(call(Case(ro, d, levels, room, entries=7, dcap=2)).dir) == 2
    r = call(Case(ro, d, levels, room, entries=2))
    assert statuses(r) == [WRITTEN, WRITTEN] and int(r.summary["units_bytes"]) == room_of(3, 3) + room_of(8, 1)
    for n in (0, -5):
        r = call(Case(ro, d, levels, room, entries=n))
        assert r.summary.tobytes() == bytes(64) and len(r.png) == 0
    r = call(Case(ro, d[:0], levels[:0], 0))
    assert r.summary.tobytes() == bytes(64)


def case_many_entries(ro, call):
    """more than one tile of the plan: 600 entries, every third one skipped, room for 350 files"""
    px = [small(100 + i, 1 + i % 7, 1 + i % 5) for i in range(600)]
    d, levels = images(ro, [(p, SKIPPED) if i % 3 == 1 else p for i, p in enumerate(px)])
    rooms = [room_of(*p.shape[::-1]) for i, p in enumerate(px) if i % 3 != 1]
    r = call(Case(ro, d, levels, sum(rooms[:350]) + 15))
    assert int(r.summary["written"]) == 350 and int(r.summary["no_room"]) == 50 and int(r.summary["skipped"]) == 200
    assert int(r.summary["needed_bytes"]) == sum(rooms)


TABLE = [case_skipped_and_invalid, case_room, case_entries_clamped, case_many_entries]


def refusals(d):
    """[(what to change in the call, a word of the message)]: d is "d_" for the resident call's argument names"""
    return [(dict(dcap=-1), "dir_capacity"), (dict(levels_bytes=-1), "levels_bytes"), (dict(png_bytes=-1), "png_bytes"),
            (dict(summary=None), d + "level_summary"), (dict(level_dir=None), d + "level_dir"), (dict(dcap=(1 << 24) + 1), "2^24"),
            (dict(levels=None), d + "levels"), (dict(png_dir=None), d + "png_dir"), (dict(out=None), d + "png_summary"),
            (dict(png=None), d + "png"), (dict(png="levels"), "overlaps"), (dict(png="levels end"), "overlaps")]
