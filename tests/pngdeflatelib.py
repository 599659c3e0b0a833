"""What tests/test_png_deflate_cpu.py and tests/test_gpu_png_deflate.py share (test infrastructure): a restatement of the
compressed preview file of include/ro_stft.h, written from its text with struct, zlib.crc32 and zlib.adler32 and none of the
code under test -- literal-only dynamic-Huffman deflate blocks (two-queue construction, the 15-bit limit rule, canonical
codes) or stored ones, whichever is shorter; a walk over a produced file that does not use the restatement (chunk CRCs,
zlib.decompress, Pillow, the size bound); the deflate calls through ctypes with guard bytes behind every output; the checks
every result goes through, for files whose sizes depend on their data; the content table.  pnglib's Case, images, guards and
decision table are used as they are.  Every comparison is exact."""
import io
import struct
import zlib

import numpy as np

import pnglib as G
from pnglib import ALIGN, GUARD, NGUARD, STORED, Case, images, outputs_for, ptr, scanlines  # noqa: F401
from unitslib import INVALID, NO_ROOM, SKIPPED, WRITTEN  # noqa: F401

CONTENTS = ["random", "ones", "zeros", "noise", "fib", "mixed"]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
HEAD_BITS = 1106


def pixels_of(content, w, h, seed=0):
    n = w * h
    if content in G.CONTENTS:
        return G.pixels_of(content, w, h, seed)
    rng = np.random.default_rng(7000 * seed + 3 * w + h)
    if content == "noise":
        # ln of Rayleigh magnitudes, the image's own min / max on 0 ... 255 (what the level calls leave of receiver noise)
        ln = np.log(np.hypot(rng.standard_normal(n), rng.standard_normal(n)).astype(np.float32))
        return ((ln - ln.min()) / max(float(ln.max() - ln.min()), 1e-30) * 255).astype(np.uint8).reshape(h, w)
    if content == "fib":
        # with end-of-block's 1, every 65535 raw bytes have the frequencies 1, 1, 2, 3, 5, ...: value k stands F(k + 1) times; the
        # filter bytes and the rest are value 0.  Every join takes the node made last and the next leaf: a chain
        fib = [1, 2]
        while sum(fib) + fib[-1] + fib[-2] < 60000:
            fib.append(fib[-1] + fib[-2])
        block = np.concatenate([np.full(f, k + 1, np.uint8) for k, f in enumerate(fib)])
        raw = np.zeros(h * (w + 1), np.uint8)
        for at in range(0, len(raw), STORED):
            part = raw[at:at + STORED]
            free = np.flatnonzero((np.arange(at, at + len(part)) % (w + 1)) != 0)
            part[free[:len(block)]] = block[:len(free)]
        return raw.reshape(h, w + 1)[:, 1:].copy()
    if content == "mixed":
        px = G.pixels_of("random", w, h, seed).reshape(-1)
        px[n // 2:] = 0
        return px.reshape(h, w)
    raise ValueError(content)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def code_lengths(freq):
    """[257 frequencies] -> ([257 lengths], the limit rule fired)"""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    assert len(used) >= 2
    leaves = [(f, ("leaf", s)) for f, s in used]
    nodes, depth = [], {}
    li = ni = 0

    def take():
        nonlocal li, ni
        if li < len(leaves) and (ni >= len(nodes) or leaves[li][0] <= nodes[ni][0]):
            li += 1
            return leaves[li - 1]
        ni += 1
        return nodes[ni - 1]
    while len(leaves) - li + len(nodes) - ni > 1:
        a, b = take(), take()
        nodes.append((a[0] + b[0], ("node", a[1], b[1])))
    num = [0] * 300
    stack = [(nodes[-1][1], 0)]
    while stack:
        t, d = stack.pop()
        if t[0] == "leaf":
            num[d] += 1
        else:
            stack += [(t[1], d + 1), (t[2], d + 1)]
    fired = any(num[16:])
    num[15] += sum(num[16:])
    num = num[:16]
    total = sum(n << (15 - l) for l, n in enumerate(num) if l)
    while total != 1 << 15:
        num[15] -= 1
        l = max(k for k in range(1, 15) if num[k])
        num[l] -= 1
        num[l + 1] += 2
        total -= 1
    lengths = [0] * 257
    order = iter(sorted(used, key=lambda fs: (-fs[0], fs[1])))
    for l in range(1, 16):
        for _ in range(num[l]):
            lengths[next(order)[1]] = l
    return lengths, fired


def canonical(lengths):
    """RFC 1951 3.2.2"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def plain(value, bits):
    """an integer as the bits of the stream in their order: its lowest bit first"""
    return format(value, "0%db" % bits)[::-1] if bits else ""


def huffman_block(part, final):
    """(the Huffman form of a block's raw bytes with its ending, the limit rule fired)"""
    freq = np.bincount(np.frombuffer(part, np.uint8), minlength=257).tolist()
    freq[256] = 1
    lengths, fired = code_lengths(freq)
    codes = canonical(lengths)
    head = plain(1 if final else 0, 1) + plain(2, 2) + plain(0, 5) + plain(0, 5) + plain(15, 4)
    head += "".join(plain(4 if s < 16 else 0, 3) for s in CL_ORDER)
    head += "".join(format(l, "04b") for l in lengths + [0])           # a Huffman code goes highest bit first
    assert len(head) == HEAD_BITS
    text = {s: format(codes[s], "0%db" % lengths[s]) for s in range(257) if lengths[s]}
    bits = head + "".join(text[v] for v in part) + text[256] + ("" if final else "000")
    bits += "0" * (-len(bits) % 8)
    out = np.packbits(np.frombuffer(bits.encode(), np.uint8) - 48, bitorder="little").tobytes()
    return out + (b"" if final else b"\x00\x00\xff\xff"), fired


def expected_file(pixels, report=None):
    """the file of a level image [H, W] uint8, to the byte; report (a list) gets (form, the limit fired) per block"""
    h, w = pixels.shape
    raw = scanlines(pixels)
    z = b"\x78\x01"
    for at in range(0, len(raw), STORED):
        part = raw[at:at + STORED]
        final = at + STORED >= len(raw)
        huff, fired = huffman_block(part, final)
        if len(huff) < 5 + len(part):
            z += huff
        else:
            z += struct.pack("<BHH", 1 if final else 0, len(part), len(part) ^ 0xFFFF) + part
        if report is not None:
            report.append(("huffman" if len(huff) < 5 + len(part) else "stored", fired))
    z += struct.pack(">I", zlib.adler32(raw))
    out = G.SIGNATURE + G.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + G.chunk(b"IDAT", z) + G.IEND
    assert len(out) <= G.file_bytes(w, h)
    return out


_EXPECTED = {}


def expected_cached(pixels):
    """expected_file and its report, computed once per image"""
    key = (pixels.shape, pixels.tobytes())
    if key not in _EXPECTED:
        report = []
        _EXPECTED[key] = (expected_file(pixels, report), report)
    return _EXPECTED[key]


def walk(data, pixels):
    """a produced file against the level image it was made of, with no help from the restatement or the code under test"""
    data = bytes(data)
    h, w = pixels.shape
    assert len(data) <= G.file_bytes(w, h)
    assert data[:8] == G.SIGNATURE
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
    assert z[:2] == b"\x78\x01"
    inflate = zlib.decompressobj()
    assert inflate.decompress(z) == scanlines(pixels) and inflate.eof and inflate.unused_data == b""      # (validates the Adler-32)
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "L" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), pixels)


# ---- a call's outputs ---------------------------------------------------------------------------------------------------------
def room_of_bytes(n):
    return -(-n // ALIGN) * ALIGN


class Result:
    """everything a call writes, guards included, as bytes; and the parts in use, typed.  pnglib.Result's checks for files
    whose sizes are their own: packed by their actual rooms"""

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
        assert all(0 < int(e["bytes"]) <= G.file_bytes(int(e["naxis1"]), int(e["naxis2"])) for e in have)
        rooms = [room_of_bytes(int(e["bytes"])) for e in have]
        assert int(s["needed_bytes"]) == sum(rooms)
        written = int(s["written"])
        assert self.dir["offset"][st == WRITTEN].tolist() == [sum(rooms[:i]) for i in range(written)]
        assert used == sum(rooms[:written])
        assert (st[(st == WRITTEN) | (st == NO_ROOM)] == WRITTEN).tolist() == [i < written for i in range(len(have))], "the prefix rule"
        for k in (SKIPPED, INVALID):
            assert self.dir[st == k].tobytes() == (bytes(28) + bytes([k, 0, 0, 0])) * int((st == k).sum())
        assert not self.dir["offset"][st == NO_ROOM].any()
        for e in self.dir[st == WRITTEN]:                   # the pad behind every file is zero
            assert not self.png[int(e["offset"]) + int(e["bytes"]):int(e["offset"]) + room_of_bytes(int(e["bytes"]))].any()

    same_bytes = G.Result.same_bytes
    file = G.Result.file
    written = G.Result.written


def host_call(ro, case):
    """ro_levels_png_deflate_host through ctypes; the sources must come back unchanged"""
    outs = outputs_for(case)
    level_dir, summary, levels = case.level_dir.copy(), case.summary.copy(), case.levels.copy()
    lib = ro.library()
    rc = lib.ro_levels_png_deflate_host(ptr(level_dir) if case.dcap else None, case.dcap, ptr(summary),
                                        ptr(levels) if levels.size else None, levels.size, ptr(outs[0]),
                                        ptr(outs[1]) if case.png_bytes else None, case.png_bytes, ptr(outs[2]))
    assert rc == 0, lib.ro_last_error()
    assert level_dir.tobytes() == case.level_dir.tobytes() and summary.tobytes() == case.summary.tobytes()
    assert levels.tobytes() == case.levels.tobytes(), "the levels were written"
    return Result(ro, case, *outs)


def check_files(case, r, walk_them=True):
    """every WRITTEN file is the restatement's file of its level image, byte for byte, and walks; NO_ROOM entries carry the
    restatement's size"""
    for d in np.flatnonzero((r.dir["status"] == WRITTEN) | (r.dir["status"] == NO_ROOM)):
        px = G.source_pixels(case, d)
        want, _ = expected_cached(px)
        assert int(r.dir["bytes"][d]) == len(want), (d, int(r.dir["bytes"][d]), len(want))
        if r.dir["status"][d] == WRITTEN:
            assert r.file(d).tobytes() == want, d
            if walk_them:
                walk(r.file(d), px)


def host_vs_python(ro):
    def call(case):
        r = host_call(ro, case)
        check_files(case, r)
        return r
    return call


def shape_case(ro, w, h, content):
    """the image behind a one-pixel one, so that it does not start at level byte 0; the room is the stored files' bound"""
    d, levels = images(ro, [G.pixels_of("random", 1, 1), pixels_of(content, w, h)], pad=64)
    return Case(ro, d, levels, G.room_of(1, 1) + G.room_of(w, h))


# ---- the decision table: pnglib's cases speak of the stored files' sizes, so they are walked through a call that checks every
# result, and the sizes are asserted here --------------------------------------------------------------------------------------
def sized(call, case):
    """the sizing call, then the call with exactly that room: (the full result, the rooms of its writable entries)"""
    probe = call(case.with_room(0))
    need = int(probe.summary["needed_bytes"])
    assert int(probe.summary["written"]) == 0 and int(probe.summary["units_bytes"]) == 0
    full = call(case.with_room(need))
    assert int(full.summary["no_room"]) == 0 and int(full.summary["units_bytes"]) == need == int(full.summary["needed_bytes"])
    st = full.dir["status"]
    assert probe.dir["bytes"].tolist() == full.dir["bytes"].tolist()
    assert [x if x != NO_ROOM else WRITTEN for x in probe.dir["status"].tolist()] == st.tolist()
    return full, [room_of_bytes(int(b)) for b in full.dir["bytes"][st == WRITTEN]]


def case_room(ro, call):
    """room equal to the actual sum writes all; one byte short makes the last entry NO_ROOM; the prefix rule; the sizing call
    (png NULL) returns the exact needed_bytes and a second call with that room writes everything"""
    d, levels = images(ro, [pixels_of("noise", 300, 250, 1), G.small(5, 300, 2), (None, SKIPPED), pixels_of("zeros", 700, 200),
                            pixels_of("mixed", 400, 400, 2), G.small(8, 2, 1)])
    case = Case(ro, d, levels, 0)
    full, rooms = sized(call, case)
    need = sum(rooms)
    assert G.statuses(full) == [WRITTEN, WRITTEN, SKIPPED, WRITTEN, WRITTEN, WRITTEN]
    assert rooms[0] < G.room_of(300, 250) and rooms[2] < G.room_of(700, 200) // 7 and rooms[1] == G.room_of(300, 2)
    for room, written in ((need - 1, 4), (need - rooms[4], 4), (need - rooms[4] - 1, 3), (sum(rooms[:2]) + 17, 2), (rooms[0], 1),
                          (rooms[0] - 1, 0)):
        r = call(case.with_room(room))
        want = [WRITTEN if i < written else NO_ROOM for i in range(5)]
        assert G.statuses(r) == want[:2] + [SKIPPED] + want[2:], (room, G.statuses(r))
        assert int(r.summary["needed_bytes"]) == need and r.dir["naxis1"].tolist() == [300, 300, 0, 700, 400, 2]
        assert r.dir["bytes"].tolist() == full.dir["bytes"].tolist()
        assert r.png.tobytes() == full.png[:len(r.png)].tobytes()                    # a file does not depend on the room
    # the small file would fit behind the first, but the second does not: nothing behind it fits
    r = call(case.with_room(rooms[0] + rooms[4]))
    assert G.statuses(r) == [WRITTEN, NO_ROOM, SKIPPED, NO_ROOM, NO_ROOM, NO_ROOM]


TABLE = [case_room] + list(G.TABLE)
