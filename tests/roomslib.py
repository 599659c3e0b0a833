"""Rooms that are no multiple of the block: more rows of the units' and the levels' decision tables (unitslib.case_room,
levelslib.case_room), written against the same `call` so that the host twins and the device walk the very same lines.
The host twins place an entry by a rule in bytes, first + room <= buf_bytes; the device plans count whole blocks of the
buffer.  The two can part only where the buffer's bytes are no multiple of the block, so those rooms are here: one byte
less than the need, a block less one byte more than the need, and less than one block with one writable entry.  What is
expected is include/ro_stft.h's rule said in Python, and every result goes through the libs' own checks (offsets, used
and needed bytes, guards) on the way."""
import numpy as np

import levelslib as L
import unitslib as U

COLS = 200
ITEMS = [(3, 0), (8, 1), (4, 2, U.EMPTY), (1, 0), (9, 1), (1, 3), (2, 0)]      # blocks 1, 3, -, 1, 3, -, 1


def expected(blocks, block, room):
    """statuses of writable entries of `blocks` blocks each in a buffer of `room` bytes: an entry is written when the blocks
    up to and including its own fit, and nothing behind the first that does not fit is written"""
    out, first = [], 0
    for b in blocks:
        out.append(U.WRITTEN if (first + b) * block <= room else U.NO_ROOM)
        first += b
    return out


def walk_rooms(call, case, block, statuses):
    blocks = [1, 3, 1, 3, 1]
    need = sum(blocks) * block
    for room in (need + block - 1, need - 1, need - block + 1, block - 1, 2 * block - 1):
        r = call(case.with_room(room))
        want = expected(blocks, block, room)
        assert statuses(r) == want[:2] + [U.SKIPPED] + want[2:4] + [U.INVALID] + want[4:], (room, statuses(r))
        used = block * sum(b for b, s in zip(blocks, want) if s == U.WRITTEN)
        assert int(r.summary["needed_bytes"]) == need and int(r.summary["units_bytes"]) == used, (room, r.summary)


def walk_one(call, one, block, statuses):
    for room in (block - 1, block, 2 * block - 1):
        r = call(one.with_room(room))
        want = expected([1], block, room)
        assert statuses(r) == want and int(r.summary["needed_bytes"]) == block, (room, statuses(r))
        assert int(r.summary["units_bytes"]) == (block if want == [U.WRITTEN] else 0)


def units_case_rooms_off_the_block(ro, call):
    d, floats = U.images(ro, ITEMS, COLS)
    d["rows"][5] = -1
    walk_rooms(call, U.Case(ro, "image", d, floats, 0, COLS, U.whole(COLS)), U.BLOCK, U.statuses)
    d, floats = U.images(ro, [(3, 0)], COLS)
    walk_one(call, U.Case(ro, "image", d, floats, 0, COLS, U.whole(COLS)), U.BLOCK, U.statuses)
    d, floats = U.runs(ro, [300])                                                   # 2400 bytes: one block
    walk_one(call, U.Case(ro, "raw", d, floats, 0), U.BLOCK, U.statuses)


def levels_case_rooms_off_the_block(ro, call):
    d, floats = U.images(ro, ITEMS, COLS)
    d["rows"][5] = -1
    arena = L.magnitudes(np.random.default_rng(4), floats)
    walk_rooms(call, U.Case(ro, "image", d, arena, 0, COLS, U.whole(COLS)), L.LBLOCK, L.statuses)
    d, floats = U.images(ro, [(3, 0)], COLS)
    walk_one(call, U.Case(ro, "image", d, L.magnitudes(np.random.default_rng(5), floats), 0, COLS, U.whole(COLS)), L.LBLOCK, L.statuses)
