#!/usr/bin/env python3
"""The FITS data units of include/ro_stft.h (ro_snapshot_units_host / ro_raw_units_host and the two resident calls) restated
in numpy, twice:

  units        the rules entry by entry, literally: SKIPPED / INVALID / SKIPPED (window without columns) / writable in that
               order; `offset` 2880 x the exclusive prefix sum of the writable entries' blocks, fitting or not; WRITTEN where
               offset + 2880 blocks <= units_bytes, else NO_ROOM; a unit is astype('>f4') of the cut, zero-padded to the block
  units_plan   the kernels of csrc/ro_units.hip: one workgroup walks the entries TILE at a time and carries the block prefix
               (the sums in 16-bit limbs, as the kernel makes them); the copy kernel finds each block's entry by binary search
               in the plan's table of first blocks and gathers the block's floats by row and column, indices clamped
Neither looks at the library.  tests/test_units_cpu.py holds the host twins to `units`; main() holds the two against each
other on random cases with a tile of a few entries and a block of a few floats, so that most cases cross their seams.

Run it: python tools/units/emu_units.py [cases]     (exit status 0 and a line "ok ..." when everything agrees)
"""
import sys

import numpy as np

EVENT_DTYPE = np.dtype([("fire_row", np.int64), ("start_row", np.int64), ("length", np.int64), ("noise", np.float32),
                        ("peak", np.int32), ("magnitude", np.float32), ("reserved", np.int32)])
SNAPSHOT_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_row", np.int64), ("offset", np.int64), ("rows", np.int32),
                           ("slot", np.int32), ("status", np.int32), ("reserved", np.int32)])
RAW_CAPTURE_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_sample", np.int64), ("samples", np.int64), ("offset", np.int64),
                              ("slot", np.int32), ("status", np.int32)])
FITS_UNIT_DTYPE = np.dtype([("offset", np.int64), ("bytes", np.int64), ("naxis2", np.int64), ("naxis1", np.int32),
                            ("status", np.int32)])
UNIT_SUMMARY_DTYPE = np.dtype([("entries", np.int64), ("written", np.int64), ("skipped", np.int64), ("no_room", np.int64),
                               ("invalid", np.int64), ("units_bytes", np.int64), ("needed_bytes", np.int64),
                               ("reserved", np.int64)])
CAPTURED = 0
WRITTEN, SKIPPED, NO_ROOM, INVALID = 0, 1, 2, 3
BLOCK = 2880
SLOTS = 8


def want(entry, arena_floats, cols=None, windows=None):
    """(status, naxis1, naxis2, first arena float, arena row floats) of one source entry: SKIPPED, INVALID, or WRITTEN for a
    writable one.  windows is None: a raw entry"""
    if int(entry["status"]) != CAPTURED:
        return SKIPPED, 0, 0, 0, 0
    offset = int(entry["offset"])
    if windows is None:
        n = int(entry["samples"])
        if n < 1 or offset < 0 or offset + 2 * n > arena_floats:
            return INVALID, 0, 0, 0, 0
        return WRITTEN, 2, n, offset, 2
    slot, rows = int(entry["slot"]), int(entry["rows"])
    if not 0 <= slot < SLOTS or rows < 1 or offset < 0 or offset + rows * cols > arena_floats:
        return INVALID, 0, 0, 0, 0
    first_col, win_cols = windows[slot]
    if win_cols == 0:
        return SKIPPED, 0, 0, 0, 0
    return WRITTEN, win_cols, rows, offset + first_col, cols


def blocks_of(naxis1, naxis2, block=BLOCK):
    return -(-4 * naxis1 * naxis2 // block)


def unit_of(arena, first, stride, naxis1, naxis2, block=BLOCK):
    """the bytes of one unit: the cut as big-endian floats, zeros up to the block"""
    idx = first + stride * np.arange(naxis2, dtype=np.int64)[:, None] + np.arange(naxis1, dtype=np.int64)[None, :]
    data = arena[idx].astype(">f4").tobytes()                # (a byte-order change only: NaN payloads survive)
    return np.frombuffer(data + bytes(blocks_of(naxis1, naxis2, block) * block - len(data)), np.uint8)


def units(directory, resolved, arena, units_bytes, cols=None, windows=None, block=BLOCK):
    """directory: SNAPSHOT_DTYPE (with cols and windows: eight (first_col, cols)) or RAW_CAPTURE_DTYPE [dir_capacity],
    `resolved` as the source summary holds it; arena: float32.  Returns (unit directory [n], the units' bytes in use,
    summary)."""
    n = min(max(int(resolved), 0), directory.shape[0])
    out = np.zeros(n, FITS_UNIT_DTYPE)
    sm = np.zeros(1, UNIT_SUMMARY_DTYPE)[0]
    sm["entries"] = n
    parts, first_b = [], 0
    for d in range(n):
        status, naxis1, naxis2, first, stride = want(directory[d], arena.size, cols, windows)
        if status != WRITTEN:
            out[d]["status"] = status
            sm["skipped" if status == SKIPPED else "invalid"] += 1
            continue
        blocks = blocks_of(naxis1, naxis2, block)
        fits = (first_b + blocks) * block <= units_bytes
        out[d] = (first_b * block if fits else 0, 4 * naxis1 * naxis2, naxis2, naxis1, WRITTEN if fits else NO_ROOM)
        if fits:
            parts.append(unit_of(arena, first, stride, naxis1, naxis2, block))
            sm["written"] += 1
            sm["units_bytes"] = (first_b + blocks) * block
        else:
            sm["no_room"] += 1
        first_b += blocks
    sm["needed_bytes"] = first_b * block
    return out, np.concatenate(parts) if parts else np.zeros(0, np.uint8), sm


def limb_cumsum(x):
    """an inclusive sum of 64-bit counts the way the kernel makes it: four ladders of 16 bits each, put together"""
    x = np.asarray(x, np.uint64)
    total = np.zeros(len(x), np.uint64)
    for limb in range(4):
        part = (x >> np.uint64(16 * limb)) & np.uint64(0xffff)
        total += np.cumsum(part).astype(np.uint64) << np.uint64(16 * limb)
    return total.astype(np.int64)


def units_plan(directory, resolved, arena, units_bytes, cols=None, windows=None, block=BLOCK, tile=256, waves=7):
    """the same outputs the way the kernels get them"""
    n = min(max(int(resolved), 0), directory.shape[0])
    out = np.zeros(n, FITS_UNIT_DTYPE)
    first_block, first_float = np.zeros(n, np.int64), np.zeros(n, np.int64)
    sm = np.zeros(1, UNIT_SUMMARY_DTYPE)[0]
    room = units_bytes // block
    block_base = used = 0
    stride = 2 if windows is None else cols
    # ---- units_plan_kernel
    for t0 in range(0, n, tile):
        idx = range(t0, min(t0 + tile, n))
        wants = [want(directory[c], arena.size, cols, windows) for c in idx]
        writable = np.array([w[0] == WRITTEN for w in wants])
        blocks = np.array([blocks_of(w[1], w[2], block) if w[0] == WRITTEN else 0 for w in wants], np.int64)
        first_b = block_base + limb_cumsum(blocks) - blocks
        fits = writable & (first_b + blocks <= room)
        for i, c in enumerate(idx):
            status, naxis1, naxis2, first, _ = wants[i]
            if writable[i]:
                out[c] = (first_b[i] * block if fits[i] else 0, 4 * naxis1 * naxis2, naxis2, naxis1, WRITTEN if fits[i] else NO_ROOM)
            else:
                out[c]["status"] = status
            first_block[c], first_float[c] = first_b[i], first if writable[i] else 0
        sm["written"] += int(fits.sum())
        sm["no_room"] += int((writable & ~fits).sum())
        sm["skipped"] += sum(w[0] == SKIPPED for w in wants)
        sm["invalid"] += sum(w[0] == INVALID for w in wants)
        if fits.any():
            last = int(np.flatnonzero(fits)[-1])
            used = max(used, int(first_b[last] + blocks[last]))
        block_base += int(blocks.sum())
    sm["entries"], sm["units_bytes"], sm["needed_bytes"] = n, used * block, block_base * block
    # ---- units_copy_kernel: wave w takes blocks w, w + waves, ...
    buf = np.full(used * block, 0xEE, np.uint8)
    bf = block // 4
    for w in range(waves):
        for b in range(w, used, waves):
            lo, hi = 0, n
            while lo < hi:
                mid = (lo + hi) >> 1
                if first_block[mid] <= b:
                    lo = mid + 1
                else:
                    hi = mid
            assert lo > 0
            u = out[lo - 1]
            k = b - int(first_block[lo - 1])
            floats, naxis1 = int(u["bytes"]) >> 2, int(u["naxis1"])
            i0 = k * bf
            assert u["status"] == WRITTEN and i0 < floats and int(u["offset"]) + (k + 1) * block <= units_bytes, (b, u)
            t = np.arange(bf, dtype=np.int64)
            if naxis1 == stride:
                at = int(first_float[lo - 1]) + i0 + t
            else:
                r0 = i0 // naxis1
                x = (i0 - r0 * naxis1) + t
                at = int(first_float[lo - 1]) + (r0 + x // naxis1) * stride + x % naxis1
            got = arena[np.clip(at, 0, arena.size - 1)].view(np.uint32).byteswap()
            got[t >= floats - i0] = 0
            at_byte = int(u["offset"]) + k * block
            buf[at_byte:at_byte + block] = got.view(np.uint8)
    return out, buf, sm


def random_case(rng, block=BLOCK):
    """arguments of one call, images or raw: entries of every status around an arena with odd bit patterns in it"""
    raw = bool(rng.integers(0, 2))
    cols = 2 if raw else int(rng.choice([1, 3, 8, 17, 65]))
    arena = rng.integers(0, 2 ** 32, int(rng.choice([0, 1, 40, 700, 5000])), dtype=np.uint64).astype(np.uint32).view(np.float32)
    dcap = int(rng.integers(0, 31))
    d = np.zeros(dcap, RAW_CAPTURE_DTYPE if raw else SNAPSHOT_DTYPE)
    d["status"] = rng.choice([0, 0, 0, 0, 1, 2], dcap)
    d["slot"] = np.where(rng.random(dcap) < 0.07, rng.choice([-1, 8, 100], dcap), rng.integers(0, SLOTS, dcap))
    size = np.where(rng.random(dcap) < 0.07, rng.choice([0, -2], dcap), rng.integers(1, max(arena.size // (3 * cols), 2), dcap))
    d["samples" if raw else "rows"] = size
    d["offset"] = np.where(rng.random(dcap) < 0.07, rng.choice([-1, arena.size, arena.size - 1], dcap),
                           rng.integers(0, max(arena.size - arena.size // 3, 1), dcap))
    d["event"]["peak"] = np.arange(dcap)
    windows = None
    if not raw:
        windows = []
        for _ in range(SLOTS):
            w = int(rng.integers(0, cols + 1)) if rng.random() < 0.85 else 0
            windows.append((int(rng.integers(0, cols - w + 1)), w))
    resolved = int(rng.integers(-1, dcap + 4))
    need = int(units(d, resolved, arena, 1 << 40, cols, windows, block)[2]["needed_bytes"])
    units_bytes = int(rng.choice([0, need, max(need - 1, 0), need // 2, need + 77, block]))
    return dict(directory=d, resolved=resolved, arena=arena, units_bytes=units_bytes, cols=None if raw else cols, windows=windows)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main(cases=200):
    rng = np.random.default_rng(22)
    seen = np.zeros(4, np.int64)
    for case in range(cases):
        block = int(rng.choice([4, 20, BLOCK]))
        args = random_case(rng, block)
        d1, u1, s1 = units(block=block, **args)
        d2, u2, s2 = units_plan(block=block, tile=int(rng.choice([3, 5, 64])), waves=int(rng.choice([1, 7])), **args)
        if not (same(d1, d2) and same(u1, u2) and s1 == s2):
            print("case %d: the plan and the rules disagree\n%s\n%s\n%s\n%s" % (case, s1, s2, d1, d2))
            return 1
        seen += (int(s1["written"]), int(s1["skipped"]), int(s1["no_room"]), int(s1["invalid"]))
    if not seen.all():
        print("the cases leave an outcome out: written, skipped, no room, invalid = %s" % seen.tolist())
        return 1
    print("ok: %d cases; written %d, skipped %d, no room %d, invalid %d" % ((cases,) + tuple(seen.tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 200))
