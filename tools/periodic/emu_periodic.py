#!/usr/bin/env python3
"""The periodic snapshots of include/ro_stft.h (ro_periodic_plan, ro_periodic_units_host and the resident call) restated in
numpy.  Nothing here looks at the library.

  replay       the cadence, ROW BY ROW: SnapshotRecorder::update / startWriting / stop (src/WaterfallBackend.cpp:415-427,
               :107-127, :400-403) with mark = row + 1 on an unwrapped ring -- not the closed form of the header, so that the
               closed form is checked against the machine.  One deviation, the header's: stop() with nothing behind the
               last snapshot queues nothing
  plan         the rules candidate by candidate over what `replay` queued: LOST / writable in that order, `offset` 2880 x
               the exclusive prefix sum of the writable candidates' blocks, WRITTEN where it fits, else NO_ROOM; next_index
               past each recorder's leading resolved entries; candidates beyond `capacity` only counted
  units        a written unit is the big-endian bit copy of ring rows (first_row + r) % ring_rows, cut to the window,
               zero-padded to the block
  units_blocks the kernel of csrc/ro_periodic.hip: block b of the units is work item b; its recorder's run, the unit and the
               unit's first row come from a few scalars per recorder; one modulo per block, a lane's slot wrapped once, the
               index clamped into the ring
tests/test_periodic_cpu.py holds the library to `replay`, `plan` and `units`; main() holds `units_blocks` against `units` on
random cases with a block of a few floats, so that most cases cross a block's and the ring's seams.

Run it: python tools/periodic/emu_periodic.py [cases]     (exit status 0 and a line "ok ..." when everything agrees)
"""
import sys

import numpy as np

PERIODIC_ENTRY_DTYPE = np.dtype([("index", np.int64), ("first_row", np.int64), ("due_row", np.int64), ("offset", np.int64),
                                 ("bytes", np.int64), ("rows", np.int32), ("naxis1", np.int32), ("recorder", np.int32),
                                 ("status", np.int32)])
PERIODIC_SUMMARY_DTYPE = np.dtype([("entries", np.int64), ("written", np.int64), ("lost", np.int64), ("no_room", np.int64),
                                   ("unlisted", np.int64), ("units_bytes", np.int64), ("needed_bytes", np.int64),
                                   ("reserved", np.int64)])
WRITTEN, LOST, NO_ROOM = 0, 1, 2
BLOCK = 2880


class Recorder:
    """the cadence's state of one SnapshotRecorder: nextSnapshot_.start, the ring's mark, what has been queued"""

    def __init__(self, snapshot_rows):
        self.snapshot_rows, self.start, self.mark, self.queued = snapshot_rows, 0, 0, []

    def start_writing(self, due_row):                          # :107-127
        length = self.mark - self.start                        # :112-113: length == 0 -> buffer_->size(start)
        if self.snapshot_rows < length:                        # :114-115
            length = self.snapshot_rows
        self.queued.append((self.start, length, due_row))      # :121
        self.start += length                                   # :122-123

    def row(self):
        """one row arrives: processFFT pushes it (the mark is the row + 1), then update() runs (:415-427)"""
        row = self.mark
        self.mark = row + 1
        if self.mark - self.start >= self.snapshot_rows + 2:   # :417
            self.start_writing(row)

    def stop(self):                                            # :400-403, writeUnfinished_
        if self.mark - self.start > 0:                         # (the deviation: the reference's size() of an empty range is
            self.start_writing(self.mark - 1)                  #  the ring's capacity, and it would queue S stale rows)


def replay(snapshot_rows, head_row, final):
    """[(first_row, rows, due_row), ...] of one recorder after head_row rows, and stop() with `final`"""
    rec = Recorder(snapshot_rows)
    for _ in range(head_row):
        rec.row()
    if final:
        rec.stop()
    return rec.queued


def blocks_of(naxis1, rows, block=BLOCK):
    return -(-4 * naxis1 * rows // block)


def plan(recorders, next_index, head_row, final, ring_rows, units_bytes, capacity, block=BLOCK):
    """recorders: [(snapshot_rows, first_col, cols), ...]; next_index: a list, updated in place.  Returns (directory, summary)"""
    out = np.zeros(0, PERIODIC_ENTRY_DTYPE)
    entries = []
    sm = np.zeros(1, PERIODIC_SUMMARY_DTYPE)[0]
    room = units_bytes // block
    first_b = 0
    for i, (snapshot_rows, _, naxis1) in enumerate(recorders):
        queued = replay(snapshot_rows, head_row, final)
        leading = True
        for k in range(int(next_index[i]), len(queued)):
            if len(entries) >= capacity:
                sm["unlisted"] += 1
                continue
            first_row, rows, due_row = queued[k]
            assert first_row == k * snapshot_rows
            e = np.zeros(1, PERIODIC_ENTRY_DTYPE)[0]
            e["index"], e["first_row"], e["due_row"], e["rows"], e["naxis1"], e["recorder"] = k, first_row, due_row, rows, naxis1, i
            if first_row < head_row - ring_rows:
                e["status"] = LOST
                sm["lost"] += 1
            else:
                blocks = blocks_of(naxis1, rows, block)
                e["bytes"] = 4 * naxis1 * rows
                if first_b + blocks <= room:
                    e["status"], e["offset"] = WRITTEN, first_b * block
                    sm["written"] += 1
                    sm["units_bytes"] = (first_b + blocks) * block
                else:
                    e["status"] = NO_ROOM
                    sm["no_room"] += 1
                    leading = False
                first_b += blocks
            if leading:
                next_index[i] = k + 1
            entries.append(e)
    sm["entries"] = len(entries)
    sm["needed_bytes"] = first_b * block
    if entries:
        out = np.array(entries, PERIODIC_ENTRY_DTYPE)
    return out, sm


def units(ring, cols, recorders, directory, units_bytes, block=BLOCK):
    """ring: float32 [ring_rows, stride].  Returns the bytes of the units in use"""
    buf = np.zeros(units_bytes, np.uint8)
    used = 0
    for e in directory:
        if e["status"] != WRITTEN:
            continue
        _, first_col, naxis1 = recorders[int(e["recorder"])]
        assert first_col + naxis1 <= cols
        slots = (int(e["first_row"]) + np.arange(int(e["rows"]), dtype=np.int64)) % ring.shape[0]
        data = np.ascontiguousarray(ring[slots, first_col:first_col + naxis1]).view(np.uint32).byteswap().view(np.uint8).reshape(-1)
        at = int(e["offset"])
        used = at + blocks_of(naxis1, int(e["rows"]), block) * block
        assert at % block == 0 and used <= units_bytes and data.size == int(e["bytes"])
        buf[at:at + data.size] = data
    return buf[:used]


def runs_of(recorders, directory, block=BLOCK):
    """the scalars the kernel gets: per recorder (row0, block0, units, unit_blocks, S, last_rows, first_col, naxis1), and the
    blocks of all of them"""
    runs = [None] * len(recorders)
    end = 0
    for e in directory:
        if e["status"] != WRITTEN:
            continue
        i = int(e["recorder"])
        snapshot_rows, first_col, naxis1 = recorders[i]
        assert int(e["offset"]) == end * block
        if runs[i] is None:
            runs[i] = [int(e["first_row"]), end, 0, blocks_of(naxis1, snapshot_rows, block), snapshot_rows, 0, first_col, naxis1]
        runs[i][2] += 1
        runs[i][5] = int(e["rows"])
        end += blocks_of(naxis1, int(e["rows"]), block)
    return runs, end


def units_blocks(ring, cols, recorders, directory, units_bytes, block=BLOCK, waves=7):
    runs, total = runs_of(recorders, directory, block)
    bf = block // 4
    ring_rows, stride = ring.shape
    flat = ring.reshape(-1).view(np.uint32)
    last = (ring_rows - 1) * stride + cols - 1
    buf = np.zeros(units_bytes, np.uint8)
    assert total * block <= units_bytes
    for me in range(waves):
        for b in range(me, total, waves):
            run = None
            for r in runs:
                if r is not None and r[2] > 0 and r[1] <= b:
                    run = r
            row0, block0, n, unit_blocks, snapshot_rows, last_rows, first_col, naxis1 = run
            j, k = divmod(b - block0, unit_blocks)
            assert j < n
            rows = last_rows if j == n - 1 else snapshot_rows
            floats, i0 = rows * naxis1, k * bf
            assert i0 < floats
            r0 = i0 // naxis1
            slot0 = (row0 + j * snapshot_rows + r0) % ring_rows
            t = np.arange(bf, dtype=np.int64)
            x = (i0 - r0 * naxis1) + t
            dr = x // naxis1
            slot = slot0 + dr
            slot = np.where(slot >= ring_rows, slot - ring_rows, slot)
            at = np.clip(slot * stride + first_col + (x - dr * naxis1), 0, last)
            got = flat[at].byteswap()
            got[t >= floats - i0] = 0
            buf[b * block:(b + 1) * block] = got.view(np.uint8)
    return buf[:total * block]


def random_case(rng, block=BLOCK):
    """arguments of one plan and its units: 1 ... 8 recorders with overlapping windows around a ring with odd bit patterns in
    it, at a head row some of whose snapshots an earlier plan has resolved already"""
    count = int(rng.choice([1, 1, 2, 3, 8]))
    cols = int(rng.choice([1, 3, 8, 17, 65, 200]))
    stride = cols + int(rng.choice([0, 3]))
    recorders = []
    for _ in range(count):
        w = int(rng.integers(1, cols + 1))
        recorders.append((int(rng.choice([1, 2, 3, 7, 20])), int(rng.integers(0, cols - w + 1)), w))
    smax = max(r[0] for r in recorders)
    ring_rows = int(rng.choice([smax + 2, 2 * smax + 3, 23, max(smax - 1, 1), smax + 1]))
    ring = rng.integers(0, 2 ** 32, (ring_rows, stride), dtype=np.uint64).astype(np.uint32).view(np.float32)
    head_row = int(rng.integers(0, 5 * smax + 4))
    next_index = [0] * count
    if rng.random() < 0.6:                                     # an earlier call, with room for everything
        plan(recorders, next_index, int(rng.integers(0, head_row + 1)), False, ring_rows, 1 << 40, 1 << 20, block)
    final = bool(rng.integers(0, 2))
    capacity = int(rng.choice([0, 1, 3, 64, 64, 64]))
    need = int(plan(recorders, list(next_index), head_row, final, ring_rows, 1 << 40, capacity, block)[1]["needed_bytes"])
    units_bytes = int(rng.choice([0, need, need, max(need - 1, 0), need // 2, need + 77, block]))
    return dict(recorders=recorders, next_index=next_index, head_row=head_row, final=final, ring=ring, cols=cols,
                units_bytes=units_bytes, capacity=capacity)


def main(cases=200):
    rng = np.random.default_rng(23)
    seen = np.zeros(4, np.int64)
    for case in range(cases):
        block = int(rng.choice([4, 20, BLOCK]))
        args = random_case(rng, block)
        d, sm = plan(args["recorders"], list(args["next_index"]), args["head_row"], args["final"], args["ring"].shape[0],
                     args["units_bytes"], args["capacity"], block)
        u1 = units(args["ring"], args["cols"], args["recorders"], d, args["units_bytes"], block)
        u2 = units_blocks(args["ring"], args["cols"], args["recorders"], d, args["units_bytes"], block, waves=int(rng.choice([1, 7])))
        if u1.tobytes() != u2.tobytes() or len(u1) != int(sm["units_bytes"]):
            print("case %d: the kernel's walk and the rules disagree\n%s\n%s" % (case, sm, d))
            return 1
        seen += (int(sm["written"]), int(sm["lost"]), int(sm["no_room"]), int(sm["unlisted"]))
    if not seen.all():
        print("the cases leave an outcome out: written, lost, no room, unlisted = %s" % seen.tolist())
        return 1
    print("ok: %d cases; written %d, lost %d, no room %d, unlisted %d" % ((cases,) + tuple(seen.tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 200))
