#!/usr/bin/env python3
"""The detector kernels of csrc/ro_events.hip restated in numpy, and checked against a line-by-line transcription of
BolidRecorder::update's state machine (src/BolidRecorder.cpp:171-267) before the kernels ever meet a device.

Three machines over the same decisions:
  fsm_reference   the transcription: STATE_INIT / STATE_BOLID / STATE_BOLID_ENDED, duration_, nextSnapshot_, with
                  mark = row + 1 (buffer_->mark(), unwrapped)
  events_closed   the closed form of include/ro_stft.h one row at a time -- what ro_events_host does
  events_tiles    the kernels: leaf, (+), the DPP ladder of a wave, the workgroup scan, and the three passes per chunk
                  (reduce a tile, scan the tiles from the carried state, emit from the tile's prefix), with the very
                  integer conventions of the kernels: summaries counted from 1 inside a tile or a chunk, (0, 0, 0) = empty
The tile and chunk sizes are parameters here, so that a few hundred rows cross many seams; the wave stays 64 lanes.

Run it: python tools/events/emu_events.py [cases]     (exit status 0 and a line "ok ..." when everything agrees)
"""
import sys

import numpy as np

EMPTY = (0, 0, 0)
PER = 4                                                  # tiles per lane of pass 2, at most


# ---- the transcription ---------------------------------------------------------------------------------------------
class FsmReference:
    INIT, BOLID, ENDED = 0, 1, 2

    def __init__(self, advance, jitter):
        self.advance, self.jitter = advance, jitter
        self.state, self.duration, self.start, self.length, self.rec = self.INIT, 0, 0, 0, None

    def update(self, row, detect, rec):
        """one BolidRecorder::update; returns the event (fire_row, start, length, rec) or None"""
        mark = row + 1
        if self.state == self.INIT:                      # :172-183
            if detect:
                self.rec = rec
                self.duration = 1
                self.start = mark - self.advance
                self.length = 2 * self.advance
                self.state = self.BOLID
        elif self.state == self.BOLID:                   # :185-193
            if detect:
                self.duration += 1
            else:
                self.length += self.duration
                self.duration = 1
                self.state = self.ENDED
        else:                                            # :195-267
            self.duration += 1
            if detect:
                self.state = self.BOLID
            elif self.duration >= self.jitter:
                self.state = self.INIT
                return (row, self.start, self.length, self.rec)
        return None


def fsm_reference(detect, recs, first_row, advance, jitter, fsm=None):
    fsm = fsm or FsmReference(advance, jitter)
    out = []
    for i, d in enumerate(detect):
        e = fsm.update(first_row + i, bool(d), recs[i])
        if e:
            out.append(e)
    return out, fsm


# ---- the closed form, one row at a time (ro_events_host) --------------------------------------------------------------
def new_state():
    return dict(open=0, first=0, last=0, rec=0)


def events_closed(detect, recs, first_row, advance, jitter, state):
    G = max(2, jitter)
    st = dict(state)
    out = []
    if len(detect) == 0:
        return out, st
    if st["open"] and st["last"] + G < first_row:
        st["open"] = 0
    for i, d in enumerate(detect):
        r = first_row + i
        if d:
            if not st["open"]:
                st.update(open=1, first=r, rec=recs[i])
            st["last"] = r
        elif st["open"] and r == st["last"] + G:
            out.append((r, st["first"] + 1 - advance, 2 * advance + st["last"] - st["first"] + 1, st["rec"]))
            st["open"] = 0
    if not st["open"]:
        st = new_state()
    return out, st


# ---- the kernels ---------------------------------------------------------------------------------------------------
def combine(a, b, G):
    if b[1] == 0:
        return a
    if a[1] == 0:
        return b
    gstart = b[2] if b[2] != b[0] else (b[0] if b[0] - a[1] - 1 >= G else a[2])
    return (a[0], b[1], gstart)


def wave_inclusive(v, G):
    """the DPP ladder over 64 lanes: row_shr 1, 2, 4, 8 inside rows of 16 lanes (a lane without a source reads EMPTY),
    row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3"""
    assert len(v) == 64
    for n in (1, 2, 4, 8):
        v = [combine(v[i - n] if i % 16 >= n else EMPTY, v[i], G) for i in range(64)]
    v = [combine(v[(i // 16) * 16 - 1] if (i // 16) in (1, 3) else EMPTY, v[i], G) for i in range(64)]
    v = [combine(v[31] if i >= 32 else EMPTY, v[i], G) for i in range(64)]
    return v


def block_exclusive(v, G):
    """exclusive (+) prefix over the workgroup's lanes (whole waves of 64) and their total"""
    assert len(v) % 64 == 0
    waves = [wave_inclusive(v[w:w + 64], G) for w in range(0, len(v), 64)]
    out, pre = [], EMPTY
    for inc in waves:
        out += [combine(pre, x, G) for x in [EMPTY] + inc[:-1]]
        pre = combine(pre, inc[63], G)
    return out, pre


def with_front(a, b, base, G):
    """A (+) B, A = (open, last, gstart) in stream rows, B counted from 1 at stream row `base`"""
    if b[1] == 0:
        return a
    bf, bl, bg = base + b[0] - 1, base + b[1] - 1, base + b[2] - 1
    if not a[0] or b[2] != b[0]:
        return (1, bl, bg)
    return (1, bl, bf if bf - a[1] - 1 >= G else a[2])


def leaves(detect, tile, T):
    d = list(detect[tile * T:(tile + 1) * T])
    d += [0] * (T - len(d))
    return d, [(i + 1, i + 1, i + 1) if x else EMPTY for i, x in enumerate(d)]


def chunk_tiles(detect, recs, first_row, advance, jitter, state, T, events_before):
    """the three launches of one chunk; returns (events with their index in the call, new state)"""
    G = max(2, jitter)
    rows = len(detect)
    tiles = (rows + T - 1) // T
    end = first_row + rows
    # pass 1
    totals = []
    for t in range(tiles):
        d, leaf = leaves(detect, t, T)
        before, total = block_exclusive(leaf, G)
        fires = sum(1 for i in range(T) if t * T + i < rows and not d[i] and before[i][1] and (i + 1) - before[i][1] == G)
        totals.append((tuple(x + t * T if total[1] else 0 for x in total), fires))
    # pass 2: `lanes` lanes, `per` consecutive tiles each
    lanes = 64
    per = (tiles + lanes - 1) // lanes
    carry = (1 if state["open"] and state["last"] + G >= first_row else 0, state["last"], state["first"])
    assert per <= PER
    # (the kernel's loops run over all PER places of a lane; the places k >= per belong to the next lane's tiles)
    mine = lambda lane, k: k < per and lane * per + k < tiles
    ex, acc_l = [[EMPTY] * PER for _ in range(lanes)], []
    for lane in range(lanes):
        acc = EMPTY
        for k in range(PER):
            ex[lane][k] = acc
            acc = combine(acc, totals[lane * per + k][0] if mine(lane, k) else EMPTY, G)
        acc_l.append(acc)
    front, chunk_total = block_exclusive(acc_l, G)
    prefix, fires_before = [None] * tiles, events_before
    for lane in range(lanes):
        for k in range(PER):
            tile = lane * per + k
            p = with_front(carry, combine(front[lane], ex[lane][k], G), first_row, G)
            t0 = first_row + tile * T
            t1 = min(t0 + T, end)
            f = p[1] + G
            tot, fires = totals[tile] if mine(lane, k) else (EMPTY, 0)
            across = mine(lane, k) and p[0] and t0 <= f < t1 and (tot[1] == 0 or f < first_row + tot[0] - 1)
            if mine(lane, k):
                prefix[tile] = (p, fires_before)
            fires_before += fires + (1 if across else 0)
    allp = with_front(carry, chunk_total, first_row, G)
    ns = new_state()
    if allp[0] and allp[1] + G >= end:
        rec = recs[allp[2] - first_row] if allp[2] >= first_row else state["rec"]
        ns = dict(open=1, first=allp[2], last=allp[1], rec=rec)
    # pass 3
    out = []
    for t in range(tiles):
        d, leaf = leaves(detect, t, T)
        before, _ = block_exclusive(leaf, G)
        front_t, at = prefix[t]
        for i in range(T):
            row = first_row + t * T + i
            p = with_front(front_t, before[i], first_row + t * T, G)
            if t * T + i < rows and not d[i] and p[0] and row == p[1] + G:
                rec = recs[p[2] - first_row] if p[2] >= first_row else state["rec"]
                out.append((at, (row, p[2] + 1 - advance, 2 * advance + p[1] - p[2] + 1, rec)))
                at += 1
    assert fires_before - events_before == len(out), "pass 2 counted %d fires, pass 3 wrote %d" % (
        fires_before - events_before, len(out))
    return out, ns


def events_tiles(detect, recs, first_row, advance, jitter, state, T=64, chunk=256):
    st, out = dict(state), []
    for done in range(0, len(detect), chunk):
        ev, st = chunk_tiles(detect[done:done + chunk], recs[done:done + chunk], first_row + done, advance, jitter, st, T,
                             len(out))
        for k, (at, e) in enumerate(ev):
            assert at == len(out), "event index %d, expected %d" % (at, len(out))
            out.append(e)
    return out, st


# ---- the comparison ------------------------------------------------------------------------------------------------
def random_decisions(rng, rows):
    """bursts and gaps of lengths drawn around the jitter values in use, so that gaps of G - 1 and G both come up"""
    d = np.zeros(rows, np.uint8)
    pos = int(rng.integers(0, 6))
    while pos < rows:
        n = int(rng.choice([1, 1, 2, 3, 7, 40]))
        d[pos:pos + n] = 1
        pos += n + int(rng.choice([1, 1, 2, 2, 3, 4, 5, 28, 29, 30, 70, 200]))
    return d


def check_case(rng, rows, advance, jitter, T, chunk, first_row):
    d = random_decisions(rng, rows)
    recs = list(range(1000, 1000 + rows))                # the "record" of a row: a number that names it
    want, fsm = fsm_reference(d, recs, first_row, advance, jitter)
    cuts = sorted(int(c) for c in rng.integers(0, rows + 1, 2))
    for name, machine in (("closed", events_closed), ("tiles", lambda *a: events_tiles(*a, T=T, chunk=chunk))):
        one, st1 = machine(d, recs, first_row, advance, jitter, new_state())
        assert one == want, (name, rows, advance, jitter, T, chunk)
        assert bool(st1["open"]) == (fsm.state != FsmReference.INIT), (name, "state")
        got, st = [], new_state()
        for lo, hi in zip([0] + cuts, cuts + [rows]):
            ev, st = machine(d[lo:hi], recs[lo:hi], first_row + lo, advance, jitter, st)
            got += ev
        assert got == want and st == st1, (name, "three calls", rows, cuts)
    a, sa = events_closed(d, recs, first_row, advance, jitter, new_state())
    b, sb = events_tiles(d, recs, first_row, advance, jitter, new_state(), T=T, chunk=chunk)
    assert sa == sb
    return len(want)


def main(cases=60):
    rng = np.random.default_rng(20261019)
    # (+) is associative on summaries that can occur: the ladder of a wave equals the serial fold
    for _ in range(200):
        G = int(rng.choice([2, 3, 5, 29]))
        d = rng.random(64) < rng.choice([0.03, 0.2, 0.7])
        leaf = [(i + 1, i + 1, i + 1) if x else EMPTY for i, x in enumerate(d)]
        inc, acc = wave_inclusive(leaf, G), EMPTY
        for i in range(64):
            acc = combine(acc, leaf[i], G)
            assert inc[i] == acc, (G, i)
    events = 0
    for case in range(cases):
        rows = int(rng.choice([1, 2, 63, 64, 65, 197, 256, 257, 700, 1500]))
        advance = int(rng.choice([0, 3, 11]))
        jitter = int(rng.choice([0, 1, 2, 3, 29, 2 * 64 + 7]))
        T, chunk = (64, 256) if case % 3 else (128, 512)
        first_row = int(rng.choice([0, 5, 2 ** 33]))
        events += check_case(rng, rows, advance, jitter, T, chunk, first_row)
    print("ok: %d cases, %d events; transcription == closed form == tiles, in one call and in three" % (cases, events))
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 60))
