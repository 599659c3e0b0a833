#!/usr/bin/env python3
"""What it costs to get the grey-level preview of a chunk's periodic snapshots to the host: ro_stft_periodic_levels_resident
(csrc/ro_levels.hip), three launches from the ring's slots to one byte per pixel, against the two routes a resident host had
before it.

One step is one chunk: the ring (synthetic positive rows; no transform runs here) is taken to hold the stream up to the
chunk's end, and every snapshot that has become due in the chunk ends as its padded uint8 ln image in pinned host memory.
Legs:
  new the plan (host arithmetic), the three launches, the levels in use to pinned host memory, synchronise
  a   the ring's rows of the due snapshots to a pinned host ring (one copy, two where they wrap), synchronise; then
      ro_periodic_levels_host over it (two logf per pixel, one host thread)
  b   the old route: a device-to-device un-wrap of those rows into a packed image, then per image a keys reset and
      ro_stft_ln_tile_resident over its rectangle (two memsets and two launches each: four operations per image, where
      the expectation below, kept as it was written, counted three), the levels to pinned host memory, synchronise
a and b are wall-clock times of the host thread from the first call to the end of the last wait or conversion, as new is;
`device` is the time between two events around the device work of new and of b alone (no download), 20 chunks enqueued back
to back by this Python thread: where the host enqueues more slowly than the device runs -- a plan, the marshalling and three
launches per chunk for new, some 46 calls of four operations each for b -- the figure is the host's enqueue rate, so it is
an UPPER BOUND of the device time, and b's is launch- and enqueue-bound.  Shapes: the headline (32768 bins, 75 % overlap,
48 kHz: S = 352, a 615-column window, chunks of 16384 rows) and
Bolidozor.json's (65536 bins, overlap 49152, 96 kHz: S = 352, the 26200 ... 26800 Hz window, chunks of 4096 rows).
`--repeats` alternations of the legs, each a window of at least `--window` seconds over consecutive chunks of the stream,
after one pass of every leg that also checks them against one another: new and b give the same bytes, a differs from them
by at most one level in few pixels (two logf).  The report goes to stdout and to `--out`.

    python tools/levels/bench_levels.py [--window 0.5] [--repeats 5] [--out profiles/levels.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK, LBLOCK = 2880, 720
PACKED_STRIDE = 1024                                         # leg b's packed image and its handle's bins
SHAPES = [  # name, sample rate, bins, overlap, snapshot_length, (low, high) Hz or None for `cols`, cols, chunk rows
    ("headline: 32768 bins, 75 % overlap, 615-column window, chunks of 16384 rows", 48000, 32768, 24576, 60, None, 615, 16384),
    ("Bolidozor.json: 65536 bins, overlap 49152, 26200 ... 26800 Hz, chunks of 4096 rows", 96000, 65536, 49152, 60,
     (26200.0, 26800.0), None, 4096),
]

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Nobody has measured any of the legs.  At the headline shape a chunk of 16384 rows makes 46 or 47 snapshots of 352 rows x 615
columns due: 10 M pixels, 40 MB of ring floats, 10 MB of levels.  The new call reads every ring float twice (reduce, store)
and writes a byte per pixel: 90 MB of HBM traffic and two logf per pixel, some tens of microseconds on the device in three
launches.  What the host then waits for is the download of 10 MB, a quarter of the units' 40 MB that
profiles/periodic_units.txt has at about 0.75 ms: 0.2 to 0.3 ms per chunk in all.  Route b makes the same passes over the same
floats, but as 46 x 3 operations (a memset and two launches per image, each image a fraction of the device) behind an
un-wrap copy: launch-bound, 5 to 10 us per operation, 0.7 to 1.5 ms per chunk on the device -- 10 x or more behind the new
call there, 3 to 5 x behind in wall-clock rows/s with the same download at the end.  Route a downloads the 40 MB of floats
(0.75 ms) and then takes two logf of every pixel on one host thread, 10 to 20 ns each: 0.2 to 0.4 s per chunk, several
hundred times behind.  Bolidozor's chunk is a quarter of the rows and two thirds of the columns, 11 or 12 snapshots and
1.7 M pixels: the same order, with b's per-image cost a larger share and the fixed costs of new (three launches, a wait)
showing.  Nothing is gated on these numbers.
"""


NOTES = """\
Reading the device lines: they are upper bounds of device time.  The 20 chunks between the two events are enqueued by one
Python thread (per chunk: new a plan, the marshalling and three launches; b some 46 calls of two memsets and two launches
each -- four operations per image, not the three the expectation counted); where that is slower than the device, the figure
is the enqueue rate.  b's figure is launch- and enqueue-bound throughout, and so is new's at Bolidozor's shape (about 20 us
for a plan and three launches).
"""


def window(fn, seconds):
    """fn() back to back for at least `seconds` of wall clock: seconds per call"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        t = time.perf_counter() - t0
        if t >= seconds and n >= 3:
            return t / n


def padded(nbytes, block):
    return -(-nbytes // block) * block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def pinned(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()

    say(EXPECTATION)
    say("Measured (%s, %d alternations, windows of >= %.1f s)" % (torch.cuda.get_device_name(0), args.repeats, args.window))
    say("=" * 100)
    stream = torch.cuda.current_stream().cuda_stream
    with ro.Stft(bins=256, overlap=0) as st, ro.Stft(bins=PACKED_STRIDE, overlap=0) as old:
        for name, rate, bins, overlap, length, band, cols, chunk in SHAPES:
            S = ro.snapshot_rows(rate, bins, overlap, length)
            if band is not None:
                cols = ro.frequency_to_bin(bins, rate, band[1]) - ro.frequency_to_bin(bins, rate, band[0])
            assert cols <= PACKED_STRIDE
            recorders = [(S, 0, cols)]
            ring_rows = chunk + S + 2 + 158                  # at least S + 2 rows more than a chunk
            most = chunk // S + 2                            # snapshots a chunk can make due
            unit, image = padded(4 * S * cols, BLOCK), padded(S * cols, LBLOCK)
            room = most * unit                               # of the units the plan is made for; the levels take a quarter
            d_ring = torch.rand((ring_rows, cols), dtype=torch.float32, device="cuda") * 100.0 + 1e-3
            ring = ro.capi.RowRing(d_ring.data_ptr(), cols, ring_rows, cols, 0)
            d_levels = torch.zeros(room // 4, dtype=torch.uint8, device="cuda")
            d_ranges = torch.zeros(most * 2, dtype=torch.float32, device="cuda")
            h_levels = pinned(room // 4)
            h_ring = pinned(4 * ring_rows * cols)            # leg a: the rows where the ring has them
            host_ring = h_ring.numpy().view(np.float32).reshape(ring_rows, cols)
            d_packed = torch.zeros((most * S, PACKED_STRIDE), dtype=torch.float32, device="cuda")      # leg b
            state = {"new": [np.zeros(1, np.int64), 0], "a": [np.zeros(1, np.int64), 0], "b": [0, 0]}
            last = {}

            def plan(leg):
                nxt, head = state[leg]
                head += chunk
                state[leg][1] = head
                return ro.periodic_plan(recorders, nxt, head, False, ring_rows, cols, room, most)

            def slots(k0, k1):
                """rows [k0 S, k1 S) as one or two runs of ring slots: [(slot, rows), ...]"""
                first, n = (k0 * S) % ring_rows, (k1 - k0) * S
                return [(first, n)] if first + n <= ring_rows else [(first, ring_rows - first), (0, n - (ring_rows - first))]

            def leg_new(device_only=False):
                directory, sm = plan("new")
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                if device_only:
                    return 0
                used = int(sm["units_bytes"]) // 4
                h_levels[:used].copy_(d_levels[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            def leg_a():
                directory, sm = plan("a")
                if len(directory):
                    k0, k1 = int(directory[0]["index"]), int(directory[-1]["index"]) + 1
                    for slot, n in slots(k0, k1):
                        h_ring[4 * slot * cols:4 * (slot + n) * cols].copy_(d_ring[slot:slot + n].view(torch.uint8).reshape(-1),
                                                                            non_blocking=True)
                torch.cuda.synchronize()
                last["a"] = ro.periodic_levels_host(host_ring, recorders, directory, room // 4)
                return len(last["a"][1])

            def leg_b(device_only=False):
                k0, head = state["b"]
                head += chunk
                k1 = max((head - 2) // S, k0)
                state["b"] = [k1, head]
                at = 0
                for slot, n in slots(k0, k1):
                    d_packed[at:at + n, :cols].copy_(d_ring[slot:slot + n], non_blocking=True)
                    at += n
                for i in range(k1 - k0):
                    old.ln_tile_resident(d_packed[i * S:], S, 0, cols, d_u8=d_levels[i * image:], d_minmax=d_ranges[2 * i:],
                                         row_stride=PACKED_STRIDE, stream=stream)
                if device_only:
                    return 0
                used = (k1 - k0) * image
                h_levels[:used].copy_(d_levels[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            # the legs against one another, on the first three chunks (the third wraps the ring where it is short of three)
            for _ in range(3):
                d_levels.zero_()
                used = leg_new()
                want = h_levels.numpy()[:used].copy()
                d_levels.zero_()                             # (b writes no padding: the zeros stand for it)
                assert leg_b() == used and h_levels.numpy()[:used].tobytes() == want.tobytes(), "new and b disagree"
                assert leg_a() == used
                d = np.abs(last["a"][1].astype(np.int16) - want.astype(np.int16))
                assert d.max() <= 1 and (d != 0).mean() < 2e-3, "new and a disagree"
            per_chunk = chunk / S
            say("%s: S = %d, %d columns, ring of %d rows; %.1f snapshots, %.2f M pixels and %.2f MB of levels per chunk" % (
                name, S, cols, ring_rows, per_chunk, 1e-6 * per_chunk * S * cols, 1e-6 * per_chunk * image))
            t = {"new": [], "a": [], "b": []}
            for _ in range(args.repeats):
                t["new"].append(window(leg_new, args.window))
                t["a"].append(window(leg_a, args.window))
                t["b"].append(window(leg_b, args.window))
            for leg, what in (("new", "plan, three launches, levels to the host        "),
                              ("a", "rows to the host, ro_periodic_levels_host there "),
                              ("b", "un-wrap, per image reset + ln tile call, levels "),):
                us = [1e6 * x for x in t[leg]]
                say("  leg %-3s %s median %10.1f us   min %10.1f   max %10.1f   %12.0f rows/s   (%s)" % (
                    leg, what, np.median(us), min(us), max(us), chunk / np.median(t[leg]), " ".join("%.1f" % x for x in us)))
            say("  rows/s of new over a = %.2f, over b = %.2f (medians)" % (np.median(t["a"]) / np.median(t["new"]),
                                                                          np.median(t["b"]) / np.median(t["new"])))
            dev = {"new": [], "b": []}
            for _ in range(args.repeats):
                for leg, fn in (("new", leg_new), ("b", leg_b)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn(True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(20):
                        fn(True)
                    e1.record()
                    torch.cuda.synchronize()
                    dev[leg].append(1e3 * e0.elapsed_time(e1) / 20)
            for leg in ("new", "b"):
                say("  device %-3s median %8.1f us per chunk   min %8.1f   max %8.1f   (%s)" % (
                    leg, np.median(dev[leg]), min(dev[leg]), max(dev[leg]), " ".join("%.1f" % x for x in dev[leg])))
            say("  device time of b over new = %.2f (medians; 20 chunks enqueued back to back between two events)" % (
                np.median(dev["b"]) / np.median(dev["new"])))
            say("  (b: %.1f us per operation at %d x 4 operations per chunk)" % (
                np.median(dev["b"]) / (4 * (chunk - 2) // S), (chunk - 2) // S))
            say()
            del d_ring, d_levels, h_levels, h_ring, host_ring, d_packed
    say(NOTES)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
