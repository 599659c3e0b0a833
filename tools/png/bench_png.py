#!/usr/bin/env python3
"""What it costs to get the preview FILES of a chunk's periodic snapshots to the host: ro_stft_levels_png_resident
(csrc/ro_png.hip) behind ro_stft_periodic_levels_resident, against finishing the files on the host.

One step is one chunk: the ring (synthetic positive rows; no transform runs here) is taken to hold the stream up to the
chunk's end, and every snapshot that has become due in the chunk ends as a complete PNG file in pinned host memory.
Legs:
  new    the plan and ro_periodic_level_dir (host arithmetic), the levels call, the upload of the level directory (entries x
         32 bytes and the summary, one copy), the PNG call, the files in use to pinned host memory (their size is host
         arithmetic: ro_png_bytes of every written entry), synchronise
  a      the plan, the levels call, the levels in use to pinned host memory, synchronise; then ro_levels_png_host over them on
         one host thread
Both are wall-clock times of the host thread from the first call to the end of the last wait or conversion.  `device` is the
time between two events around the PNG call alone, 20 chunks enqueued back to back by this Python thread over levels and a
directory that are already on the device: where the host enqueues more slowly than the device runs, the figure is the
host's enqueue rate, so it is an UPPER BOUND of the device time.  Shapes: the headline (32768 bins, 75 % overlap, 48 kHz:
S = 352, a 615-column window, chunks of 16384 rows) and Bolidozor.json's (65536 bins, overlap 49152, 96 kHz: S = 352, the
26200 ... 26800 Hz window, chunks of 4096 rows).  `--repeats` alternations of the legs, each a window of at least `--window`
seconds over consecutive chunks of the stream, after one pass of both legs that checks them against one another: the same
bytes.  The report goes to stdout and to `--out`.

    python tools/png/bench_png.py [--window 0.5] [--repeats 5] [--out profiles/png.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK, LBLOCK, ALIGN = 2880, 720, 16
SHAPES = [  # name, sample rate, bins, overlap, snapshot_length, (low, high) Hz or None for `cols`, cols, chunk rows
    ("headline: 32768 bins, 75 % overlap, 615-column window, chunks of 16384 rows", 48000, 32768, 24576, 60, None, 615, 16384),
    ("Bolidozor.json: 65536 bins, overlap 49152, 26200 ... 26800 Hz, chunks of 4096 rows", 96000, 65536, 49152, 60,
     (26200.0, 26800.0), None, 4096),
]

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Nobody has measured any of the legs.  At the headline shape a chunk of 16384 rows makes 46 or 47 snapshots of 352 rows x 615
columns due: 10 MB of levels (profiles/levels.txt: 263 us per chunk to the host, 50 us of it on the device), and as files
352 x 616 raw bytes in 4 stored blocks each, 217 KB a file, some 186 blocks per chunk.  The PNG call is three launches; a
workgroup takes a stored block, reads 64 KB of levels a byte at a time and writes 64 KB, with a division and eight LDS
look-ups per word: 186 workgroups on 256 CUs, one round, 10 to 30 us on the device, and with the plan and the finish
launches 20 to 40 us in all.  Leg new adds that, an upload of 1.5 KB and the marshalling of one more call to the levels leg and
downloads the same 10 MB: 300 to 350 us per chunk.  Leg a downloads the levels (263 us) and then makes two dependent passes
over every byte on one host thread -- a table look-up per byte for the CRC-32, an add and two remainders per byte for the
Adler-32 -- at 100 to 300 MB/s together: 35 to 100 ms per chunk, 100 to 300 x behind.  Bolidozor's chunk is a quarter of
the rows and two thirds of the columns, 11 or 12 files of 144 KB (3 blocks each): the same order, with the fixed costs of new
(six launches, a copy each way, a wait) a larger share.  Nothing is gated on these numbers.
"""

NOTES = """\
Reading the device lines: they are upper bounds of device time.  The 20 chunks between the two events are enqueued by one
Python thread (the marshalling of one call and three launches per chunk); where that is slower than the device, the
figure is the enqueue rate.
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
    with ro.Stft(bins=256, overlap=0) as st:
        for name, rate, bins, overlap, length, band, cols, chunk in SHAPES:
            S = ro.snapshot_rows(rate, bins, overlap, length)
            if band is not None:
                cols = ro.frequency_to_bin(bins, rate, band[1]) - ro.frequency_to_bin(bins, rate, band[0])
            recorders = [(S, 0, cols)]
            ring_rows = chunk + S + 2 + 158                  # at least S + 2 rows more than a chunk
            most = chunk // S + 2                            # snapshots a chunk can make due
            unit, image = padded(4 * S * cols, BLOCK), padded(S * cols, LBLOCK)
            file_room = padded(ro.png_bytes(cols, S), ALIGN)
            room, png_room = most * unit, most * file_room
            d_ring = torch.rand((ring_rows, cols), dtype=torch.float32, device="cuda") * 100.0 + 1e-3
            ring = ro.capi.RowRing(d_ring.data_ptr(), cols, ring_rows, cols, 0)
            d_levels = torch.zeros(room // 4, dtype=torch.uint8, device="cuda")
            d_ranges = torch.zeros(most * 2, dtype=torch.float32, device="cuda")
            d_ldir = torch.zeros(most * 32 + 64, dtype=torch.uint8, device="cuda")   # the level directory, then its summary
            h_ldir = pinned(most * 32 + 64)
            d_png = torch.zeros(png_room, dtype=torch.uint8, device="cuda")
            d_png_dir = torch.zeros(most * 32, dtype=torch.uint8, device="cuda")
            d_png_sum = torch.zeros(64, dtype=torch.uint8, device="cuda")
            h_png, h_levels = pinned(png_room), pinned(room // 4)
            state = {"new": [np.zeros(1, np.int64), 0], "a": [np.zeros(1, np.int64), 0]}
            last = {}

            def plan(leg):
                nxt, head = state[leg]
                head += chunk
                state[leg][1] = head
                return ro.periodic_plan(recorders, nxt, head, False, ring_rows, cols, room, most)

            def png_call():
                st.levels_png_resident(d_ldir, most, d_ldir[most * 32:], d_levels, room // 4, d_png_dir, d_png, png_room, d_png_sum,
                                       stream=stream)

            def leg_new():
                directory, sm = plan("new")
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                level_dir, level_sm = ro.periodic_level_dir(directory)
                h = h_ldir.numpy()
                h[:len(level_dir) * 32] = level_dir.view(np.uint8)
                h[most * 32:] = np.array([level_sm]).view(np.uint8)
                d_ldir.copy_(h_ldir, non_blocking=True)
                png_call()
                used = sum(padded(ro.png_bytes(int(e["naxis1"]), int(e["naxis2"])), ALIGN) for e in level_dir if e["status"] == 0)
                h_png[:used].copy_(d_png[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            def leg_a():
                directory, sm = plan("a")
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                used = int(sm["units_bytes"]) // 4
                h_levels[:used].copy_(d_levels[:used], non_blocking=True)
                torch.cuda.synchronize()
                level_dir, level_sm = ro.periodic_level_dir(directory)
                last["a"] = ro.levels_png_host(level_dir, np.array([level_sm]), h_levels.numpy()[:used], png_room)
                return len(last["a"][1])

            # the legs against one another, on the first three chunks
            for _ in range(3):
                used = leg_new()
                assert used > 0 and leg_a() == used and h_png.numpy()[:used].tobytes() == last["a"][1].tobytes(), "new and a disagree"
            per_chunk = chunk / S
            say("%s: S = %d, %d columns, ring of %d rows; %.1f files of %d bytes, %.2f MB of files per chunk" % (
                name, S, cols, ring_rows, per_chunk, ro.png_bytes(cols, S), 1e-6 * per_chunk * file_room))
            t = {"new": [], "a": []}
            for _ in range(args.repeats):
                t["new"].append(window(leg_new, args.window))
                t["a"].append(window(leg_a, args.window))
            for leg, what in (("new", "levels, directory upload, PNG call, files to the host  "),
                              ("a", "levels to the host, ro_levels_png_host there           "),):
                us = [1e6 * x for x in t[leg]]
                say("  leg %-3s %s median %10.1f us   min %10.1f   max %10.1f   %12.0f rows/s   (%s)" % (
                    leg, what, np.median(us), min(us), max(us), chunk / np.median(t[leg]), " ".join("%.1f" % x for x in us)))
            say("  rows/s of new over a = %.2f (medians)" % (np.median(t["a"]) / np.median(t["new"])))
            dev = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                png_call()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(20):
                    png_call()
                e1.record()
                torch.cuda.synchronize()
                dev.append(1e3 * e0.elapsed_time(e1) / 20)
            say("  device: the PNG call alone   median %8.1f us per chunk   min %8.1f   max %8.1f   (%s)" % (
                np.median(dev), min(dev), max(dev), " ".join("%.1f" % x for x in dev)))
            say()
            del d_ring, d_levels, d_png, h_png, h_levels
    say(NOTES)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
