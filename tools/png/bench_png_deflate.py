#!/usr/bin/env python3
"""What the compressed preview files cost and save: ro_stft_levels_png_deflate_resident (csrc/ro_png_deflate.hip) against the
stored-block call it stands beside, and against compressing on the host.

One step is one chunk, as in tools/png/bench_png.py: the ring is taken to hold the stream up to the chunk's end, and every
periodic snapshot that has become due in the chunk ends as a complete PNG file in pinned host memory.  The ring's rows are
real ones: the transform (run_resident) of Gaussian noise with a synthetic event -- a tone thirty times the noise's sigma
that drifts through the window for a few hundred rows out of every few thousand -- cut to the window's columns, so the levels
are ln images of receiver noise and not constants or uniform bytes, which only bracket the ratio.
Legs, each ending with the files in pinned host memory:
  new     the plan and ro_periodic_level_dir (host arithmetic), the levels call, the upload of the level directory, the deflate
          call, the directory and the summary to the host, a wait (the files' sizes are the data's), units_bytes of files to
          the host, a wait
  stored  the same with ro_stft_levels_png_resident, whose sizes are host arithmetic: one download, one wait
  host    the plan, the levels call, the levels in use to pinned host memory, a wait; then ro_levels_png_deflate_host over them
          on one host thread
All are wall-clock times of the host thread.  `device` is the time between two events around the call alone, 20 chunks
enqueued back to back over levels and a directory already on the device (an upper bound where the host enqueues more
slowly than the device runs).  The byte ratio is the files of new over the files of stored.  `--repeats` alternations of the
legs, each a window of at least `--window` seconds over consecutive chunks, after one pass that checks new against host: the
same bytes.  The report goes to stdout and to `--out`.

    python tools/png/bench_png_deflate.py [--window 0.5] [--repeats 5] [--out profiles/png_deflate.txt]
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
Nobody has measured the device call.  What is known: on synthetic 352 x 615 ln images of Rayleigh magnitudes a Python
restatement of the stream gives Huffman-only files of 0.78 (pure noise) and 0.71 (noise with a strong event) of the stored
ones, so the byte ratio here, on rows of the transform itself, should be 0.71 to 0.79; and the stored call takes 44.5 us
(headline) and 43.0 us (Bolidozor) on the device and 323 us and 133 us to the host (profiles/png.txt).
The deflate call is six launches instead of three and makes three passes over the levels.  Its measure launch has a
workgroup per block: a histogram of 64 KB through LDS adds (10 us or so), three loops of 257 broadcast reads per lane, and ONE
lane that runs the 256 joins, the depths and the limit rule out of LDS -- some 3500 dependent LDS accesses at 50 ns: 150 to
200 us, which no other block hides because the 186 (35) blocks of a chunk run side by side on 256 CUs.  The emit launch is the
stored call's work plus two more reads of the levels from cache and an LDS OR per word: 40 to 80 us.  With the four small
launches: 250 to 400 us on the device per chunk, six to nine times the stored call, nearly the same at both shapes.  Leg new
then downloads a fifth to a quarter fewer bytes (2.3 MB less at the headline shape, 40 to 50 us on PCIe) but waits twice:
500 to 700 us at the headline shape against stored's 323 us, 350 to 500 us against 133 us at Bolidozor's.  So end to end
new is expected to be SLOWER than stored, by 1.5 to 3 x: the gain is bytes on disk and on the station's uplink, not time.
Leg host makes the twin's passes on one thread (histogram, codes, a bit writer, CRC-32 and Adler-32 byte by byte, all of it
twice: once to measure, once to write): 80 to 200 ms per headline chunk, two hundred times behind new.  Nothing is gated on
these numbers.
"""

NOTES = """\
Reading the device lines: they are upper bounds of device time.  The 20 chunks between the two events are enqueued by one
Python thread; where that is slower than the device, the figure is the enqueue rate.
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


def fill_ring(ro, torch, d_ring, bins, overlap, first_col, cols):
    """rows of the transform of noise with an event, cut to the window, into every row of the ring"""
    hop = bins - overlap
    piece = 512
    rows_total = d_ring.shape[0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20260521)
    d_rows = torch.empty((piece, bins), dtype=torch.float32, device="cuda")
    tone_bin = first_col + cols // 2 - bins // 2           # the window's middle column, as a signed frequency bin
    with ro.Stft(bins=bins, overlap=overlap) as st:
        for k, at in enumerate(range(0, rows_total, piece)):
            n = min(piece, rows_total - at)
            samples = (n - 1) * hop + bins
            iq = torch.randn((samples, 2), dtype=torch.float32, device="cuda", generator=gen)
            if k % 4 == 1:                                 # the event: a drifting tone in the middle 300 rows of this piece
                i = torch.arange(samples, dtype=torch.float64, device="cuda")
                lo, hi = 100 * hop, 400 * hop
                drift = (tone_bin + 40.0 * (i - lo) / (hi - lo)) / bins
                phase = 2.0 * np.pi * torch.cumsum(drift, 0)
                on = ((i >= lo) & (i < hi)).to(torch.float32) * 30.0
                iq[:, 0] += on * torch.cos(phase).to(torch.float32)
                iq[:, 1] += on * torch.sin(phase).to(torch.float32)
                del i, drift, phase, on
            st.run_resident(iq, ro.RO_IQ_F32, samples, 0, n, d_rows, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            d_ring[at:at + n] = d_rows[:n, first_col:first_col + cols]
            del iq
    del d_rows


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
    for name, rate, bins, overlap, length, band, cols, chunk in SHAPES:
        S = ro.snapshot_rows(rate, bins, overlap, length)
        first_col = bins // 2 + bins // 8
        if band is not None:
            first_col = ro.frequency_to_bin(bins, rate, band[0])
            cols = ro.frequency_to_bin(bins, rate, band[1]) - first_col
        recorders = [(S, 0, cols)]
        ring_rows = chunk + S + 2 + 158                  # at least S + 2 rows more than a chunk
        most = chunk // S + 2                            # snapshots a chunk can make due
        unit = padded(4 * S * cols, BLOCK)
        file_room = padded(ro.png_bytes(cols, S), ALIGN)
        room, png_room = most * unit, most * file_room
        d_ring = torch.empty((ring_rows, cols), dtype=torch.float32, device="cuda")
        fill_ring(ro, torch, d_ring, bins, overlap, first_col, cols)
        with ro.Stft(bins=256, overlap=0) as st:
            ring = ro.capi.RowRing(d_ring.data_ptr(), cols, ring_rows, cols, 0)
            d_levels = torch.zeros(room // 4, dtype=torch.uint8, device="cuda")
            d_ranges = torch.zeros(most * 2, dtype=torch.float32, device="cuda")
            d_ldir = torch.zeros(most * 32 + 64, dtype=torch.uint8, device="cuda")   # the level directory, then its summary
            h_ldir = pinned(most * 32 + 64)
            d_png = torch.zeros(png_room, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(most * 32 + 64, dtype=torch.uint8, device="cuda")    # the files' directory, then their summary
            h_out = pinned(most * 32 + 64)
            h_png, h_levels = pinned(png_room), pinned(room // 4)
            state = {leg: [np.zeros(1, np.int64), 0] for leg in ("new", "stored", "host")}
            last = {}

            def plan(leg):
                nxt, head = state[leg]
                head += chunk
                state[leg][1] = head
                return ro.periodic_plan(recorders, nxt, head, False, ring_rows, cols, room, most)

            def deflate_call():
                st.levels_png_deflate_resident(d_ldir, most, d_ldir[most * 32:], d_levels, room // 4, d_out, d_png, png_room,
                                               d_out[most * 32:], stream=stream)

            def stored_call():
                st.levels_png_resident(d_ldir, most, d_ldir[most * 32:], d_levels, room // 4, d_out, d_png, png_room,
                                       d_out[most * 32:], stream=stream)

            def levels_and_directory(leg):
                directory, sm = plan(leg)
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                level_dir, level_sm = ro.periodic_level_dir(directory)
                h = h_ldir.numpy()
                h[:len(level_dir) * 32] = level_dir.view(np.uint8)
                h[most * 32:] = np.array([level_sm]).view(np.uint8)
                d_ldir.copy_(h_ldir, non_blocking=True)
                return level_dir

            def leg_new():
                levels_and_directory("new")
                deflate_call()
                h_out.copy_(d_out, non_blocking=True)
                torch.cuda.synchronize()
                used = int(h_out.numpy()[most * 32:].view(ro.capi.UNIT_SUMMARY_DTYPE)["units_bytes"][0])
                h_png[:used].copy_(d_png[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            def leg_stored():
                level_dir = levels_and_directory("stored")
                stored_call()
                used = sum(padded(ro.png_bytes(int(e["naxis1"]), int(e["naxis2"])), ALIGN) for e in level_dir if e["status"] == 0)
                h_png[:used].copy_(d_png[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            def leg_host():
                directory, sm = plan("host")
                st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, room // 4, stream=stream)
                used = int(sm["units_bytes"]) // 4
                h_levels[:used].copy_(d_levels[:used], non_blocking=True)
                torch.cuda.synchronize()
                level_dir, level_sm = ro.periodic_level_dir(directory)
                last["host"] = ro.levels_png_deflate_host(level_dir, np.array([level_sm]), h_levels.numpy()[:used], png_room)
                return len(last["host"][1])

            # new against host on the first three chunks: the same bytes; and the byte ratio over them
            new_bytes = stored_bytes = files = 0
            for _ in range(3):
                used = leg_new()
                got = h_png.numpy()[:used].tobytes()
                png_dir = h_out.numpy()[:most * 32].view(ro.capi.FITS_UNIT_DTYPE).copy()
                assert used > 0 and leg_host() == used and got == last["host"][1].tobytes(), "new and host disagree"
                new_bytes += used
                stored_bytes += leg_stored()
                files += int((png_dir["bytes"] > 0).sum())
            per_chunk = chunk / S
            say("%s: S = %d, %d columns from column %d, ring of %d rows; %.1f files per chunk" % (
                name, S, cols, first_col, ring_rows, per_chunk))
            say("  bytes: %d files of %d bytes stored, %.0f bytes compressed on average; byte ratio new / stored = %.4f; "
                "%.2f MB against %.2f MB of files per chunk" % (files, ro.png_bytes(cols, S), new_bytes / files,
                                                                 new_bytes / stored_bytes, 1e-6 * per_chunk * new_bytes / files,
                                                                 1e-6 * per_chunk * stored_bytes / files))
            legs = (("new", leg_new, "levels, directory upload, deflate call, sizes, files to the host"),
                    ("stored", leg_stored, "levels, directory upload, stored call, files to the host       "),
                    ("host", leg_host, "levels to the host, ro_levels_png_deflate_host there           "))
            t = {leg: [] for leg, _, _ in legs}
            for _ in range(args.repeats):
                for leg, fn, _ in legs:
                    t[leg].append(window(fn, args.window))
            for leg, _, what in legs:
                us = [1e6 * x for x in t[leg]]
                say("  leg %-6s %s median %10.1f us   min %10.1f   max %10.1f   %12.0f rows/s   (%s)" % (
                    leg, what, np.median(us), min(us), max(us), chunk / np.median(t[leg]), " ".join("%.1f" % x for x in us)))
            say("  time of new over stored = %.2f, of host over new = %.2f (medians)" % (
                np.median(t["new"]) / np.median(t["stored"]), np.median(t["host"]) / np.median(t["new"])))
            dev = {"deflate": [], "stored": []}
            for _ in range(args.repeats):
                for which, call in (("deflate", deflate_call), ("stored", stored_call)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    call()
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(20):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    dev[which].append(1e3 * e0.elapsed_time(e1) / 20)
            for which in ("deflate", "stored"):
                say("  device: the %-7s call alone   median %8.1f us per chunk   min %8.1f   max %8.1f   (%s)" % (
                    which, np.median(dev[which]), min(dev[which]), max(dev[which]), " ".join("%.1f" % x for x in dev[which])))
            say()
        del d_ring, d_levels, d_png, h_png, h_levels
    say(NOTES)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
