#!/usr/bin/env python3
"""What it costs to get a chunk's periodic snapshots to the host as FITS data units: ro_stft_periodic_units_resident
(csrc/ro_periodic.hip), one launch from the ring's slots to the units, against the two routes a resident host had before it.

One step is one chunk: the ring (synthetic rows; no transform runs here) is taken to hold the stream up to the chunk's end,
and every snapshot that has become due in the chunk ends as its padded big-endian data unit in pinned host memory, ready
for one fwrite behind its header.  Legs:
  new the plan (host arithmetic), the one launch, the units in use to pinned host memory, synchronise
  a   the ring's rows of the due snapshots to pinned host memory (one copy, two where they wrap), synchronise; then per
      snapshot the cut to the recorder's columns and astype('>f4') into a zero-padded buffer (numpy, one host thread)
  b   a device-to-device un-wrap of those rows into a packed image (one copy, two where they wrap), ro_snapshot_t entries and
      a summary built by hand and uploaded, ro_stft_snapshot_units_resident, the units in use to pinned host memory,
      synchronise
a and b are built only from calls the parent commit has.  All three are wall-clock times of the host thread from the first
call to the end of the last wait or conversion; `device` is the time between two events around the device work of new and
of b alone (no download).  Shapes: the headline (32768 bins, 75 % overlap, 48 kHz: S = 352, a 615-column window, chunks of
16384 rows) and Bolidozor.json's (65536 bins, overlap 49152, 96 kHz: S = 352, the 26200 ... 26800 Hz window, chunks of 4096
rows).  `--repeats` alternations of the legs, each a window of at least `--window` seconds over consecutive chunks of the
stream, after one warm-up pass of every leg.  The legs must give the same bytes; the tool checks it on the first chunks.
The report goes to stdout and to `--out`.

    python tools/periodic/bench_periodic.py [--window 0.5] [--repeats 5] [--out profiles/periodic_units.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK = 2880
SHAPES = [  # name, sample rate, bins, overlap, snapshot_length, (low, high) Hz or None for `cols`, cols, chunk rows
    ("headline: 32768 bins, 75 % overlap, 615-column window, chunks of 16384 rows", 48000, 32768, 24576, 60, None, 615, 16384),
    ("Bolidozor.json: 65536 bins, overlap 49152, 26200 ... 26800 Hz, chunks of 4096 rows", 96000, 65536, 49152, 60,
     (26200.0, 26800.0), None, 4096),
]

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Nobody has measured any of the three legs.  At the headline shape a chunk of 16384 rows makes 46 or 47 snapshots of 352 rows
x 615 columns due: 40 MB of ring rows become 40 MB of units.  The new call reads every ring byte once and writes every unit
byte once, 80 MB of HBM traffic: tens of microseconds on the device.  Route b moves the same bytes twice (the un-wrap copy,
then the units kernel over the packed image) and uploads a directory: about twice the device time, still far below a
millisecond.  What the host waits for in both is the download of 40 MB, a millisecond or two -- so in wall-clock rows/s the
new call and b should be within ten per cent of one another, the new call ahead by what b spends on its extra copy, the
directory and its upload; on the device alone the new call should be about 2 x ahead.  Route a downloads the same 40 MB and
then makes FITSWriter's pass on one host thread, a cut and a byte swap of every float, which profiles/fits_units.txt has at
several times the download: the new call should be 5 to 20 x ahead of a.  Bolidozor's chunk is a quarter of the rows and two
thirds of the columns, 11 or 12 snapshots and 7 MB: the same ratios, with the fixed costs (launches, waits) a larger share.
Nothing is gated on these numbers.
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


def padded(nbytes):
    return -(-nbytes // BLOCK) * BLOCK


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
    with ro.Stft(bins=256, overlap=0) as st:                 # (the call needs a handle for its device; no transform runs)
        for name, rate, bins, overlap, length, band, cols, chunk in SHAPES:
            S = ro.snapshot_rows(rate, bins, overlap, length)
            if band is not None:
                cols = ro.frequency_to_bin(bins, rate, band[1]) - ro.frequency_to_bin(bins, rate, band[0])
            recorders = [(S, 0, cols)]
            ring_rows = chunk + S + 2 + 158                  # at least S + 2 rows more than a chunk
            most = chunk // S + 2                            # snapshots a chunk can make due
            room = most * padded(4 * S * cols)
            d_ring = torch.randn((ring_rows, cols), dtype=torch.float32, device="cuda")
            ring = ro.capi.RowRing(d_ring.data_ptr(), cols, ring_rows, cols, 0)
            d_units = torch.zeros(room, dtype=torch.uint8, device="cuda")
            h_units = pinned(room)
            h_rows = pinned(4 * most * S * cols)             # leg a: the rows as they come off the ring
            host_units = np.zeros(room, np.uint8)            # ... and its padded buffer
            d_packed = torch.zeros((most * S, cols), dtype=torch.float32, device="cuda")      # leg b
            h_dir, h_sum = pinned(most * 72), pinned(64)
            d_dir = torch.zeros(most * 72, dtype=torch.uint8, device="cuda")
            d_sum = torch.zeros(64, dtype=torch.uint8, device="cuda")
            d_unit_dir = torch.zeros(most * 32, dtype=torch.uint8, device="cuda")
            d_unit_sum = torch.zeros(64, dtype=torch.uint8, device="cuda")
            state = {"new": [np.zeros(1, np.int64), 0], "a": [0, 0], "b": [0, 0]}        # next snapshot, head row

            def due(leg):
                """the closed form by hand, for the legs that have no plan: snapshots [k0, k1) at the next chunk's end"""
                k0, head = state[leg]
                head += chunk
                k1 = max((head - 2) // S, k0)
                state[leg] = [k1, head]
                return k0, k1

            def slots(k0, k1):
                """rows [k0 S, k1 S) as one or two runs of ring slots: [(slot, rows), ...]"""
                first, n = (k0 * S) % ring_rows, (k1 - k0) * S
                return [(first, n)] if first + n <= ring_rows else [(first, ring_rows - first), (0, n - (ring_rows - first))]

            def leg_new(device_only=False):
                nxt, head = state["new"]
                head += chunk
                state["new"][1] = head
                directory, sm = ro.periodic_plan(recorders, nxt, head, False, ring_rows, cols, room, most)
                st.periodic_units_resident(ring, recorders, directory, d_units, room, stream=stream)
                if device_only:
                    return 0
                used = int(sm["units_bytes"])
                h_units[:used].copy_(d_units[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            def leg_a():
                k0, k1 = due("a")
                at = 0
                for slot, n in slots(k0, k1):
                    h_rows[at:at + 4 * n * cols].copy_(d_ring[slot:slot + n].view(torch.uint8).reshape(-1), non_blocking=True)
                    at += 4 * n * cols
                torch.cuda.synchronize()
                rows = h_rows.numpy()[:at].view(np.float32).reshape(-1, cols)
                out = 0
                for i in range(k1 - k0):
                    cut = rows[i * S:(i + 1) * S, recorders[0][1]:recorders[0][1] + cols]
                    nbytes = 4 * cut.size
                    host_units[out:out + nbytes].view(">f4").reshape(cut.shape)[...] = cut
                    host_units[out + nbytes:out + padded(nbytes)] = 0
                    out += padded(nbytes)
                return out

            def leg_b(device_only=False):
                k0, k1 = due("b")
                at = 0
                for slot, n in slots(k0, k1):
                    d_packed[at:at + n].copy_(d_ring[slot:slot + n], non_blocking=True)
                    at += n
                n = k1 - k0
                directory = h_dir.numpy()[:n * 72].view(ro.capi.SNAPSHOT_DTYPE)
                directory[...] = 0
                directory["first_row"] = np.arange(k0, k1) * S
                directory["rows"], directory["status"] = S, ro.RO_SNAP_CAPTURED
                directory["offset"] = np.arange(n) * S * cols
                summary = h_sum.numpy().view(ro.capi.SNAP_SUMMARY_DTYPE)
                summary[...] = 0
                summary["resolved"] = summary["captured"] = n
                d_dir[:n * 72].copy_(h_dir[:n * 72], non_blocking=True)
                d_sum.copy_(h_sum, non_blocking=True)
                st.snapshot_units_resident(d_dir, n, d_sum, d_packed, n * S * cols, cols, [(recorders[0][1], cols)], d_unit_dir,
                                           d_units, room, d_unit_sum, stream=stream)
                if device_only:
                    return 0
                used = n * padded(4 * S * cols)              # (known on the host here: nothing is read back to size the copy)
                h_units[:used].copy_(d_units[:used], non_blocking=True)
                torch.cuda.synchronize()
                return used

            # the same bytes, on the first three chunks (the third wraps the ring where the ring is short of three chunks)
            for _ in range(3):
                used = leg_new()
                want = h_units.numpy()[:used].tobytes()
                assert leg_a() == used and host_units[:used].tobytes() == want, "new and a disagree"
                assert leg_b() == used and h_units.numpy()[:used].tobytes() == want, "new and b disagree"
            per_chunk = chunk / S
            say("%s: S = %d, %d columns, ring of %d rows; %.1f snapshots and %.2f MB of units per chunk" % (
                name, S, cols, ring_rows, per_chunk, 1e-6 * per_chunk * padded(4 * S * cols)))
            t = {"new": [], "a": [], "b": []}
            for _ in range(args.repeats):
                t["new"].append(window(leg_new, args.window))
                t["a"].append(window(leg_a, args.window))
                t["b"].append(window(leg_b, args.window))
            for leg, what in (("new", "plan, one launch, units to the host          "),
                              ("a", "rows to the host, cut + swap + pad there      "),
                              ("b", "un-wrap, directory by hand, units call, units "),):
                us = [1e6 * x for x in t[leg]]
                say("  leg %-3s %s median %10.1f us   min %10.1f   max %10.1f   %12.0f rows/s   (%s)" % (
                    leg, what, np.median(us), min(us), max(us), chunk / np.median(t[leg]), " ".join("%.1f" % x for x in us)))
            say("  rows/s of new over a = %.2f, over b = %.2f (medians)" % (np.median(t["a"]) / np.median(t["new"]),
                                                                          np.median(t["b"]) / np.median(t["new"])))
            # the device's part alone: events around 20 chunks of each, alternated
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
            say()
            del d_ring, d_units, h_units, h_rows, d_packed
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
