#!/usr/bin/env python3
"""What it costs to get the rows of a chunk's events to the host: the parent commit's way against the row ring and
ro_stft_snapshots_resident (csrc/ro_snapshots.hip).

One step is one chunk of `--rows` image rows of 615 columns (radio-observer.json's snapshot band at 32768 bins) that are
already in HBM with their scan records; no transform runs here.  Legs:
  a   the parent's way: keep the chunk's rows (a device copy behind the previous chunk's), ro_stft_events_resident,
      copy the summary and the events to pinned host memory, SYNCHRONISE, then per event whose rows are complete one
      ro_stft_cut_windows_resident of its rows and one copy of them to pinned host memory; synchronise
  b   ro_stft_ring_put_resident, ro_stft_events_resident, ro_stft_snapshots_resident, then ONE download of the summary,
      the directory and the arena at their full size; synchronise
  b'  as b, but the summary is fetched first (a synchronisation) and only the directory entries and arena floats in use
      after it
All are wall-clock times of the host thread from the first call to the end of the last wait.  Two event densities: a few
events per chunk and many.  Five alternations of the legs, each a window of at least `--window` seconds.  The legs must
give the same images; the tool checks it.  The report goes to stdout and to `--out`.

    python tools/snapshots/bench_snapshots.py [--window 0.3] [--repeats 5] [--out profiles/snapshots.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BINS, FIRST_COL, COLS = 1024, 204, 615
DETECTOR = (11, 29)                                          # radio-observer.json at 32768 bins, 75 % overlap
SNAP = 120
DENSITIES = [("few events", 1024), ("many events", 64)]      # a burst of 3 ... 12 detect rows every so many rows

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Nobody has measured either leg.  The copies themselves are trivial for the device: an event's snapshot is some 30 to 50 rows
of 615 floats (about 100 KB), a chunk's ring put 10 MB.  What differs is the host's part: leg a waits for the events before
it can issue anything, then makes two calls per event (a cut and a copy); leg b makes three calls and one download whatever
the number of events, and waits once.  With a few events per chunk both legs are a handful of calls and should be of the
same order, leg b's full-size download of a mostly empty arena possibly costing it the difference; with a hundred events per
chunk leg a's two hundred calls (several microseconds each) should make it several times slower than leg b'.  Nothing is
gated on these numbers.
"""


def records(ro, rows, every, seed=0):
    rng = np.random.default_rng(seed)
    d = np.zeros(rows, bool)
    for i, first in enumerate(range(17, rows, every)):
        d[first:first + (3, 6, 12, 5)[i % 4]] = True
    recs = np.zeros(rows, ro.capi.SCAN_DTYPE)
    recs["noise"] = (1.0 + rng.random(rows)).astype(np.float32)
    recs["average"] = recs["noise"] * np.where(d, np.float32(3.0), np.float32(1.5))
    recs["peak"] = rng.integers(0, 410, rows)
    return recs


def window(fn, seconds):
    """fn() back to back for at least `seconds` of wall clock: seconds per call"""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        t = time.perf_counter() - t0
        if t >= seconds and n >= 3:
            return t / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(EXPECTATION)
    say("Measured (%s, %d alternations, windows of >= %.1f s, chunks of %d rows x %d columns)" % (
        torch.cuda.get_device_name(0), args.repeats, args.window, args.rows, COLS))
    say("=" * 100)
    stream = torch.cuda.current_stream().cuda_stream
    rows = args.rows
    first = rows                                             # the step is the stream's second chunk: rows [rows, 2 rows)
    head = first + rows
    ring_rows = 2 * rows
    bands = ro.Bands(low_noise=20, noise_width=64, low_detect=300, detect_width=64, avg_bins=9)
    image = (np.arange(2 * rows, dtype=np.float32)[:, None] * 1000 + np.arange(COLS, dtype=np.float32)[None, :])
    for name, every in DENSITIES:
        recs = records(ro, rows, every)
        cap = max(8, 2 * rows // every)
        pcap = 64
        arena_floats = cap * SNAP * COLS
        with ro.Stft(bins=BINS, overlap=0, bands=bands) as st:
            d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
            d_image = torch.from_numpy(image[rows:].copy()).cuda()               # this chunk's image
            d_state = torch.zeros(32, dtype=torch.uint8, device="cuda")
            d_events = torch.zeros(cap * 40, dtype=torch.uint8, device="cuda")
            d_summary = torch.zeros(24, dtype=torch.uint8, device="cuda")
            h_events = torch.empty(d_events.shape, dtype=torch.uint8).pin_memory()
            h_summary = torch.empty(d_summary.shape, dtype=torch.uint8).pin_memory()
            # leg a: the rows kept as full-width rows (the cut reads rows of at least `bins` floats), previous chunk in front
            d_kept = torch.zeros((2 * rows, BINS), dtype=torch.float32, device="cuda")
            d_kept[:rows, FIRST_COL:FIRST_COL + COLS] = torch.from_numpy(image[:rows].copy()).cuda()
            d_cut = torch.zeros((cap, SNAP * COLS), dtype=torch.float32, device="cuda")
            h_cut = torch.empty((cap, SNAP * COLS), dtype=torch.float32).pin_memory()
            # leg b: the ring (the previous chunk is in it), the lists, the outputs in one block: summary | directory | arena
            d_ring = torch.zeros((ring_rows, COLS), dtype=torch.float32, device="cuda")
            d_ring[:rows] = torch.from_numpy(image[:rows].copy()).cuda()
            ring = ro.capi.RowRing(d_ring.data_ptr(), COLS, ring_rows, COLS, 0)
            d_pending = torch.zeros(pcap * 40, dtype=torch.uint8, device="cuda")
            d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
            dir_bytes = (cap + pcap) * 72
            d_out = torch.zeros(64 + dir_bytes + arena_floats * 4, dtype=torch.uint8, device="cuda")
            h_out = torch.empty(d_out.shape, dtype=torch.uint8).pin_memory()
            d_sum, d_dir, d_arena = d_out[:64], d_out[64:64 + dir_bytes], d_out[64 + dir_bytes:]
            got = {}

            def leg_a():
                d_kept[rows:, FIRST_COL:FIRST_COL + COLS].copy_(d_image)
                d_state.zero_()
                st.events_resident(rows, [DETECTOR], d_state, d_records=d_recs, first_row=first, d_events=d_events,
                                   capacity=cap, d_summary=d_summary, stream=stream)
                h_summary.copy_(d_summary, non_blocking=True)
                h_events.copy_(d_events, non_blocking=True)
                torch.cuda.synchronize()
                n = min(int(h_summary.numpy().view(ro.capi.DETECT_SUMMARY_DTYPE)["events"][0]), cap)
                ev = h_events.numpy().view(ro.capi.EVENT_DTYPE)[:n]
                done = []
                for i in range(n):
                    lo = max(int(ev["start_row"][i]), 0)
                    hi = int(ev["start_row"][i]) + min(int(ev["length"][i]), SNAP)
                    if hi > head or hi <= lo:
                        continue                             # (a host remembers the first kind for the next chunk)
                    st.cut_windows_resident(d_kept[lo:], hi - lo, [(FIRST_COL, COLS)], d_cut[i], row_stride=BINS,
                                            image_stride=COLS, stream=stream)
                    h_cut[i, :(hi - lo) * COLS].copy_(d_cut[i, :(hi - lo) * COLS], non_blocking=True)
                    done.append((i, lo, hi))
                torch.cuda.synchronize()
                got["a"] = done

            def put_events_snapshots():
                d_count.zero_()
                d_state.zero_()
                st.ring_put_resident(d_image, first, rows, ring, stream=stream)
                st.events_resident(rows, [DETECTOR], d_state, d_records=d_recs, first_row=first, d_events=d_events,
                                   capacity=cap, d_summary=d_summary, stream=stream)
                st.snapshots_resident(1, SNAP, ring, head, d_pending, d_count, pcap, d_dir, d_arena, arena_floats, d_sum,
                                      d_events=d_events, capacity=cap, d_summary=d_summary, stream=stream)

            def leg_b():
                put_events_snapshots()
                h_out.copy_(d_out, non_blocking=True)
                torch.cuda.synchronize()

            def leg_b2():
                put_events_snapshots()
                h_out[:64].copy_(d_sum, non_blocking=True)
                torch.cuda.synchronize()
                sm = h_out[:64].numpy().view(ro.capi.SNAP_SUMMARY_DTYPE)[0]
                nd, nf = int(sm["resolved"]) * 72, int(sm["arena_floats"]) * 4
                h_out[64:64 + nd].copy_(d_dir[:nd], non_blocking=True)
                h_out[64 + dir_bytes:64 + dir_bytes + nf].copy_(d_arena[:nf], non_blocking=True)
                torch.cuda.synchronize()

            leg_a()
            for leg in (leg_b, leg_b2):
                h_out.zero_()
                leg()
                sm = h_out[:64].numpy().view(ro.capi.SNAP_SUMMARY_DTYPE)[0]
                d = h_out[64:64 + int(sm["resolved"]) * 72].numpy().view(ro.capi.SNAPSHOT_DTYPE)
                arena = h_out[64 + dir_bytes:].numpy().view(np.float32)
                assert len(got["a"]) == int(sm["captured"]) == d.size > 0 and int(sm["lost"]) == 0, (len(got["a"]), sm)
                for (i, lo, hi), e in zip(got["a"], d):
                    n = (hi - lo) * COLS
                    assert (int(e["first_row"]), int(e["rows"])) == (lo, hi - lo), "the legs disagree"
                    assert np.array_equal(arena[int(e["offset"]):int(e["offset"]) + n], h_cut[i, :n].numpy()), "the legs disagree"
                    assert arena[int(e["offset"])] == lo * 1000.0
            a, b, b2 = [], [], []
            for _ in range(args.repeats):
                a.append(window(leg_a, args.window) * 1e6)
                b.append(window(leg_b, args.window) * 1e6)
                b2.append(window(leg_b2, args.window) * 1e6)
            say("%s: a burst every %d rows; %d events in the chunk, %d snapshots complete (%.2f MB), %d pending; arena of %.1f MB" % (
                name, every, int(h_summary.numpy().view(ro.capi.DETECT_SUMMARY_DTYPE)["events"][0]), int(sm["captured"]),
                int(sm["arena_floats"]) * 4 / 1e6, int(sm["pending"]), arena_floats * 4 / 1e6))
            for tag, what, t in (("a ", "events, wait, a cut and a copy per event  ", a), ("b ", "put, events, snapshots, one full download", b),
                                 ("b'", "... summary first, then what is in use   ", b2)):
                say("  leg %s %s median %9.1f us   min %9.1f   max %9.1f   (%s)" % (
                    tag, what, np.median(t), min(t), max(t), " ".join("%.1f" % x for x in t)))
            say("  a / b = %.2f, a / b' = %.2f (medians)" % (np.median(a) / np.median(b), np.median(a) / np.median(b2)))
            say()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
