#!/usr/bin/env python3
"""What it costs to get the raw I/Q of a chunk's events to the host as float pairs: a copy per event, issued by the host
once it has seen the snapshot directory, against ro_stft_raw_resident (csrc/ro_raw.hip).

One step is one chunk of `--rows` rows at the headline shape (32768 bins, 75 % overlap, 48 kHz) whose samples are already
in HBM in their wire format, as two chunk buffers that overlap by bins - hop samples, and whose snapshot directory is
already on the device (synthetic: snapshots of 40 rows spread over the chunk); no transform and no snapshot call runs
here.  Legs:
  a   the directory's way round the host: copy the snapshots' summary and directory to pinned host memory, SYNCHRONISE,
      then per captured entry one device-to-host copy of its sample run (two where it straddles the buffers) in the wire
      format; synchronise; convert to float pairs on the host (numpy)
  b   ro_stft_raw_resident, then the summary to pinned host memory, SYNCHRONISE, then the raw directory entries and the
      arena floats in use; synchronise
Both are wall-clock times of the host thread from the first call to the end of the last wait (leg a's conversion
included: the floats are what the FITS writer takes).  Two event densities, a few events per chunk and many, in two wire
formats.  Five alternations of the legs, each a window of at least `--window` seconds.  The legs must give the same
floats; the tool checks it.  The report goes to stdout and to `--out`.

    python tools/raw/bench_raw.py [--window 0.3] [--repeats 5] [--out profiles/raw_capture.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BINS, OVERLAP, RATE = 32768, 24576, 48000
SNAP = 40                                                    # rows of a snapshot: 40 / 5 x 48000 = 384000 samples of raw I/Q
DENSITIES = [("few events", 4), ("many events", 64)]

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Nobody has measured either leg.  At the headline shape a snapshot of 40 rows has a raw run of 384000 samples: 1.5 MB as
int16 pairs, 3.1 MB as float pairs.  The device's part is small either way (a run is read and written once, a few
microseconds each at HBM rates); what the host sees is dominated by the download.  Leg b downloads float pairs, leg a
the wire format, so with int16 samples leg a moves HALF the bytes over the link and then pays for the conversion on the
host (numpy, single-threaded, about a millisecond per run), while with float32 samples both move the same bytes and leg
a's conversion is a copy.  With a few events per chunk leg a is one wait and one copy per event more than leg b's two
waits, and the two should be of the same order, the link's time for some 6 to 12 MB (a fraction of a millisecond) plus
leg a's conversion.  With 64 events leg b downloads 197 MB in one copy (some 4 to 8 ms at the link's rate); leg a issues
64 or more copies of 1.5 or 3.1 MB -- large enough that the per-copy cost of the rows' case (profiles/snapshots.txt:
two small calls per event, 1.9 x to 9 x slower) should NOT show -- and converts 49 M numbers on the host, which should
cost it tens of milliseconds: leg b ahead by a small factor for float32 samples, and for int16 samples by whatever the
host's conversion costs beyond the halved download.  What leg b buys a resident host besides is that nothing waits for
the directory: the call is issued with the chunk's other calls.  Nothing is gated on these numbers.
"""


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
    say("Measured (%s, %d alternations, windows of >= %.1f s, chunks of %d rows of %d bins, hop %d)" % (
        torch.cuda.get_device_name(0), args.repeats, args.window, args.rows, BINS, BINS - OVERLAP))
    say("=" * 100)
    stream = torch.cuda.current_stream().cuda_stream
    rows, hop = args.rows, BINS - OVERLAP
    chunk_samples = (rows - 1) * hop + BINS
    first_row = rows                                         # the step is the stream's second chunk: rows [rows, 2 rows)
    firsts = [0, rows * hop]                                 # the two chunk buffers' first samples
    L = int(SNAP / 5.0 * RATE)
    with ro.Stft(bins=BINS, overlap=OVERLAP, sample_rate=RATE) as st:
        for fmt, fmt_name, dtype in ((ro.RO_IQ_I16, "int16", np.int16), (ro.RO_IQ_F32, "float32", np.float32)):
            rng = np.random.default_rng(3)
            d_iq = []
            for k in range(2):
                a = rng.integers(-2000, 2000, (chunk_samples, 2), dtype=np.int16).astype(dtype)
                d_iq.append(torch.from_numpy(a).cuda())
                del a
            spans = [(d_iq[k], firsts[k], chunk_samples, fmt) for k in range(2)]
            for name, events in DENSITIES:
                # snapshots of SNAP rows spread over the chunk, the first one starting in the chunk in front
                starts = first_row - SNAP // 2 + (np.arange(events) * ((rows - SNAP) // events))
                directory = np.zeros(events, ro.capi.SNAPSHOT_DTYPE)
                directory["event"]["start_row"], directory["event"]["length"] = starts, SNAP
                directory["event"]["fire_row"], directory["event"]["peak"] = starts + SNAP - 11, np.arange(events)
                directory["first_row"], directory["rows"], directory["status"] = starts, SNAP, ro.RO_SNAP_CAPTURED
                snap_summary = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
                snap_summary["resolved"] = snap_summary["captured"] = events
                d_dir = torch.from_numpy(directory.view(np.uint8).reshape(-1).copy()).cuda()
                d_snap_sum = torch.from_numpy(snap_summary.view(np.uint8).reshape(-1).copy()).cuda()
                h_dir = torch.empty(d_dir.shape, dtype=torch.uint8).pin_memory()
                h_snap_sum = torch.empty(d_snap_sum.shape, dtype=torch.uint8).pin_memory()
                pcap = 64
                arena_floats = events * 2 * L
                # leg a: one pinned buffer per event, in the wire format
                h_runs = torch.empty((events, L, 2), dtype=d_iq[0].dtype).pin_memory()
                # leg b: the pending list, and the outputs in one block: summary | raw directory | arena
                d_pending = torch.zeros(pcap * 72, dtype=torch.uint8, device="cuda")
                d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
                dir_bytes = (events + pcap) * 72
                d_out = torch.zeros(64 + dir_bytes + arena_floats * 4, dtype=torch.uint8, device="cuda")
                h_out = torch.empty(d_out.shape, dtype=torch.uint8).pin_memory()
                d_sum, d_raw_dir, d_arena = d_out[:64], d_out[64:64 + dir_bytes], d_out[64 + dir_bytes:]
                got = {}

                def leg_a():
                    h_snap_sum.copy_(d_snap_sum, non_blocking=True)
                    h_dir.copy_(d_dir, non_blocking=True)
                    torch.cuda.synchronize()
                    n = int(h_snap_sum.numpy().view(ro.capi.SNAP_SUMMARY_DTYPE)["resolved"][0])
                    d = h_dir.numpy().view(ro.capi.SNAPSHOT_DTYPE)[:n]
                    done = []
                    for i in range(n):
                        if d["status"][i] != ro.RO_SNAP_CAPTURED:
                            continue
                        start = int(d["event"]["start_row"][i])
                        length = int(d["rows"][i]) + int(d["first_row"][i]) - start
                        f, ln = start * hop + 1, int(length / 5.0 * RATE)
                        if f + ln > firsts[1] + chunk_samples:
                            continue                         # (a host remembers these for the next chunk)
                        cut = min(max(firsts[1] - f, 0), ln)  # samples the later buffer does not hold
                        if cut:
                            h_runs[i, :cut].copy_(d_iq[0][f - firsts[0]:f - firsts[0] + cut], non_blocking=True)
                        if cut < ln:
                            h_runs[i, cut:ln].copy_(d_iq[1][f + cut - firsts[1]:f + ln - firsts[1]], non_blocking=True)
                        done.append((i, f, ln))
                    torch.cuda.synchronize()
                    got["a"] = [(f, ln, h_runs[i, :ln].numpy().astype(np.float32)) for i, f, ln in done]

                def leg_b():
                    d_count.zero_()
                    st.raw_resident(d_dir, events, d_snap_sum, spans, d_pending, d_count, pcap, d_raw_dir, d_arena, arena_floats,
                                    d_sum, stream=stream)
                    h_out[:64].copy_(d_sum, non_blocking=True)
                    torch.cuda.synchronize()
                    sm = h_out[:64].numpy().view(ro.capi.RAW_SUMMARY_DTYPE)[0]
                    nd, nf = int(sm["resolved"]) * 72, int(sm["arena_floats"]) * 4
                    h_out[64:64 + nd].copy_(d_raw_dir[:nd], non_blocking=True)
                    h_out[64 + dir_bytes:64 + dir_bytes + nf].copy_(d_arena[:nf], non_blocking=True)
                    torch.cuda.synchronize()

                leg_a()
                h_out.zero_()
                leg_b()
                sm = h_out[:64].numpy().view(ro.capi.RAW_SUMMARY_DTYPE)[0]
                d = h_out[64:64 + int(sm["resolved"]) * 72].numpy().view(ro.capi.RAW_CAPTURE_DTYPE)
                arena = h_out[64 + dir_bytes:].numpy().view(np.float32)
                assert len(got["a"]) == int(sm["captured"]) == d.size > 0 and int(sm["lost"]) == 0, (len(got["a"]), sm)
                straddle = 0
                for (f, ln, floats), e in zip(got["a"], d):
                    assert (int(e["first_sample"]), int(e["samples"])) == (f, ln), "the legs disagree"
                    assert np.array_equal(arena[int(e["offset"]):int(e["offset"]) + 2 * ln], floats.reshape(-1)), "the legs disagree"
                    straddle += f < firsts[1] < f + ln
                a, b = [], []
                for _ in range(args.repeats):
                    a.append(window(leg_a, args.window) * 1e6)
                    b.append(window(leg_b, args.window) * 1e6)
                say("%s, %s samples: %d snapshots of %d rows in the directory, %d raw runs complete (%d across the buffers' seam, "
                    "%.1f MB of float pairs), %d pending" % (name, fmt_name, events, SNAP, int(sm["captured"]), straddle,
                                                           int(sm["arena_floats"]) * 4 / 1e6, int(sm["pending"])))
                for tag, what, t in (("a", "directory, wait, a copy per event, convert on the host", a),
                                     ("b", "raw call, summary, wait, what is in use               ", b)):
                    say("  leg %s  %s median %9.1f us   min %9.1f   max %9.1f   (%s)" % (
                        tag, what, np.median(t), min(t), max(t), " ".join("%.1f" % x for x in t)))
                say("  a / b = %.2f (medians)" % (np.median(a) / np.median(b)))
                say()
                del h_runs, h_out, d_out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
