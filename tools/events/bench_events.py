#!/usr/bin/env python3
"""What it costs to know whether anything happened: events from scan records that are in HBM, the parent commit's way
against the device call (ro_stft_events_resident, csrc/ro_events.hip).

Legs, on the same records (uploaded once; no transform runs here):
  a  the parent's way: copy the records of every slot to pinned host memory, synchronise, run ro_events_host over each slot
  b  ro_stft_events_resident, then copy the summaries and the events (`--capacity` per slot) to pinned host memory, synchronise
Both are wall-clock times of the host thread from the first call to the end of the last wait: what stands between "the
rows are done" and "the host knows".  Leg b's GPU time (HIP events around the call) and, with `--kernel-stats DIR` (the
output directory of `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/events/bench_events.py
--kernels-only`), the three kernels' own times are reported beside it.

Shapes: 16384 rows x 1 slot (one benchmark step) and 168747 rows x 8 slots (config 5), both with detect rows like C5's
chirps: a burst every 176 rows, 3, 6, 12, 23 rows long in turn (0.5, 1, 2, 4 s every 30 s at 5.86 rows/s).  Five
alternations of the two legs, each leg a window of at least `--window` seconds.  Both legs must give the same events;
the tool checks it.  The report goes to stdout and to `--out`.

    python tools/events/bench_events.py [--window 0.3] [--repeats 5] [--out profiles/events.txt]
"""
import argparse
import csv
import glob
import importlib
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = [("one benchmark step", 16384, 1), ("config 5", 168747, 8)]
DETECTOR = (11, 29)                                          # radio-observer.json at 32768 bins, 75 % overlap

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Leg b is three small launches and two small copies.  At one benchmark step (16384 rows x 1 slot: 192 KiB of records, 64
tiles) every launch is shorter than its own launch latency, so the leg is bound by launch latency: a few tens of
microseconds, mostly the host's calls and the final wait.  At config 5 (168747 rows x 8 slots: 16 MB of records, 5280
tiles per tile pass) the two tile passes each read the 8 bytes of a 12-byte record they need, at a stride of 12 or 96
bytes, so they move the 16 MB about twice: at a few TB/s some tens of microseconds of GPU time -- a small fraction of
the 10 ms the transform of those rows takes at the headline rate.  Leg a has to bring the same 16 MB over the host link
(about 0.3 ms at 50 GB/s) and then walk 1.35 M records on one host thread (a few ns each: some ms); it should be one to
two orders of magnitude slower than leg b at config 5, and of the same order as leg b at one step, where both are a
handful of calls.  Nothing is gated on these numbers.
"""


def c5_like_records(ro, rows, slots, seed=0):
    rng = np.random.default_rng(seed)
    recs = np.zeros((rows, slots), ro.capi.SCAN_DTYPE)
    for s in range(slots):
        d = np.zeros(rows, bool)
        for i, first in enumerate(range(117 + 13 * s, rows, 176)):
            d[first:first + (3, 6, 12, 23)[i % 4]] = True
        recs["noise"][:, s] = (1.0 + rng.random(rows)).astype(np.float32)
        recs["average"][:, s] = recs["noise"][:, s] * np.where(d, np.float32(3.0), np.float32(1.5))
        recs["peak"][:, s] = rng.integers(0, 410, rows)
    return recs


def kernel_lines(directory):
    """the three kernels' own times from a rocprofv3 kernel trace of `--kernels-only` (20 calls per shape), per shape: the
    dispatches of a kernel are told apart by their grid (y = slots for the tile passes, x = 256 x slots for the scan)"""
    out = ["The three kernels alone, rocprofv3 --kernel-trace over 20 calls per shape (us):"]
    per = {}
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            m = re.search(r"events_[a-z]+_kernel", row["Kernel_Name"])
            if m:
                grid = (int(row["Grid_Size_X"]) // 256, int(row["Grid_Size_Y"]))
                per.setdefault((m.group(0), grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    order = {"events_reduce_kernel": 0, "events_scan_kernel": 1, "events_emit_kernel": 2}
    for (name, grid), t in sorted(per.items(), key=lambda kv: (kv[0][1][0] if kv[0][0] == "events_scan_kernel" else kv[0][1][1], order[kv[0][0]])):
        out.append("  %-22s %5d x %d workgroups  calls %3d  median %6.1f  min %6.1f  max %6.1f" % (
            name, grid[0], grid[1], len(t), np.median(t), min(t), max(t)))
    return out


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
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="20 device calls per shape and nothing else (to be traced)")
    ap.add_argument("--bench-ab", default=None, help='file of bench.py result lines, "this <json>" / "parent <json>"')
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(EXPECTATION)
    say("Measured (%s, %d alternations, windows of >= %.1f s, events kept per slot: %d)" % (
        torch.cuda.get_device_name(0), args.repeats, args.window, args.capacity))
    say("=" * 100)
    stream = torch.cuda.current_stream().cuda_stream
    for name, rows, slots in SHAPES:
        recs = c5_like_records(ro, rows, slots)
        bands = [ro.Bands(low_noise=2000 + 1000 * s, noise_width=409, low_detect=12000 + 1000 * s, detect_width=410, avg_bins=27)
                 for s in range(slots)]
        dets = [DETECTOR] * slots
        with ro.Stft(bins=32768, overlap=24576, bands=bands[0], extra_bands=bands[1:]) as st:
            d_primary = torch.from_numpy(np.ascontiguousarray(recs[:, 0]).view(np.uint8).reshape(-1)).cuda()
            d_extra = torch.from_numpy(np.ascontiguousarray(recs[:, 1:]).view(np.uint8).reshape(-1)).cuda() if slots > 1 else None
            h_primary = torch.empty(d_primary.shape, dtype=torch.uint8).pin_memory()
            h_extra = torch.empty(d_extra.shape, dtype=torch.uint8).pin_memory() if slots > 1 else None
            d_state = torch.zeros(slots * 32, dtype=torch.uint8, device="cuda")
            d_events = torch.zeros(slots * args.capacity * 40, dtype=torch.uint8, device="cuda")
            d_summary = torch.zeros(slots * 24, dtype=torch.uint8, device="cuda")
            h_events = torch.empty(d_events.shape, dtype=torch.uint8).pin_memory()
            h_summary = torch.empty(d_summary.shape, dtype=torch.uint8).pin_memory()
            host_out = {}

            def leg_a():
                h_primary.copy_(d_primary, non_blocking=True)
                if slots > 1:
                    h_extra.copy_(d_extra, non_blocking=True)
                torch.cuda.synchronize()
                p = h_primary.numpy().view(ro.capi.SCAN_DTYPE)
                e = h_extra.numpy().view(ro.capi.SCAN_DTYPE).reshape(rows, slots - 1) if slots > 1 else None
                for s in range(slots):
                    ev, _, sm, _ = ro.events_host(p if s == 0 else e[:, s - 1], dets[s], capacity=args.capacity)
                    host_out[s] = (ev, sm)

            def leg_b():
                d_state.zero_()
                st.events_resident(rows, dets, d_state, d_records=d_primary, d_extra=d_extra, d_events=d_events,
                                   capacity=args.capacity, d_summary=d_summary, stream=stream)
                h_summary.copy_(d_summary, non_blocking=True)
                h_events.copy_(d_events, non_blocking=True)
                torch.cuda.synchronize()

            if args.kernels_only:
                for _ in range(20):
                    leg_b()
                continue
            leg_a()
            leg_b()
            sm = h_summary.numpy().view(ro.capi.DETECT_SUMMARY_DTYPE)
            ev = h_events.numpy().view(ro.capi.EVENT_DTYPE).reshape(slots, args.capacity)
            for s in range(slots):
                n = int(host_out[s][1]["events"])
                assert sm[s].tolist() == host_out[s][1].tolist(), (s, sm[s], host_out[s][1])
                assert ev[s, :min(n, args.capacity)].tobytes() == host_out[s][0].tobytes(), "slot %d: the legs disagree" % s
            # leg b's GPU time alone: HIP events around the call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            gpu = []
            for _ in range(20):
                d_state.zero_()
                e0.record()
                st.events_resident(rows, dets, d_state, d_records=d_primary, d_extra=d_extra, d_events=d_events,
                                   capacity=args.capacity, d_summary=d_summary, stream=stream)
                e1.record()
                torch.cuda.synchronize()
                gpu.append(e0.elapsed_time(e1) * 1e3)
            a, b = [], []
            for _ in range(args.repeats):
                a.append(window(leg_a, args.window) * 1e6)
                b.append(window(leg_b, args.window) * 1e6)
            say("%s: %d rows x %d slot%s, %.2f MB of records, %d events in all" % (
                name, rows, slots, "s" if slots > 1 else "", rows * slots * 12 / 1e6, int(sm["events"].sum())))
            say("  leg a  records to the host + ro_events_host   median %10.1f us   min %10.1f   max %10.1f   (%s)" % (
                np.median(a), min(a), max(a), " ".join("%.1f" % x for x in a)))
            say("  leg b  ro_stft_events_resident + its results  median %10.1f us   min %10.1f   max %10.1f   (%s)" % (
                np.median(b), min(b), max(b), " ".join("%.1f" % x for x in b)))
            say("  leg b's three launches, HIP events around the call: median %.1f us, min %.1f, max %.1f (20 calls)" % (
                np.median(gpu), min(gpu), max(gpu)))
            say("  a / b = %.1f; leg b is %.2f %% of the %.2f ms the transform of these rows takes at 16.7 M rows/s" % (
                np.median(a) / np.median(b), 100 * np.median(b) * 1e-6 / (rows / 16.7e6), rows / 16.7e3))
            say()
    if args.kernels_only:
        return 0
    if args.kernel_stats:
        for text in kernel_lines(args.kernel_stats):
            say(text)
        say()
    if args.bench_ab:
        import json
        vals = {"this": [], "parent": []}
        for line in open(args.bench_ab):
            who, _, js = line.partition(" ")
            if who in vals and js.strip().startswith("{"):
                vals[who].append(json.loads(js)["value"])
        say("bench.py --gpus 1 (launches none of this), alternated with the parent commit, value per run:")
        for who in ("parent", "this"):
            say("  %-6s %s   median %.1f" % (who, " ".join("%.1f" % v for v in vals[who]), np.median(vals[who])))
        lo, hi = min(vals["parent"] + vals["this"]), max(vals["parent"] + vals["this"])
        say("  this / parent (medians) = %.4f; spread of all runs %.1f ... %.1f" % (
            np.median(vals["this"]) / np.median(vals["parent"]), lo, hi))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
