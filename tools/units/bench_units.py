#!/usr/bin/env python3
"""What it costs to get a chunk's event files to the host as FITS data units: the arenas downloaded whole and cut, swapped and
padded on the host, against ro_stft_snapshot_units_resident / ro_stft_raw_units_resident (csrc/ro_units.hip).

One step is one chunk of 4096 rows at the headline shape (32768 bins, 75 % overlap, 48 kHz) whose snapshot arena and raw
arena are already on the device with their directories and summaries, as ro_stft_snapshots_resident and
ro_stft_raw_resident leave them (synthetic: snapshots of 40 rows, raw runs of 384000 samples; no transform and none of those
calls runs here).  Legs:
  a   the parent's way: the two summaries and directories to pinned host memory, SYNCHRONISE, the arena floats in use,
      synchronise; then per captured entry the cut to its recorder's columns and astype('>f4') into a zero-padded buffer
      (numpy, one host thread)
  b   the two unit calls, the two unit summaries to pinned host memory, SYNCHRONISE, the unit directories and the units in
      use; synchronise
Both are wall-clock times of the host thread from the first call to the end of the last wait or conversion: what is left
after either is one fwrite per file behind its header.  Two settings -- one detector whose recorder keeps all 615 columns of
the image (nothing is cut), and eight detectors of 256 columns each in a 2048-column image -- with 4 and with 64 events in
the chunk, the images alone, the raw runs alone and both.  Five alternations of the legs, each a window of at least
`--window` seconds.  The legs must give the same bytes; the tool checks it.  The report goes to stdout and to `--out`.

    python tools/units/bench_units.py [--window 0.3] [--repeats 5] [--out profiles/fits_units.txt]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

RATE = 48000
SNAP = 40                                                    # rows of a snapshot: 40 / 5 x 48000 = 384000 samples of raw I/Q
BLOCK = 2880
SETTINGS = [("one detector, 615 columns, nothing cut", 615, [(0, 615)]),
            ("eight detectors of 256 columns in a 2048-column image", 2048, [(256 * s, 256) for s in range(8)])]
DENSITIES = [("few events", 4), ("many events", 64)]

EXPECTATION = """\
Expectation, written down before the first run
==============================================
Nobody has measured either leg.  Per event the image is 40 rows of the image's columns (98 KB at 615 columns, 328 KB at
2048) and the raw run 384000 float pairs, 3.07 MB: the raw runs are 9 to 30 times the images' bytes, so "both" is the raw
runs' time in either leg.  The device's part of leg b is small (every byte is read once and written once at HBM rates, a
few microseconds per event); what the host sees is the download, which should dominate leg b.  Leg a downloads the arenas
and then makes the pass FITSWriter makes: a strided cut and a byte swap of every float on one host thread
(profiles/raw_capture.txt has this kind of pass costing more than the download it follows).  So: where nothing is cut (615
of 615 columns, and every raw run) leg b should be ahead by the host's swap pass, a factor of 2 to 4; with eight recorders
sharing a 2048-column image leg a downloads eight recorders' columns to keep one, and leg b should be ahead on the images
by about the cut factor, 8, times what the swap pass adds -- on a part that is a tenth of the bytes, so hardly visible in
"both".  With 4 events the images' legs are a few calls and waits each and the difference should be small in absolute terms
(tens of microseconds).  Nothing is gated on these numbers.
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


def padded(nbytes):
    return -(-nbytes // BLOCK) * BLOCK


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def pinned(nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()

    say(EXPECTATION)
    say("Measured (%s, %d alternations, windows of >= %.1f s, snapshots of %d rows, raw runs of %d samples)" % (
        torch.cuda.get_device_name(0), args.repeats, args.window, SNAP, int(SNAP / 5.0 * RATE)))
    say("=" * 100)
    stream = torch.cuda.current_stream().cuda_stream
    L = int(SNAP / 5.0 * RATE)
    with ro.Stft(bins=32768, overlap=24576, sample_rate=RATE) as st:
        for setting, cols, windows in SETTINGS:
            for name, events in DENSITIES:
                rng = np.random.default_rng(events)
                # what the snapshots call and the raw call leave: directories, summaries, packed arenas
                snap_dir = np.zeros(events, ro.capi.SNAPSHOT_DTYPE)
                snap_dir["rows"], snap_dir["status"] = SNAP, ro.RO_SNAP_CAPTURED
                snap_dir["slot"] = np.arange(events) % len(windows)
                snap_dir["offset"] = np.arange(events) * SNAP * cols
                snap_sum = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
                snap_sum["resolved"] = snap_sum["captured"] = events
                snap_sum["arena_floats"] = events * SNAP * cols
                raw_dir = np.zeros(events, ro.capi.RAW_CAPTURE_DTYPE)
                raw_dir["samples"], raw_dir["status"] = L, ro.RO_SNAP_CAPTURED
                raw_dir["slot"], raw_dir["offset"] = snap_dir["slot"], np.arange(events) * 2 * L
                raw_sum = np.zeros(1, ro.capi.RAW_SUMMARY_DTYPE)
                raw_sum["resolved"] = raw_sum["captured"] = events
                raw_sum["arena_floats"] = events * 2 * L
                src = {"images": (snap_dir, snap_sum, events * SNAP * cols), "raw runs": (raw_dir, raw_sum, events * 2 * L)}
                d_src, h_src, d_out, h_out, room = {}, {}, {}, {}, {}
                for part, (directory, summary, floats) in src.items():
                    arena = torch.from_numpy(rng.standard_normal(floats, dtype=np.float32)).cuda()
                    d_src[part] = (dev(directory), dev(summary), arena)
                    h_src[part] = (pinned(directory.nbytes), pinned(64), pinned(4 * floats))
                    if part == "images":
                        room[part] = sum(padded(4 * SNAP * windows[s % len(windows)][1]) for s in range(events))
                    else:
                        room[part] = events * padded(8 * L)
                    d_out[part] = (torch.zeros(events * 32, dtype=torch.uint8, device="cuda"),
                                   torch.zeros(room[part], dtype=torch.uint8, device="cuda"),
                                   torch.zeros(64, dtype=torch.uint8, device="cuda"))
                    h_out[part] = (pinned(events * 32), pinned(room[part]), pinned(64))
                host_units = {part: np.zeros(room[part], np.uint8) for part in src}      # leg a's padded buffers
                dtypes = {"images": (ro.capi.SNAPSHOT_DTYPE, ro.capi.SNAP_SUMMARY_DTYPE),
                          "raw runs": (ro.capi.RAW_CAPTURE_DTYPE, ro.capi.RAW_SUMMARY_DTYPE)}

                def leg_a(parts):
                    for part in parts:
                        h_src[part][1].copy_(d_src[part][1], non_blocking=True)
                        h_src[part][0].copy_(d_src[part][0], non_blocking=True)
                    torch.cuda.synchronize()
                    for part in parts:
                        used = int(h_src[part][1].numpy().view(dtypes[part][1])["arena_floats"][0]) * 4
                        h_src[part][2][:used].copy_(d_src[part][2].view(torch.uint8)[:used], non_blocking=True)
                    torch.cuda.synchronize()
                    for part in parts:
                        n = int(h_src[part][1].numpy().view(dtypes[part][1])["resolved"][0])
                        d = h_src[part][0].numpy().view(dtypes[part][0])[:n]
                        arena = h_src[part][2].numpy().view(np.float32)
                        out, at = host_units[part], 0
                        for e in d:
                            if e["status"] != ro.RO_SNAP_CAPTURED:
                                continue
                            o = int(e["offset"])
                            if part == "images":
                                first, wc = windows[int(e["slot"])]
                                cut = arena[o:o + int(e["rows"]) * cols].reshape(-1, cols)[:, first:first + wc]
                            else:
                                cut = arena[o:o + 2 * int(e["samples"])]
                            nbytes = 4 * cut.size
                            out[at:at + nbytes].view(">f4").reshape(cut.shape)[...] = cut
                            out[at + nbytes:at + padded(nbytes)] = 0
                            at += padded(nbytes)

                def leg_b(parts):
                    for part in parts:
                        d_dir, d_sum, d_arena = d_src[part]
                        u_dir, u_units, u_sum = d_out[part]
                        if part == "images":
                            st.snapshot_units_resident(d_dir, events, d_sum, d_arena, d_arena.numel(), cols, windows, u_dir, u_units,
                                                       room[part], u_sum, stream=stream)
                        else:
                            st.raw_units_resident(d_dir, events, d_sum, d_arena, d_arena.numel(), u_dir, u_units, room[part], u_sum,
                                                  stream=stream)
                        h_out[part][2].copy_(u_sum, non_blocking=True)
                    torch.cuda.synchronize()
                    for part in parts:
                        sm = h_out[part][2].numpy().view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
                        n, used = int(sm["entries"]) * 32, int(sm["units_bytes"])
                        h_out[part][0][:n].copy_(d_out[part][0][:n], non_blocking=True)
                        h_out[part][1][:used].copy_(d_out[part][1][:used], non_blocking=True)
                    torch.cuda.synchronize()

                both = ("images", "raw runs")
                leg_a(both)
                leg_b(both)
                for part in both:
                    sm = h_out[part][2].numpy().view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
                    assert int(sm["written"]) == events and int(sm["units_bytes"]) == room[part], sm
                    assert h_out[part][1].numpy()[:room[part]].tobytes() == host_units[part].tobytes(), "the legs disagree"
                say("%s; %s: %d events, images %.2f MB in the arena -> %.2f MB of units, raw runs %.1f MB -> %.1f MB" % (
                    setting, name, events, 4e-6 * events * SNAP * cols, 1e-6 * room["images"], 8e-6 * events * L,
                    1e-6 * room["raw runs"]))
                for parts, label in ((("images",), "images  "), (("raw runs",), "raw runs"), (both, "both    ")):
                    a, b = [], []
                    for _ in range(args.repeats):
                        a.append(window(lambda: leg_a(parts), args.window) * 1e6)
                        b.append(window(lambda: leg_b(parts), args.window) * 1e6)
                    for tag, what, t in (("a", "arenas to the host, cut + swap + pad there", a),
                                         ("b", "unit calls, summaries, wait, units in use ", b)):
                        say("  %s leg %s  %s median %10.1f us   min %10.1f   max %10.1f   (%s)" % (
                            label, tag, what, np.median(t), min(t), max(t), " ".join("%.1f" % x for x in t)))
                    say("  %s a / b = %.2f (medians)" % (label, np.median(a) / np.median(b)))
                say()
                del d_src, h_src, d_out, h_out, host_units
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
