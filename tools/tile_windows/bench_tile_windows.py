#!/usr/bin/env python3
"""What cutting tile windows out of full rows costs (ro_stft_run_resident_windows, csrc/ro_cut_windows.hip), on resident
inputs at bench.py's default shape: 32768 bins, overlap 24576, 16384 rows, radio-observer.json's bands.

Legs, all on the same samples and the same row buffer:
  0  run_resident, records, no tile              the yardstick the cut's cost is taken against
  1  run_resident, records and the 615-column tile (the one tile of a handle: the fused epilogue writes it)
  2  run_resident_windows, radio-observer.json's two windows [22528,+409) [23278,+615)
  3  run_resident_windows, one 2048-column window [22528,+2048) (the bolid event band)
  4  run_resident_windows, 8 windows of 128 columns spread over the row

One process; every leg is warmed up first; then the legs alternate `--repeats` times, each leg a HIP-event window of at
least `--window` seconds of back-to-back launches.

The cut alone, as it runs in those calls -- behind a transform that has just written 2 GiB of rows, which are long out of
L2 -- is timed with a pair of events around it, and so is the standalone tile_kernel (ro_stft_time_resident's second
figure on an RO_PRECISION_F64 handle, whose plan does not fuse the tile) for a tile of as many columns.
`--tile-kernel-only` prints the tile_kernel figures alone and uses nothing the parent commit lacks; `--reference FILE`
takes the text of such a run of the parent commit into the report.  `--bench-ab FILE` takes bench.py result lines
("this <json>" / "parent <json>", alternated) into it.  The report goes to stdout and to `--out`.

    python tools/tile_windows/bench_tile_windows.py [--rows 16384] [--window 0.3] [--repeats 5] [--out profiles/tile_windows.txt]
"""
import argparse
import importlib
import json
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

BINS, OVERLAP = 32768, 24576
TILE = (23278, 615)
LISTS = [("two windows (radio-observer.json)", [(22528, 409), (23278, 615)]),
         ("one 2048-column window", [(22528, 2048)]),
         ("eight 128-column windows", [(2000 + 4000 * i, 128) for i in range(8)])]
TILE_COLS = (615, 1024, 2048)

EXPECTATION = """\
Expectation, written down before the first run
==============================================
cut_windows_kernel reads rows that the transform of the same call has just written: 16384 rows x 128 KiB = 2 GiB, long
out of the 32 MiB of L2 and out of the 256 MiB Infinity Cache by the time the cut gets to them -- what scan_sets_kernel
found for its bands (profiles/scan_sets.txt).  It moves 4 bytes in and 4 bytes out per wanted column and nothing else,
so it should cost ABOUT WHAT THE STANDALONE tile_kernel COSTS FOR THE SAME NUMBER OF COLUMNS ON THE SAME ROWS (both are
one dword per lane, consecutive lanes on consecutive columns): within +-30 % of it, and a few per cent of the call at most
(1024 columns are 1/32 of the bytes the transform writes).  The 8-window list reads 8 short runs per row instead of one or
two: more partly used cache lines, so somewhat more per column than the one-window list.  Legs 0 and 1 launch none of the
new code.  No pass / fail bar hangs on any of these numbers.
"""


def timed(torch, launch, window_s):
    """seconds per launch over a window of at least window_s"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch()                                   # (the first launch after another leg has been seen to take tens of ms)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(4):
        launch()
    e1.record()
    torch.cuda.synchronize()
    iters = max(2, int(math.ceil(window_s / max(e0.elapsed_time(e1) * 1e-3 / 4, 1e-6))) + 1)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    total = e0.elapsed_time(e1) * 1e-3
    return total / iters, total


def tile_kernel_ms(ro, torch, iq, samples, rows, d_rows, cols, iters=6):
    """the standalone tile_kernel behind a transform of the same rows: an FP64 handle does not fuse the tile, and
    ro_stft_time_resident's second figure is the time between the events around what follows the transform"""
    d_tile = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=BINS, overlap=OVERLAP, tile=(22528, cols), precision=ro.RO_PRECISION_F64) as st:
        st.time_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, 2, d_tile=d_tile)                 # warm-up
        _, _, behind = st.time_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, iters, d_tile=d_tile)
    return behind


def cut_ms(ro, torch, st, iq, samples, rows, d_rows, windows, d_image, stream, iters=12):
    """the cut behind a transform of the same rows, a pair of events around it"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in pairs:
        st.run_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, stream=stream)
        e0.record()
        st.cut_windows_resident(d_rows, rows, windows, d_image, stream=stream)
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in pairs[2:]]))


def bench_ab_section(path):
    runs = {"this": [], "parent": []}
    lines = []
    for line in open(path):
        m = re.match(r"\s*(this|parent)\s+(\{.*\})\s*$", line)
        if m:
            value = json.loads(m.group(2))["value"]
            runs[m.group(1)].append(value)
            lines.append("  %-6s %12.0f rows/s" % (m.group(1), value))
    out = ["bench.py's default line, this tree and the parent commit alternated on one device (`python bench.py --gpus 1`)",
           "=" * 110] + lines
    if runs["this"] and runs["parent"]:
        t, p = np.array(runs["this"]), np.array(runs["parent"])
        both = np.concatenate([t, p])
        out.append("  median of %d: this tree %.0f, parent %.0f rows/s: this / parent = %.4f; spread of the alternations (max - min) "
                   "/ median: this tree %.2f %%, parent %.2f %%, all runs %.2f %%" %
                   (len(t), np.median(t), np.median(p), np.median(t) / np.median(p), 100 * (t.max() - t.min()) / np.median(t),
                    100 * (p.max() - p.min()) / np.median(p), 100 * (both.max() - both.min()) / np.median(both)))
        moved = abs(np.median(t) / np.median(p) - 1) > (both.max() - both.min()) / np.median(both)
        out.append("  the default run launches none of the new code; moved beyond the spread of the alternations: %s" %
                   ("YES" if moved else "no"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of launches per timed leg, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_windows.txt"))
    ap.add_argument("--tile-kernel-only", action="store_true")
    ap.add_argument("--reference", default=None, help="text of a --tile-kernel-only run of the parent commit")
    ap.add_argument("--bench-ab", default=None, help="bench.py result lines, 'this <json>' / 'parent <json>'")
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    import ro_oracle as oracle
    rows = args.rows
    samples = (rows - 1) * (BINS - OVERLAP) + BINS
    g = torch.Generator(device="cuda")
    g.manual_seed(0xC3)
    iq = torch.randn((samples, 2), generator=g, device="cuda", dtype=torch.float32)
    d_rows = torch.empty((rows, BINS), dtype=torch.float32, device="cuda")
    if args.tile_kernel_only:
        for cols in TILE_COLS:
            print("tile_kernel %d columns: %.4f ms" % (cols, tile_kernel_ms(ro, torch, iq, samples, rows, d_rows, cols)))
        return 0
    b = oracle.bolid_bands(BINS, 48000, OVERLAP, 10300, 10900, 9000, 9600, 2, 5, 40)          # radio-observer.json:62-87
    bands = ro.Bands(low_noise=b.low_noise, noise_width=b.noise_width, low_detect=b.low_detect, detect_width=b.detect_width,
                     avg_bins=b.avg_bins)
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    d_tile = torch.empty((rows, TILE[1]), dtype=torch.float32, device="cuda")
    d_image = torch.empty((rows, 2048), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    plain = ro.Stft(bins=BINS, overlap=OVERLAP, bands=bands)
    tiled = ro.Stft(bins=BINS, overlap=OVERLAP, bands=bands, tile=TILE)
    legs = [("0 run_resident, no tile", lambda: plain.run_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, d_records=d_recs,
                                                                   stream=stream)),
            ("1 run_resident, 615-column tile", lambda: tiled.run_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows,
                                                                           d_tile=d_tile, d_records=d_recs, stream=stream))]
    for i, (name, windows) in enumerate(LISTS):
        legs.append(("%d windows: %s" % (2 + i, name),
                     lambda windows=windows: plain.run_resident_windows(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, windows,
                                                                        d_image, d_records=d_recs, stream=stream)))
    for _ in range(2):                                                  # warm-up: code objects, clocks
        for _, leg in legs:
            leg()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    shortest = 1e9
    for _ in range(args.repeats):
        for name, leg in legs:
            per, total = timed(torch, leg, args.window)
            times[name].append(per)
            shortest = min(shortest, total)
    med = {name: float(np.median(v)) for name, v in times.items()}
    out = ["$ python tools/tile_windows/bench_tile_windows.py", "", EXPECTATION,
           "Measured", "========",
           "%d bins / overlap %d, %d rows, radio-observer.json's bands; %d alternations, shortest window %.2f s" %
           (BINS, OVERLAP, rows, args.repeats, shortest)]
    base = med[legs[0][0]]
    for name, _ in legs:
        v = np.array(times[name])
        out.append("  %-46s median %8.4f ms  (min %.4f, max %.4f, spread %.1f %%)  %10.0f rows/s  %+.2f %% against leg 0" %
                   (name, 1e3 * med[name], 1e3 * v.min(), 1e3 * v.max(), 100 * (v.max() - v.min()) / med[name],
                    rows / med[name], 100 * (med[name] / base - 1)))
    spread0 = (max(times[legs[0][0]]) - min(times[legs[0][0]])) / base
    out += ["", "The cut and the standalone tile_kernel, each alone behind a transform of the same %d rows (events around it)" % rows,
            "-" * 110]
    tile_here = {cols: tile_kernel_ms(ro, torch, iq, samples, rows, d_rows, cols) for cols in TILE_COLS}
    tile_parent = {}
    if args.reference:
        text = open(args.reference).read()
        tile_parent = {int(c): float(ms) for c, ms in re.findall(r"tile_kernel (\d+) columns: ([0-9.]+) ms", text)}
    for cols in TILE_COLS:
        out.append("  tile_kernel, one run of %4d columns: %s%.4f ms on this tree (the kernel is the parent's, byte for byte)" %
                   (cols, "%.4f ms on the parent commit, " % tile_parent[cols] if cols in tile_parent else "", tile_here[cols]))
    held = True
    for (name, windows), leg in zip(LISTS, legs[2:]):
        total = sum(n for _, n in windows)
        ms = cut_ms(ro, torch, plain, iq, samples, rows, d_rows, windows, d_image, stream)
        ref_cols = min(TILE_COLS, key=lambda c: abs(c - total))
        ref = tile_parent.get(ref_cols, tile_here[ref_cols]) * total / ref_cols
        in_call = 1e3 * (med[leg[0]] - base)
        held &= 0.7 <= ms / ref <= 1.3
        out.append("  cut, %-34s %4d columns: %.4f ms = %.2f x tile_kernel for as many columns (%.4f ms from the %d-column "
                   "figure); in the call: %+.4f ms over leg 0 (whose own spread is %.4f ms)" %
                   (name + ",", total, ms, ms / ref, ref, ref_cols, in_call, 1e3 * spread0 * base))
    out += ["", "Expectation held (every cut within +-30 %% of tile_kernel for as many columns): %s" % ("yes" if held else "NO")]
    # the image is the rows' columns, bit for bit
    windows = LISTS[2][1]
    plain.run_resident_windows(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, windows, d_image, image_stride=d_image.shape[1],
                               d_records=d_recs, stream=stream)
    torch.cuda.synchronize()
    cols = torch.from_numpy(np.concatenate([np.arange(f, f + n) for f, n in windows])).cuda()
    same = torch.equal(d_image[:, :cols.numel()].view(torch.int32), d_rows[:, cols].view(torch.int32))
    out.append("image of the eight windows bit-identical to rows[:, columns]: %s" % ("yes" if same else "NO"))
    if args.bench_ab:
        out += [""] + bench_ab_section(args.bench_ab)
    plain.close()
    tiled.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
