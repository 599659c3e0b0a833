#!/usr/bin/env python3
"""A/B of the band-only transform against the full-row path serving the same consumer, on resident inputs.

  (a) run_resident: full rows + the snapshot tile + scan records  (what a host that feeds the recorders did before)
  (b) band_resident: the hull of tile and bands + scan records

One process; every shape is warmed up first; then the two legs alternate five times, each leg a HIP-event window of at
least 0.5 s of back-to-back launches.  Shapes: Bolidozor.json (65536 / 49152, 4096 rows, the hull of its bands and its
snapshot columns) and Ionozor.json's doppler configuration (524288 / 262144, 512 rows, 218 columns, no scan).

Prints, per shape: rows/s of each leg with the spread of the five repeats, the ratio b / a, the share of the HBM peak
the band's algorithmic bytes (hop x 8 + cols x 4 per row) make in (b), and the worst parity figure of both legs on the
first 8 rows (max |x - oracle| / max of the full oracle row).

    python tools/band/bench_band.py [--window 0.5] [--repeats 5] [--precision f32|f64] [--windows]

--precision f64: both legs on an RO_PRECISION_F64 handle, where (a) with tile = band is the only other way to serve the
consumer in the reference's arithmetic.  Shapes: Ionozor's doppler configuration as above, and 131072 / 98304, 2048 rows,
the 777-column hull of Bolidozor's bands at that size, with records.  The parity figure becomes per-bin:
max |x - oracle| / oracle over the band's bins of the first 8 rows.

--windows: the window-list call at the flagship shape, radio-observer.json (32768 / 24576, 4096 rows), whose hull of
1365 columns band_resident refuses: (a) as above with the 615-column snapshot tile and records, (b) band_windows_resident
over the windows ro_bands_windows gives for the bands and that tile (the noise band; the detect band with the tile), with
records.  Parity of (b) is taken on the tile's columns of its image and on the whole image.
"""
import argparse
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HBM_PEAK_GBS = 8000.0            # the figure bench.py uses (HBM3E spec)


def make_stream(torch, samples, bins, fs, first_col, cols, seed):
    """sigma = 1 noise + amplitude 300 some 5000 columns outside the band + amplitude 3 inside it, made on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    iq = torch.randn((samples, 2), generator=g, device="cuda", dtype=torch.float32)
    outside = first_col + cols + 5000 if first_col + cols + 5000 < bins else first_col - 5000
    for col, amp in ((outside + 0.21, 300.0), (first_col + cols // 2 + 0.37, 3.0)):
        w = 2.0 * math.pi * (col - bins / 2) / bins                       # radians per sample
        for lo in range(0, samples, 1 << 24):
            hi = min(samples, lo + (1 << 24))
            ph = torch.arange(lo, hi, device="cuda", dtype=torch.float64) * w
            iq[lo:hi, 0] += (amp * torch.cos(ph)).to(torch.float32)
            iq[lo:hi, 1] += (amp * torch.sin(ph)).to(torch.float32)
    return iq


def timed(torch, launch, window_s):
    """rows-independent: seconds per launch over a window of at least window_s"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    torch.cuda.synchronize()
    iters = max(2, int(math.ceil(window_s / max(e0.elapsed_time(e1) * 1e-3, 1e-6))) + 1)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    total = e0.elapsed_time(e1) * 1e-3
    return total / iters, total


def shape(torch, ro, oracle, name, bins, overlap, fs, rows, bands, tile, band, args, f64=False, windows=None):
    """windows (a list of (first_col, cols)): leg (b) is band_windows_resident over them; `band` is then the one of them
    that gets the signal's in-band tone"""
    hop = bins - overlap
    first_col, cols = band
    if windows is not None:
        cols = sum(n for _, n in windows)
        take = np.concatenate([np.arange(f, f + n) for f, n in windows])
    else:
        take = np.arange(first_col, first_col + cols)
    samples = (rows - 1) * hop + bins
    iq = make_stream(torch, samples, bins, fs, band[0], band[1], seed=bins)
    d_rows = torch.empty((rows, bins), dtype=torch.float32, device="cuda")
    d_tile = torch.empty((rows, tile[1]), dtype=torch.float32, device="cuda")
    d_band = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    rec_a = torch.zeros((rows, 3), dtype=torch.float32, device="cuda") if bands is not None else None
    rec_b = torch.zeros((rows, 3), dtype=torch.float32, device="cuda") if bands is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    kw = {"precision": ro.RO_PRECISION_F64} if f64 else {}
    with ro.Stft(bins=bins, overlap=overlap, sample_rate=fs, bands=bands, tile=tile, **kw) as st:
        def leg_a():
            st.run_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, d_tile=d_tile, d_records=rec_a, stream=stream)

        def leg_b():
            if windows is not None:
                st.band_windows_resident(iq, ro.RO_IQ_F32, samples, 0, rows, windows, d_band, d_records=rec_b, stream=stream)
            else:
                st.band_resident(iq, ro.RO_IQ_F32, samples, 0, rows, first_col, cols, d_band, d_records=rec_b, stream=stream)

        for _ in range(2):                                              # warm-up: tables, scratch, clocks
            leg_a()
            leg_b()
        torch.cuda.synchronize()
        ta, tb, shortest = [], [], 1e9
        for _ in range(args.repeats):
            for leg, acc in ((leg_a, ta), (leg_b, tb)):
                per, total = timed(torch, leg, args.window)
                acc.append(rows / per)
                shortest = min(shortest, total)
    ta, tb = np.array(ta), np.array(tb)
    # parity of both legs on the first 8 rows of the timed input
    n8 = min(8, rows)
    want = oracle.stft(iq[:(n8 - 1) * hop + bins].cpu().numpy(), bins, overlap, max_rows=n8).astype(np.float64)
    ref = want.max(axis=1)
    err_a = (np.abs(d_tile[:n8].cpu().numpy() - want[:, tile[0]:tile[0] + tile[1]]).max(axis=1) / ref).max()
    err_b = (np.abs(d_band[:n8].cpu().numpy() - want[:, take]).max(axis=1) / ref).max()
    if f64:                                                             # per bin, on the band's bins
        wa, wb = want[:, tile[0]:tile[0] + tile[1]], want[:, take]
        err_a = (np.abs(d_tile[:n8].cpu().numpy() - wa) / wa).max()
        err_b = (np.abs(d_band[:n8].cpu().numpy() - wb) / wb).max()
    same_peaks = ""
    if bands is not None:
        pa = rec_a.cpu().numpy().view(ro.capi.SCAN_DTYPE)["peak"].reshape(-1)
        pb = rec_b.cpu().numpy().view(ro.capi.SCAN_DTYPE)["peak"].reshape(-1)
        same_peaks = "   peaks equal on %d of %d rows" % (int((pa == pb).sum()), rows)
    alg = hop * 8 + cols * 4
    spread = lambda x: (x.max() - x.min()) / np.median(x)
    ratio = np.median(tb) / np.median(ta)
    what = "band [%d,+%d)" % (first_col, cols) if windows is None else \
        "windows %s (%d columns)" % (" ".join("[%d,+%d)" % w for w in windows), cols)
    print("%s: %d bins / overlap %d, %d rows, %s, tile [%d,+%d), shortest window %.2f s" %
          (name, bins, overlap, rows, what, tile[0], tile[1], shortest))
    print("  (a) full rows + tile%s: median %10.0f rows/s  (min %.0f, max %.0f, spread %.1f %%)" %
          (" + records" if bands is not None else "", np.median(ta), ta.min(), ta.max(), 100 * spread(ta)))
    print("  (b) band only%s:        median %10.0f rows/s  (min %.0f, max %.0f, spread %.1f %%)" %
          (" + records" if bands is not None else "", np.median(tb), tb.min(), tb.max(), 100 * spread(tb)))
    print("  b / a = %.2f   (slowest b / fastest a = %.2f)" % (ratio, tb.min() / ta.max()))
    print("  (b) algorithmic bytes %d per row: %.1f GB/s = %.3f of the %.0f GB/s HBM peak" %
          (alg, alg * np.median(tb) / 1e9, alg * np.median(tb) / 1e9 / HBM_PEAK_GBS, HBM_PEAK_GBS))
    print("  parity on the first %d rows, max err / %s: (a) %.2e  (b) %.2e%s" %
          (n8, "oracle, per bin" if f64 else "full row max", err_a, err_b, same_peaks))
    if windows is not None:                                             # the tile's columns, cut from (b)'s image
        at = int(np.searchsorted(take, tile[0]))
        assert (take[at:at + tile[1]] == np.arange(tile[0], tile[0] + tile[1])).all()
        err_t = (np.abs(d_band[:n8, at:at + tile[1]].cpu().numpy() - want[:, tile[0]:tile[0] + tile[1]]).max(axis=1) / ref).max()
        print("  (b) on the tile's columns alone: %.2e" % err_t)
    return tb.min() > ta.max()


def main_f64(torch, ro, oracle, args):
    ok = True
    fs = 96000
    # Ionozor.json:27-28, the doppler recorder's 40 Hz around 10.6 kHz: no scan
    bins, overlap = 524288, 262144
    band = (ro.frequency_to_bin(bins, fs, 10580.0), 218)
    ok &= shape(torch, ro, oracle, "Ionozor doppler (FP64)", bins, overlap, fs, max(8, int(512 * args.rows_scale)), None, band,
                band, args, f64=True)
    # Bolidozor.json:84-93's bands on a 131072-bin row: their hull is the band and the tile
    bins, overlap = 131072, 98304
    b = oracle.bolid_bands(bins, fs, overlap, 26450, 26550, 26000, 26300, 5, 2, 40)
    bands = ro.Bands(low_noise=b.low_noise, noise_width=b.noise_width, low_detect=b.low_detect,
                     detect_width=b.detect_width, avg_bins=b.avg_bins)
    band = ro.bands_hull(bands, bins)
    ok &= shape(torch, ro, oracle, "Bolidozor bands at 131072 (FP64)", bins, overlap, fs, max(8, int(2048 * args.rows_scale)),
                bands, band, band, args, f64=True)
    print("FP64 band only faster than FP64 full rows at both shapes by more than the repeats' spread: %s" % ("yes" if ok else "NO"))
    return 0


def main_windows(torch, ro, oracle, args):
    # radio-observer.json:62-87 (bands) and the snapshot's 10100 ... 11000 Hz
    bins, overlap, fs = 32768, 24576, 48000
    b = oracle.bolid_bands(bins, fs, overlap, 10300, 10900, 9000, 9600, 2, 5, 40)
    bands = ro.Bands(low_noise=b.low_noise, noise_width=b.noise_width, low_detect=b.low_detect,
                     detect_width=b.detect_width, avg_bins=b.avg_bins)
    t0, t1 = ro.frequency_to_bin(bins, fs, 10100.0), ro.frequency_to_bin(bins, fs, 11000.0)
    tile = (t0, t1 - t0)
    windows = [(w.first_col, w.cols) for w in ro.bands_windows(bands, bins, *tile)]
    hull = ro.bands_hull(bands, bins, *tile)
    assert ro.band_windows_supported(bins, windows) and not ro.band_supported(bins, hull[1])
    faster = shape(torch, ro, oracle, "radio-observer.json, window list", bins, overlap, fs, max(8, int(4096 * args.rows_scale)),
                   bands, tile, windows[-1], args, windows=windows)
    print("window list faster than full rows by more than the repeats' spread: %s" % ("yes" if faster else "NO"))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timed leg, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scale both row counts (quick runs)")
    ap.add_argument("--precision", choices=("f32", "f64"), default="f32", help="precision of the handle both legs run on")
    ap.add_argument("--windows", action="store_true", help="the window-list call at radio-observer.json's shape, nothing else")
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    import ro_oracle as oracle
    oracle.lib()
    ok = True
    if args.windows:
        return main_windows(torch, ro, oracle, args)
    if args.precision == "f64":
        return main_f64(torch, ro, oracle, args)
    # Bolidozor.json:45-46, :75-76 (snapshot columns), :84-93 (bands; avg_freq_range at its default of 40 Hz)
    bins, overlap, fs = 65536, 49152, 96000
    b = oracle.bolid_bands(bins, fs, overlap, 26450, 26550, 26000, 26300, 5, 2, 40)
    bands = ro.Bands(low_noise=b.low_noise, noise_width=b.noise_width, low_detect=b.low_detect,
                     detect_width=b.detect_width, avg_bins=b.avg_bins)
    t0, t1 = ro.frequency_to_bin(bins, fs, 26200.0), ro.frequency_to_bin(bins, fs, 26800.0)
    tile = (t0, t1 - t0)
    band = ro.bands_hull(bands, bins, *tile)
    ok &= shape(torch, ro, oracle, "Bolidozor", bins, overlap, fs, max(8, int(4096 * args.rows_scale)), bands, tile, band, args)
    # Ionozor.json:27-28, the doppler recorder's 40 Hz around 10.6 kHz: no scan
    bins, overlap = 524288, 262144
    band = (ro.frequency_to_bin(bins, fs, 10580.0), 218)
    ok &= shape(torch, ro, oracle, "Ionozor doppler", bins, overlap, fs, max(8, int(512 * args.rows_scale)), None, band, band, args)
    print("band only faster than full rows at both shapes by more than the repeats' spread: %s" % ("yes" if ok else "NO"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
