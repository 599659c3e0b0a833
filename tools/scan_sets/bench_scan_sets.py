#!/usr/bin/env python3
"""What an extra band set costs (ro_stft_set_extra_bands, csrc/ro_scan_sets.hip), on resident inputs at bench.py's
default shape: 32768 bins, overlap 24576, 16384 rows, radio-observer.json's bands as the primary set.

Legs, all on the same samples and the same row buffer:
  run_resident                      the call as it always was (transform with the fused primary scan)
  run_resident_sets, 0 extra sets   d_extra = NULL: the same kernels as run_resident
  run_resident_sets, 1 / 3 / 7      extra sets that are copies of the primary shifted by 1000 columns each
  scan_resident                     the existing scan_kernel alone on the rows: the yardstick for one set
  scan_sets_resident, 1 / 3 / 7     the new kernel alone on the rows

One process; every leg is warmed up first; then the legs alternate `--repeats` times, each leg a HIP-event window of at
least `--window` seconds of back-to-back launches.  Prints the median time per launch of every leg with the spread of
the repeats, the cost per extra set ((t_k - t_0) / k) against the standalone scan of one set, and checks that every
set's records equal the standalone scan of the same rows with that set as the primary.

    python tools/scan_sets/bench_scan_sets.py [--rows 16384] [--window 0.5] [--repeats 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timed leg, at least")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    ro = importlib.import_module("radio-observer_amd")
    import ro_oracle as oracle
    bins, overlap, rows = 32768, 24576, args.rows
    hop = bins - overlap
    samples = (rows - 1) * hop + bins
    b = oracle.bolid_bands(bins, 48000, overlap, 10300, 10900, 9000, 9600, 2, 5, 40)          # radio-observer.json:62-87

    def shifted(k):
        return ro.Bands(low_noise=b.low_noise - 1000 * k, noise_width=b.noise_width, low_detect=b.low_detect - 1000 * k,
                        detect_width=b.detect_width, avg_bins=b.avg_bins)

    g = torch.Generator(device="cuda")
    g.manual_seed(0xC3)
    iq = torch.randn((samples, 2), generator=g, device="cuda", dtype=torch.float32)
    d_rows = torch.empty((rows, bins), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    d_extra = torch.zeros((rows * 7, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    counts = (0, 1, 3, 7)
    handles = {k: ro.Stft(bins=bins, overlap=overlap, bands=shifted(0), extra_bands=[shifted(1 + i) for i in range(k)])
               for k in counts}
    legs = [("run_resident", lambda: handles[0].run_resident(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, d_records=d_recs,
                                                           stream=stream))]
    for k in counts:
        legs.append(("run_resident_sets, %d extra" % k,
                     lambda k=k: handles[k].run_resident_sets(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, d_records=d_recs,
                                                              d_extra=d_extra if k else None, stream=stream)))
    legs.append(("scan_resident", lambda: handles[0].scan_resident(d_rows, rows, d_recs, stream=stream)))
    for k in counts[1:]:
        legs.append(("scan_sets_resident, %d extra" % k,
                     lambda k=k: handles[k].scan_sets_resident(d_rows, rows, d_extra, stream=stream)))
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
    print("32768 bins / overlap %d, %d rows, primary bands %d/%d/%d/%d/%d, extra sets shifted down by 1000 columns each; "
          "%d repeats, shortest window %.2f s" % (overlap, rows, b.low_noise, b.noise_width, b.low_detect, b.detect_width,
                                                  b.avg_bins, args.repeats, shortest))
    for name, _ in legs:
        v = np.array(times[name])
        print("  %-30s median %9.3f ms  (min %.3f, max %.3f, spread %.1f %%)  %10.0f rows/s" %
              (name, 1e3 * med[name], 1e3 * v.min(), 1e3 * v.max(), 100 * (v.max() - v.min()) / med[name], rows / med[name]))
    t0, scan = med["run_resident_sets, 0 extra"], med["scan_resident"]
    print("  run_resident_sets(d_extra = NULL) / run_resident = %.4f" % (t0 / med["run_resident"]))
    for k in counts[1:]:
        per_set = (med["run_resident_sets, %d extra" % k] - t0) / k
        alone = med["scan_sets_resident, %d extra" % k] / k
        print("  %d extra sets: %+.3f ms per set behind the transform = %.2f x the standalone scan of one set (%.3f ms); "
              "the new kernel alone: %.3f ms per set = %.2f x; whole call %+.2f %%" %
              (k, 1e3 * per_set, per_set / scan, 1e3 * scan, 1e3 * alone, alone / scan,
               100 * (med["run_resident_sets, %d extra" % k] / t0 - 1)))
    # every set's records == the standalone scan of the same rows with that set as the primary
    handles[7].run_resident_sets(iq, ro.RO_IQ_F32, samples, 0, rows, d_rows, d_records=d_recs, d_extra=d_extra, stream=stream)
    torch.cuda.synchronize()
    extra = d_extra.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(rows, 7)
    d_one = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    ok = True
    for i in range(7):
        with ro.Stft(bins=bins, overlap=overlap, bands=shifted(1 + i)) as one:
            one.scan_resident(d_rows, rows, d_one, stream=stream)
            torch.cuda.synchronize()
        want = d_one.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1)
        ok &= all(np.array_equal(extra[:, i][f].view(np.uint32), want[f].view(np.uint32)) for f in ("noise", "peak", "average"))
    print("  records of the 7 extra sets bit-identical to scan_resident with each set as the primary: %s" % ("yes" if ok else "NO"))
    for h in handles.values():
        h.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
