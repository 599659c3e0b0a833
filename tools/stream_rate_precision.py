#!/usr/bin/env python3
"""GPU box: rows/s through the reference's interface -- Frontend::process -> HipWaterfallBackend::process (vector<Complex>,
two doubles per sample) -> BolidRecorder::update per row -- at C3 (N = 32768, 75 % overlap, 48 kHz), in both precisions
(WaterfallConfig::precision), at the Backend's latency-bound default batch and at max_batch_rows = 256.  Shader clock
and package power from the amdgpu hwmon files (bench.py's sampler: plain reads, no settings touched) where the box has
them.  Reported in DESIGN.md §5; never the bench headline.

    python tools/stream_rate_precision.py [SECONDS]      (default 5 s per leg)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: one HIP runtime in the process)

import bench  # noqa: E402
import precisionlib as P  # noqa: E402

BINS, OVERLAP, FS, BLOCK = 32768, 24576, 48000, 4096


def leg(precision, max_batch_rows, seconds):
    sampler = bench.ClockPowerSampler(torch, 0)
    sampler.start()
    rc, s = P.stream_bench(precision, BINS, OVERLAP, FS, BLOCK, seconds, max_batch_rows, warm_calls=400)
    sampler.stop()
    late = [r for r in sampler.samples if r[0] > sampler.samples[0][0] + 0.4 * seconds] if sampler.samples else []
    mhz = np.array([r[1] for r in late], dtype=np.float64)
    w = np.array([r[2] for r in late], dtype=np.float64)
    rows_s = s["rows"] / s["seconds"]
    per_batch_host_us = 1e6 * s["seconds"] / max(s["batches"], 1) if s["batches"] else float("nan")
    name = "F64" if precision == P.RO_PRECISION_F64 else "F32"
    print("%s batch %-4s (%4d rows/launch): rc %d, %.4g rows/s (%.1f x real time), %d calls of %d samples, "
          "%.1f us per call (max %.2f ms), push %.1f us avg, %d batches, %.1f us of wall time per batch, GPU %.3f ms per timed batch; "
          "PCIe in %.2f GB/s; sclk %s MHz, package %s W"
          % (name, "dflt" if max_batch_rows == 0 else str(max_batch_rows), s["batch_rows"], rc, rows_s,
             rows_s / (FS / (BINS - OVERLAP)), s["calls"], BLOCK, 1e3 * s["call_ms_avg"], s["call_ms_max"],
             1e3 * s["push_ms_avg"], s["batches"], per_batch_host_us, s["batch_gpu_ms_avg"],
             rows_s * (BINS - OVERLAP) * (16 if precision == P.RO_PRECISION_F64 else 8) / 1e9,
             "%.0f" % np.nanmean(mhz) if len(mhz) else "n/a", "%.0f" % np.nanmean(w) if len(w) else "n/a"), flush=True)
    return rc, rows_s


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 5.0
    assert torch.cuda.is_available(), "needs the MI355X"
    P.require()
    print("# Backend::process rows/s at C3 (bins %d, overlap %d, %d Hz), blocks of %d Complex, %s"
          % (BINS, OVERLAP, FS, BLOCK, torch.cuda.get_device_name(0)), flush=True)
    res = {}
    bad = 0
    for mbr in (0, 256):
        for prec in (P.RO_PRECISION_F32, P.RO_PRECISION_F64):
            rc, r = leg(prec, mbr, seconds)
            bad += rc != 0
            res[(mbr, prec)] = r
    for mbr in (0, 256):
        print("# batch %s: F64 / F32 = %.3f" % ("dflt" if mbr == 0 else mbr,
                                                res[(mbr, P.RO_PRECISION_F64)] / res[(mbr, P.RO_PRECISION_F32)]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
