"""GPU: C5 (BASELINE.json configs[4], the 8-hour stream of tests/test_gpu_c5.py: 168 747 rows of N = 32768 at 75 %
overlap) in RO_PRECISION_F64 on one handle, scan records on.  The FP64 records drive the product's BolidRecorder state
machine and, separately, the oracle FSM: the two event lists are equal, and equal the events of the float32 records of
the same stream.  The marginal rows of both modes -- where the detector's decision or peak bin hangs on the last bits --
are counted and printed."""
import ctypes as C

import numpy as np
import pytest

from util import C5_SAMPLES, JSON_BOLID, c5_slice

pytestmark = pytest.mark.gpu

BINS, OVERLAP, HOP, FS = 32768, 24576, 8192, 48000
BLOCK = 16384                      # rows per launch
RING = 2816                        # the row ring: ceil(60 s x 5.859 rows/s) x 8 (tests/test_gpu_c5.py)


def records_and_detect_band(ro, torch, precision, bands, iq, R):
    """(scan records [R] of SCAN_DTYPE, detect-band magnitudes [R, detect_width]) of one handle over the whole stream"""
    tile = (bands.low_detect, bands.detect_width)
    scratch = torch.empty((BLOCK, BINS), dtype=torch.float32, device="cuda")
    d_tile = torch.empty((R, tile[1]), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((R, 3), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with ro.Stft(bins=BINS, overlap=OVERLAP, bands=bands, tile=tile, precision=precision) as st:
        for b in range(0, R, BLOCK):
            n = min(BLOCK, R - b)
            st.run_resident(iq, ro.RO_IQ_F32, iq.shape[0], b, n, scratch, d_tile=d_tile[b:b + n],
                            d_records=d_recs[b:b + n], stream=s)
        torch.cuda.synchronize()
    recs = d_recs.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1).copy()
    band = d_tile.cpu().numpy()
    del scratch, d_tile, d_recs
    return recs, band


def marginal(recs, band):
    """rows where a / (2 n) lies within 1e-5 of 1 (the detection threshold) | rows whose two largest detect-band
    magnitudes lie within one float32 ulp (the peak bin)"""
    ratio = recs["average"].astype(np.float64) / (2.0 * recs["noise"].astype(np.float64))
    near_threshold = np.abs(ratio - 1.0) <= 1e-5
    top2 = -np.partition(-band, 1, axis=1)[:, :2]
    near_tie = (top2[:, 0] - top2[:, 1]) <= np.spacing(top2[:, 0])
    return near_threshold, near_tie


def oracle_events(ro, oracle, recs, bands, R):
    rate = ro.fft_sample_rate(FS, BINS, OVERLAP)
    f = oracle.BolidFsm(11, 29, rate, FS, 10300.0, 10900.0)
    out = []
    for i in range(R):
        ev = f.update(recs["noise"][i], recs["average"][i],
                      ro.bin_to_frequency(BINS, FS, bands.low_detect + int(recs["peak"][i])), (i + 1) % RING)
        if ev.fired:
            out.append((i, ev.snap_start, ev.snap_length, ev.peak_freq))
    return out


def product_events(recs, R):
    from hostlib import BolidEvent, host_library
    L = host_library()
    assert L is not None, "tests/harness/libro_host_harness.so missing: run __graft_entry__.build()"
    L.ro_host_bolid_replay.restype = C.c_int64
    L.ro_host_bolid_replay.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_int64,
                                       C.POINTER(BolidEvent), C.c_int]
    buf = (BolidEvent * 2048)()
    recs_c = np.ascontiguousarray(recs)
    n = L.ro_host_bolid_replay(BINS, OVERLAP, FS, JSON_BOLID["min_detect"], JSON_BOLID["max_detect"],
                               JSON_BOLID["min_noise"], JSON_BOLID["max_noise"], JSON_BOLID["advance_time"],
                               JSON_BOLID["jitter_time"], JSON_BOLID["avg_freq_range"], C.c_void_p(recs_c.ctypes.data),
                               R, buf, 2048)
    assert n <= 2048
    return [(buf[i].row, buf[i].start, buf[i].length, buf[i].peakFreq) for i in range(n)]


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return min(len(a), len(b)), a[len(b):len(b) + 1], b[len(a):len(a) + 1]


def test_c5_f64_events_equal_oracle_fsm_and_f32(ro, oracle, torch_cuda):
    from test_gpu_scan import json_bands
    torch = torch_cuda
    R = ro.row_count(C5_SAMPLES, BINS, OVERLAP)
    assert R == 168747
    bands = json_bands(ro, oracle)
    iq = c5_slice(torch, 0, C5_SAMPLES)
    rec64, band64 = records_and_detect_band(ro, torch, ro.RO_PRECISION_F64, bands, iq, R)
    rec32, band32 = records_and_detect_band(ro, torch, ro.RO_PRECISION_F32, bands, iq, R)
    del iq
    torch.cuda.empty_cache()
    thr64, tie64 = marginal(rec64, band64)
    thr32, tie32 = marginal(rec32, band32)
    print("C5 marginal rows, FP64: %d within 1e-5 of the threshold, %d with a peak tie within one ulp"
          % (thr64.sum(), tie64.sum()))
    print("C5 marginal rows, F32:  %d within 1e-5 of the threshold, %d with a peak tie within one ulp"
          % (thr32.sum(), tie32.sum()))
    det64 = rec64["average"].astype(np.float64) > 2.0 * rec64["noise"].astype(np.float64)
    det32 = rec32["average"].astype(np.float64) > 2.0 * rec32["noise"].astype(np.float64)
    print("C5 rows detected: FP64 %d, F32 %d, differing %d" % (det64.sum(), det32.sum(), (det64 != det32).sum()))

    def why(row):
        row = int(row)
        return "row %d (FP64 marginal: threshold %s, peak tie %s; F32 marginal: threshold %s, peak tie %s)" % (
            row, bool(thr64[row]), bool(tie64[row]), bool(thr32[row]), bool(tie32[row]))

    got = product_events(rec64, R)
    want = oracle_events(ro, oracle, rec64, bands, R)
    if got != want:
        i, x, y = first_difference(got, want)
        row = (x[0] if isinstance(x, tuple) else y[0]) if (x or y) else 0
        pytest.fail("FP64: product FSM and oracle FSM differ at event %d: %r vs %r -- %s" % (i, x, y, why(row)))
    want32 = oracle_events(ro, oracle, rec32, bands, R)
    if want != want32:
        i, x, y = first_difference(want, want32)
        row = (x[0] if isinstance(x, tuple) else y[0]) if (x or y) else 0
        pytest.fail("FP64 and F32 events differ at event %d: %r vs %r -- %s" % (i, x, y, why(row)))
    assert 959 <= len(want) <= 960
