"""CPU-side checks of several band sets per row (ro_stft_set_extra_bands, csrc/ro_scan_sets.hip): the new entry points
of the C ABI exist, are bound and refuse without a device; the host mirror hands every detector its own scan record
(the reference calls every recorder for every row, src/WaterfallBackend.cpp:534-536, and each BolidRecorder derives its own
bands, src/BolidRecorder.cpp:84-104); the new kernel's emitted metadata."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from detectorslib import ManualDetectors, detectors_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_stft_set_extra_bands", "ro_stft_extra_bands", "ro_stft_run_resident_sets", "ro_stft_scan_sets_resident",
       "ro_stft_fetch_sets")
A_FREQS = (10300.0, 10900.0, 9000.0, 9600.0)            # radio-observer.json:62-87
B_FREQS = (5300.0, 5900.0, 4000.0, 4600.0)


@pytest.fixture(scope="module")
def D():
    if detectors_library() is None:
        pytest.fail("tests/harness_detectors/libro_detectors_harness.so missing: run __graft_entry__.build()")
    return detectors_library()


def test_new_symbols_exist_and_are_bound(ro):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"#define\s+RO_MAX_EXTRA_BANDS\s+7\b", header) and ro.capi.RO_MAX_EXTRA_BANDS == 7
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    for method in ("set_extra_bands", "run_resident_sets", "scan_sets_resident", "fetch_sets"):
        assert callable(getattr(ro.Stft, method))


def test_new_calls_without_a_handle_or_a_device(ro):
    """A null handle is RO_ERR_INVALID for every new call, like the calls they extend.  Without a device the way to a
    handle ends in ro_stft_create's RO_ERR_HIP -- also with extra_bands, which are applied after creation: there is no
    host-side scan to fall back to."""
    import torch
    lib = ro.library()
    b = ro.Bands(low_noise=0, noise_width=8, low_detect=16, detect_width=8, avg_bins=3)
    n64 = C.c_int64(7)
    assert lib.ro_stft_set_extra_bands(None, C.byref(b), 1) == -1
    assert lib.ro_stft_set_extra_bands(None, None, 0) == -1
    assert lib.ro_stft_extra_bands(None, None) == -1
    assert lib.ro_stft_run_resident_sets(None, None, 0, 0, 0, 0, None, 0, None, None, None, None) == -1
    assert lib.ro_stft_scan_sets_resident(None, None, 0, 0, None, None, None) == -1
    assert lib.ro_stft_fetch_sets(None, 1, 0, 0, None, None, None, None, C.byref(n64)) == -1 and n64.value == 7
    assert b"null" in lib.ro_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(ro.StftError) as e:
            ro.Stft(bins=1024, overlap=512, bands=b, extra_bands=[b, b])
        assert e.value.code == -3                            # RO_ERR_HIP


def bursts(rows, first, last, seed, detect_width):
    """a record stream whose average crosses twice the noise on rows [first, last]"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rows):
        n = np.float32(1.0 + 0.1 * rng.random())
        a = np.float32(n * (3.0 if first <= r <= last else 1.5))
        out.append((n, int(rng.integers(0, detect_width)), a))
    return out


def fsm_events(oracle, bins, overlap, rate, freqs, adv_t, jit_t, avg, cap, stream):
    b = oracle.bolid_bands(bins, rate, overlap, freqs[0], freqs[1], freqs[2], freqs[3], adv_t, jit_t, avg)
    fft_rate = oracle.lib().ro_oracle_fft_sample_rate(rate, bins, overlap)
    fsm = oracle.BolidFsm(b.advance, b.jitter, fft_rate, rate, freqs[0], freqs[1])
    out = []
    for i, (n, p, a) in enumerate(stream):
        fq = oracle.lib().ro_oracle_bin_to_frequency(bins, rate, b.low_detect + int(p))
        ev = fsm.update(n, a, fq, (i + 1) % cap)
        if ev.fired:
            out.append((i, ev.snap_start, ev.snap_length, ev.raw_length, ev.duration_s, ev.noise, ev.peak_freq,
                        ev.magnitude, ev.fmin, ev.fmax))
    return out, b, fsm.f.state


def as_tuples(events):
    return [(e.row, e.start, e.length, e.rawLength, e.duration, e.noise, e.peakFreq, e.magnitude, e.fmin, e.fmax)
            for e in events]


def test_two_detectors_each_see_their_own_record(D, oracle):
    """Two detectors on one ManualWaterfall, fed different record streams: each event list is the oracle's FSM on that
    detector's stream, with peakFreq from that detector's own lowDetectBin_.  (With one record per row shared by all
    detectors, both lists would be the first stream's.)"""
    bins, overlap, rate, rows = 32768, 24576, 48000, 120
    m = ManualDetectors(bins, overlap, [A_FREQS, B_FREQS], advance_time=0.5, jitter_time=1.0)
    assert m.started and m.error == "" and m.scan_enabled() and m.extra_sets() == 1
    ba, bb = m.bands(0), m.bands(1)
    assert (ba[7], bb[7]) == (0, 1)                                          # scan slots in addRecorder order
    assert ba[:4] == (23415, 410, 22528, 409) and bb[:4] == (20002, 409, 19114, 410) and ba[6] == bb[6] == 27
    sa = bursts(rows, 20, 30, 1, ba[1])
    sb = bursts(rows, 60, 65, 2, bb[1])
    for r in range(rows):
        m.push([sa[r], sb[r]])
    cap = m.ring_capacity()
    want_a, oa, state_a = fsm_events(oracle, bins, overlap, rate, A_FREQS, 0.5, 1.0, 40, cap, sa)
    want_b, ob, state_b = fsm_events(oracle, bins, overlap, rate, B_FREQS, 0.5, 1.0, 40, cap, sb)
    assert (oa.low_detect, ob.low_detect) == (ba[0], bb[0])
    got_a, got_b = as_tuples(m.events(0)), as_tuples(m.events(1))
    assert len(want_a) == 1 and len(want_b) == 1
    assert got_a == want_a and got_b == want_b and got_a != got_b
    assert (m.state(0), m.state(1)) == (state_a, state_b)
    # the event's frequency is a bin of the detector's OWN band
    lib = oracle.lib()
    for got, lo, width in ((got_a, ba[0], ba[1]), (got_b, bb[0], bb[1])):
        fqs = {lib.ro_oracle_bin_to_frequency(bins, rate, lo + p) for p in range(width)}
        assert got[0][6] in fqs
    assert got_b[0][6] < 6000.0 < got_a[0][6]
    m.close()


def test_a_ninth_detector_is_refused_and_one_detector_is_as_before(D, oracle):
    bins, overlap, rate = 32768, 24576, 48000
    freqs = [(1000.0 * k + 300.0, 1000.0 * k + 900.0, 1000.0 * k - 1000.0, 1000.0 * k - 400.0) for k in range(2, 11)]
    m8 = ManualDetectors(bins, overlap, freqs[:8])
    assert m8.started and m8.error == "" and m8.extra_sets() == 7
    assert [m8.bands(i)[7] for i in range(8)] == list(range(8))
    m8.close()
    m9 = ManualDetectors(bins, overlap, freqs)
    assert not m9.started and not m9.scan_enabled() and m9.extra_sets() == 0
    assert "more than 8 detectors" in m9.error and "RO_MAX_EXTRA_BANDS = 7" in m9.error
    m9.push([(1.0, 0, 5.0)] * 8)                             # no detector runs on somebody else's record
    assert all(m9.state(i) == 0 and m9.events(i) == [] for i in range(9))
    m9.close()
    # one detector, rows through the pushRow signature that has one record: the oracle's FSM, as ever
    m1 = ManualDetectors(bins, overlap, [A_FREQS], advance_time=0.5, jitter_time=1.0)
    assert m1.started and m1.extra_sets() == 0 and m1.bands(0)[7] == 0
    s = bursts(100, 20, 30, 3, m1.bands(0)[1])
    for n, p, a in s:
        m1.push_single(float(n), p, float(a))
    want, _, state = fsm_events(oracle, bins, overlap, rate, A_FREQS, 0.5, 1.0, 40, m1.ring_capacity(), s)
    assert len(want) == 1 and as_tuples(m1.events(0)) == want and m1.state(0) == state
    m1.close()


def test_scan_sets_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_scan_sets.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_scan_sets.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)", isa)
    # the three register forms launch_scan_sets chooses between
    assert len(entries) == 3 and all("scan_sets_kernel" in n for n, _ in entries), entries
    bad = [(n, int(s)) for n, s in entries if int(s) != 0]
    assert not bad, bad
