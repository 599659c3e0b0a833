"""CPU-side checks of the detector (events from scan records, csrc/ro_events.hip): the new entry points exist, are bound and
refuse without a handle; ro_events_host against the oracle's transcription of BolidRecorder::update's state machine
(src/BolidRecorder.cpp:135, :171-267) with mark = row + 1, and against the closed form where the oracle's `int` ends; the
numpy restatement of the kernels' tile algebra (tools/events/emu_events.py); the kernels' emitted metadata.  Every
comparison is exact."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from eventslib import (GUARD, ROOT, bursts, closed_form, header_constant, host_call, marginal_numpy, oracle_events,
                       random_decisions, records_for, same_bytes)

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_events_host", "ro_stft_events_resident", "ro_stft_run_resident_events")
ADVANCES = (0, 3, 11)
JITTERS = (0, 1, 2, 3, 29)


def test_exports_and_abi(ro):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("ro_detector_t", "ro_event_t", "ro_detect_state_t", "ro_detect_summary_t"):
        assert re.search(r"\}\s*%s;" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    cfg = ro.capi.Config()
    cfg.struct_size = 1
    h = C.c_void_p()
    assert lib.ro_stft_create(C.byref(cfg), C.byref(h)) == -1
    m = re.search(rb"neither (\d+) \(ABI 2\)", lib.ro_last_error())
    assert m and int(m.group(1)) == C.sizeof(ro.capi.Config) == 96
    assert ro.capi.EVENT_DTYPE.itemsize == 40 and ro.EVENT_DTYPE is ro.capi.EVENT_DTYPE
    assert ro.capi.DETECT_STATE_DTYPE.itemsize == 32 and ro.capi.DETECT_SUMMARY_DTYPE.itemsize == 24
    assert C.sizeof(ro.capi.Detector) == 8
    assert callable(ro.events_host) and callable(ro.capi.events_host)
    for method in ("events_resident", "run_resident_events"):
        assert callable(getattr(ro.Stft, method)), method
    T, chunk = header_constant("RO_EVENTS_TILE_ROWS"), header_constant("RO_EVENTS_CHUNK_ROWS")
    assert T >= 64 and T % 64 == 0 and chunk % T == 0 and chunk > T


def test_struct_sizes_as_the_library_writes_them(ro):
    """40-byte events, a 32-byte state and a 24-byte summary: the library writes exactly these bytes and no others"""
    recs = records_for(ro, bursts(40, [(3, 2), (20, 1)]))
    state = np.full(3, GUARD, np.uint8).repeat(32).view(ro.capi.DETECT_STATE_DTYPE)      # entry 0 in use, 1 and 2 guards
    state[0] = np.zeros(1, ro.capi.DETECT_STATE_DTYPE)[0]
    summary = np.full(2 * 24, GUARD, np.uint8)
    events = np.full(4 * 40, GUARD, np.uint8)
    det = ro.capi.Detector(1, 3)
    rc = ro.library().ro_events_host(C.c_void_p(recs.ctypes.data), 1, 0, 40, C.byref(det), C.c_void_p(state.ctypes.data),
                                     C.c_void_p(events.ctypes.data), 4, C.c_void_p(summary.ctypes.data), None)
    assert rc == 0
    ev = events.view(ro.capi.EVENT_DTYPE)
    assert summary.view(ro.capi.DETECT_SUMMARY_DTYPE)[0].tolist() == (2, 3, 0) and np.all(summary[24:] == GUARD)
    assert ev["fire_row"][:2].tolist() == [7, 23] and ev["reserved"][:2].tolist() == [0, 0] and np.all(events[80:] == GUARD)
    assert ev["start_row"][:2].tolist() == [3, 20] and ev["length"][:2].tolist() == [4, 3]
    assert np.all(state.view(np.uint8)[32:] == GUARD) and not state.view(np.uint8)[:32].any()


@pytest.mark.parametrize("advance", ADVANCES)
@pytest.mark.parametrize("jitter", JITTERS)
def test_hand_made_sequences_against_the_oracle(ro, oracle, advance, jitter):
    G = max(2, jitter)
    det = (advance, jitter)

    def check(detect, events):
        recs = records_for(ro, detect, seed=advance * 100 + jitter)
        got, state, summary, dbytes = host_call(ro, recs, det)
        want, want_open = oracle_events(ro, oracle, recs, advance, jitter)
        assert same_bytes(got, want), (got, want)
        assert int(summary["events"]) == events == want.size
        assert int(summary["detect_rows"]) == int(np.count_nonzero(detect)) and np.array_equal(dbytes, detect)
        assert bool(state["open"][0]) == want_open
        cf, cf_state, _ = closed_form(ro, recs, advance, jitter)
        assert same_bytes(got, cf) and same_bytes(state, cf_state)
        return got, state, recs

    rows = 40 + 4 * G
    # a gap of exactly G - 1 quiet rows merges two bursts, a gap of exactly G splits them
    got, _, recs = check(bursts(rows, [(5, 3), (8 + G - 1, 2)]), 1)
    assert got[0]["fire_row"] == 8 + G - 1 + 1 + G and got[0]["length"] == 2 * advance + 3 + G - 1 + 2
    assert got[0]["start_row"] == 5 + 1 - advance and got[0]["peak"] == recs["peak"][5] and got[0]["noise"] == recs["noise"][5]
    got, _, recs = check(bursts(rows, [(5, 3), (8 + G, 2)]), 2)
    assert got["fire_row"].tolist() == [7 + G, 9 + G + G] and got["length"].tolist() == [2 * advance + 3, 2 * advance + 2]
    assert got[1]["magnitude"] == recs["average"][8 + G]
    # the fire row is the last row; one row fewer and the group stays open, and the next call's first row fires it
    d = bursts(9 + G, [(6, 3)])
    got, state, _ = check(d, 1)
    assert got[0]["fire_row"] == d.size - 1 and not state["open"][0]
    got, state, recs = check(d[:-1], 0)
    assert state["open"][0] == 1 and state["first_detect_row"][0] == 6 and state["last_detect_row"][0] == 8
    assert state["peak"][0] == recs["peak"][6] and state["noise"][0] == recs["noise"][6]
    more = records_for(ro, np.zeros(3, bool), seed=7)
    fired, state2, summary, _ = host_call(ro, more, det, first_row=d.size - 1, state=state.copy())
    assert fired.size == 1 and fired[0]["fire_row"] == d.size - 1 and fired[0]["start_row"] == 7 - advance
    assert fired[0]["length"] == 2 * advance + 3 and fired[0]["peak"] == recs["peak"][6] and not state2.view(np.uint8).any()
    # ... and a state whose group could no longer fire is closed silently
    fired, state2, summary, _ = host_call(ro, more, det, first_row=d.size, state=state.copy())
    assert fired.size == 0 and int(summary["events"]) == 0 and not state2.view(np.uint8).any()
    # all detect, no detect, and no rows at all
    _, state, _ = check(np.ones(50, bool), 0)
    assert state["open"][0] == 1 and state["first_detect_row"][0] == 0 and state["last_detect_row"][0] == 49
    _, state, _ = check(np.zeros(50, bool), 0)
    assert not state.view(np.uint8).any()
    keep = state2.copy()
    keep[0] = (4, 5, 1.0, 2, 3.0, 1)
    got, state, summary, _ = host_call(ro, records_for(ro, np.zeros(0, bool)), det, first_row=1000, state=keep.copy())
    assert got.size == 0 and same_bytes(state, keep) and summary.tolist() == (0, 0, 0)


def test_threshold_nan_and_inf(ro, oracle):
    """a == 2 n is no detect, the next float above is; NaN compares false (src/BolidRecorder.cpp:135 in double)"""
    two = np.float32(2.0)
    up = np.nextafter(two, np.float32(np.inf), dtype=np.float32)
    cases = [(1.0, two, 0), (1.0, up, 1), (1.0, np.nextafter(two, np.float32(0), dtype=np.float32), 0),
             (np.nan, 5.0, 0), (1.0, np.nan, 0), (np.nan, np.nan, 0), (1.0, np.inf, 1), (np.inf, np.inf, 0),
             (np.inf, 1.0, 0), (0.0, 0.0, 0), (0.0, 1.0, 1), (-1.0, -1.0, 1),
             (np.float32(1e-30), np.nextafter(np.float32(1e-30) * two, np.float32(1), dtype=np.float32), 1),
             (np.float32(3.4e38), np.float32(3.4e38), 0), (np.float32(1.7e38), np.float32(3.4e38), 0)]
    recs = np.zeros(len(cases) * 4, ro.capi.SCAN_DTYPE)
    recs["noise"], recs["average"] = 1.0, 1.0
    want = np.zeros(recs.size, np.uint8)
    for i, (n, a, d) in enumerate(cases):                   # every case followed by three quiet rows
        recs[4 * i] = (n, i, a)
        want[4 * i] = d
    for jitter in (0, 3):
        got, state, summary, dbytes = host_call(ro, recs, (2, jitter))
        assert np.array_equal(dbytes, want)
        ev, _ = oracle_events(ro, oracle, recs, 2, jitter)
        assert same_bytes(got, ev) and got.size == int(want.sum())
        assert got["peak"].tolist() == [i for i, c in enumerate(cases) if c[2]]
        assert np.isinf(got["magnitude"][got["peak"] == 6]).all()
        cf, cf_state, cf_detect = closed_form(ro, recs, 2, jitter)
        assert same_bytes(got, cf) and np.array_equal(cf_detect, want)


@pytest.mark.parametrize("seed", range(4))
def test_random_sequences_one_call_three_calls_oracle(ro, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    rows = int(rng.integers(1500, 4000))
    advance, jitter = int(rng.choice(ADVANCES)), int(rng.choice(JITTERS))
    recs = records_for(ro, random_decisions(rng, rows), seed=seed)
    want, want_open = oracle_events(ro, oracle, recs, advance, jitter)
    assert want.size > 10
    one, state1, summary1, detect1 = host_call(ro, recs, (advance, jitter))
    assert same_bytes(one, want) and bool(state1["open"][0]) == want_open
    cuts = sorted(int(c) for c in rng.integers(0, rows + 1, 2))
    parts, state, total = [], np.zeros(1, ro.capi.DETECT_STATE_DTYPE), np.zeros(3, np.int64)
    for lo, hi in zip([0] + cuts, cuts + [rows]):
        ev, state, summary, _ = host_call(ro, recs[lo:hi], (advance, jitter), first_row=lo, state=state)
        parts.append(ev)
        total += np.array(summary.tolist())
    assert same_bytes(np.concatenate(parts), one) and same_bytes(state, state1) and total.tolist() == list(summary1.tolist())
    # a column of a [row][set] array: the stride walks it
    wide = np.zeros((rows, 3), ro.capi.SCAN_DTYPE)
    wide[:, 1] = recs
    ev, st, sm, dt = host_call(ro, wide[:, 1], (advance, jitter))
    assert same_bytes(ev, one) and same_bytes(st, state1) and np.array_equal(dt, detect1)
    # the package's wrapper returns the same
    ev, st, sm, dt = ro.events_host(wide[:, 1], (advance, jitter), want_detect=True)
    assert same_bytes(ev, one) and same_bytes(st, state1) and sm.tolist() == summary1.tolist() and np.array_equal(dt, detect1)
    # where the oracle's int ends: rows from 2^33 on, against the closed form
    base = 2 ** 33
    far, far_state, _, _ = host_call(ro, recs, (advance, jitter), first_row=base)
    cf, cf_state, _ = closed_form(ro, recs, advance, jitter, first_row=base)
    assert same_bytes(far, cf) and same_bytes(far_state, cf_state)
    assert np.array_equal(far["fire_row"] - base, one["fire_row"]) and np.array_equal(far["length"], one["length"])


def test_marginal_rows(ro):
    rng = np.random.default_rng(5)
    n = (0.5 + rng.random(4000)).astype(np.float32)
    delta = np.concatenate([1e-5 * (1.0 + 1e-3 * rng.standard_normal(2000)), rng.uniform(-3e-5, 3e-5, 2000)])
    delta *= rng.choice([-1.0, 1.0], delta.size)
    recs = np.zeros(n.size, ro.capi.SCAN_DTYPE)
    recs["noise"] = n
    recs["average"] = (2.0 * n.astype(np.float64) * (1.0 + delta)).astype(np.float32)
    recs[:4] = [(0.0, 0, 0.0), (np.nan, 0, 1.0), (1.0, 0, np.inf), (1.0, 0, 2.0)]
    want = marginal_numpy(recs)
    assert 500 < np.count_nonzero(want) < 3500 and want[3] and not want[:3].any()
    _, _, summary, _ = host_call(ro, recs, (0, 2), capacity=0)
    assert int(summary["marginal_rows"]) == int(np.count_nonzero(want))


def test_capacity_smaller_than_the_events(ro, oracle):
    recs = records_for(ro, bursts(200, [(10 * i, 2) for i in range(1, 19)]))
    want, _ = oracle_events(ro, oracle, recs, 3, 2)
    assert want.size == 18
    for cap in (0, 1, 7, 18, 25):
        got, state, summary, _ = host_call(ro, recs, (3, 2), capacity=cap)         # (host_call checks the guards)
        assert int(summary["events"]) == 18 and same_bytes(got, want[:min(cap, 18)])


def test_refusals(ro):
    lib = ro.library()
    recs = records_for(ro, bursts(20, [(3, 2)]))
    state = np.zeros(1, ro.capi.DETECT_STATE_DTYPE)
    events = np.zeros(4, ro.capi.EVENT_DTYPE)
    p = lambda x: C.c_void_p(x.ctypes.data)

    def call(records=p(recs), stride=1, rows=20, det=ro.capi.Detector(1, 2), st=p(state), ev=p(events), cap=4):
        return lib.ro_events_host(records, stride, 0, rows, C.byref(det) if det is not None else None, st, ev, cap, None, None)
    assert call() == 0
    for bad in (dict(records=None), dict(stride=0), dict(rows=-1), dict(cap=-1), dict(det=None), dict(st=None),
                dict(ev=None), dict(det=ro.capi.Detector(-1, 2)), dict(det=ro.capi.Detector(1, -2))):
        assert call(**bad) == -1, bad
        assert lib.ro_last_error()
    assert call(ev=None, cap=0) == 0 and call(records=None, rows=0) == 0
    with pytest.raises(ro.StftError) as e:
        ro.events_host(recs, (1, -1))
    assert e.value.code == -1 and "jitter" in str(e.value)


def test_handle_calls_without_a_handle(ro):
    lib = ro.library()
    det = (ro.capi.Detector * 1)(ro.capi.Detector(1, 2))
    assert lib.ro_stft_events_resident(None, None, None, 0, 0, det, None, None, 0, None, None, None) == -1
    assert b"null handle" in lib.ro_last_error()
    assert lib.ro_stft_run_resident_events(None, None, 0, 0, 0, 0, None, 0, None, None, None, det, None, None, 0, None,
                                           None, None) == -1
    assert b"null handle" in lib.ro_last_error()


def test_the_emulator_of_the_kernels_runs_green(capsys):
    spec = importlib.util.spec_from_file_location("emu_events", os.path.join(ROOT, "tools", "events", "emu_events.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    assert emu.main(24) == 0
    assert capsys.readouterr().out.startswith("ok: 24 cases")


def test_events_kernels_build_pin(tmp_path):
    """three kernels; none spills or uses scratch; LDS is the few words the waves of a workgroup exchange"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_events.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_events.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.group_segment_fixed_size:\s*(\d+)[\s\S]*?\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)"
                         r"[\s\S]*?\.vgpr_count:\s*(\d+)[\s\S]*?\.vgpr_spill_count:\s*(\d+)", isa)
    seen = {}
    for lds, name, scratch, vgprs, spills in entries:
        short = re.search(r"events_[a-z]+_kernel", name).group(0)
        print("%s: %s VGPRs, LDS %s, scratch %s, spills %s" % (short, vgprs, lds, scratch, spills))
        assert (int(scratch), int(spills)) == (0, 0), short
        seen[short] = (int(lds), int(vgprs))
    assert sorted(seen) == ["events_emit_kernel", "events_reduce_kernel", "events_scan_kernel"], entries
    # LDS: four waves' summaries (48 bytes) and their counts (16 bytes each); one row or four tiles per lane fit in
    # a quarter of the 128 VGPRs that would still let eight waves share a SIMD
    assert seen["events_reduce_kernel"][0] == 96 and seen["events_scan_kernel"][0] == 96 and seen["events_emit_kernel"][0] == 64
    assert seen["events_reduce_kernel"][1] <= 32 and seen["events_emit_kernel"][1] <= 32 and seen["events_scan_kernel"][1] <= 64
    # the wave scans are DPP moves, as many ladders as there are scans
    assert len(re.findall(r"row_bcast:31", isa)) >= 3 * 3 and "ds_bpermute" in isa
