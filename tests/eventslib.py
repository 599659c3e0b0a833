"""What tests/test_events_cpu.py and tests/test_gpu_events.py share (test infrastructure): records with a wanted decision
per row, the oracle's state machine driven with mark = row + 1, the closed form of include/ro_stft.h restated group by
group, and the raw ro_events_host call with guard entries behind its outputs."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5                                              # every byte of a guard entry


def header_constant(name):
    """an integer #define of csrc/ro_events.h"""
    text = open(os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_events.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)\b" % name, text).group(1))


def records_for(ro, detect, seed=0):
    """SCAN_DTYPE records whose decision is `detect`: noise in [1, 2), average 3 n or 1.5 n, a peak that names the row"""
    detect = np.asarray(detect, bool)
    rng = np.random.default_rng(seed)
    recs = np.zeros(detect.size, ro.capi.SCAN_DTYPE)
    recs["noise"] = (1.0 + rng.random(detect.size)).astype(np.float32)
    recs["average"] = recs["noise"] * np.where(detect, np.float32(3.0), np.float32(1.5)).astype(np.float32)
    recs["peak"] = rng.integers(0, 400, detect.size)
    return recs


def bursts(rows, spans):
    """detect rows: [(first, count), ...] -> bool[rows]"""
    d = np.zeros(rows, bool)
    for lo, n in spans:
        d[lo:lo + n] = True
    return d


def random_decisions(rng, rows, gaps=(1, 1, 2, 2, 3, 4, 5, 28, 29, 30, 70, 300)):
    d = np.zeros(rows, bool)
    pos = int(rng.integers(0, 6))
    while pos < rows:
        n = int(rng.choice([1, 1, 2, 3, 7, 40]))
        d[pos:pos + n] = True
        pos += n + int(rng.choice(gaps))
    return d


def events_array(ro, tuples):
    out = np.zeros(len(tuples), ro.capi.EVENT_DTYPE)
    for i, t in enumerate(tuples):
        out[i] = tuple(t) + (0,)
    return out


def oracle_events(ro, oracle, recs, advance, jitter):
    """EVENT_DTYPE array of what oracle.BolidFsm fires over `recs` as rows 0, 1, ... with mark = row + 1 (buffer_->mark(),
    unwrapped); the peak column travels as the machine's peak frequency (small integers are exact floats).  Also whether
    the machine ends outside STATE_INIT."""
    f = oracle.BolidFsm(advance, jitter, 1.0, 48000, 0.0, 0.0)
    out = []
    for r in range(recs.size):
        ev = f.update(recs["noise"][r], recs["average"][r], float(recs["peak"][r]), r + 1)
        if ev.fired:
            out.append((r, ev.snap_start, ev.snap_length, np.float32(ev.noise), int(ev.peak_freq), np.float32(ev.magnitude)))
    return events_array(ro, out), f.f.state != 0


def closed_form(ro, recs, advance, jitter, first_row=0):
    """The closed form, group by group (not row by row as the library's host call does it): detect rows whose gaps are at
    most G - 1 quiet rows form a group; it fires at last + G if that row has been seen.  Returns (events, state, detect)."""
    G = max(2, jitter)
    n, a = recs["noise"].astype(np.float64), recs["average"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        detect = a > n * 2.0
    rows = np.flatnonzero(detect)
    state = np.zeros(1, ro.capi.DETECT_STATE_DTYPE)
    if rows.size == 0:
        return events_array(ro, []), state, detect.astype(np.uint8)
    cuts = np.flatnonzero(np.diff(rows) - 1 >= G) + 1
    out = []
    for grp in np.split(rows, cuts):
        r0, last = int(grp[0]), int(grp[-1])
        rec = recs[r0]
        if last + G < recs.size:
            out.append((first_row + last + G, first_row + r0 + 1 - advance, 2 * advance + last - r0 + 1, rec["noise"],
                        rec["peak"], rec["average"]))
        else:
            state[0] = (first_row + r0, first_row + last, rec["noise"], rec["peak"], rec["average"], 1)
    return events_array(ro, out), state, detect.astype(np.uint8)


def marginal_numpy(recs):
    """tests/test_gpu_precision_c5.py:42-43"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = recs["average"].astype(np.float64) / (2.0 * recs["noise"].astype(np.float64))
        return np.abs(ratio - 1.0) <= 1e-5


def host_call(ro, recs, detector, first_row=0, state=None, capacity=None, guard=3):
    """ro_events_host through ctypes with `guard` guard entries behind the events and guard bytes behind the decisions;
    returns (events written, state, summary, detect) after checking that every guard is intact"""
    rows = recs.size
    cap = rows if capacity is None else capacity
    state = np.zeros(1, ro.capi.DETECT_STATE_DTYPE) if state is None else state
    events = np.full((cap + guard) * ro.capi.EVENT_DTYPE.itemsize, GUARD, np.uint8)
    detect = np.full(rows + guard, GUARD, np.uint8)
    summary = np.zeros(1, ro.capi.DETECT_SUMMARY_DTYPE)
    det = ro.capi.Detector(*detector)
    stride = recs.strides[0] // ro.capi.SCAN_DTYPE.itemsize if rows else 1
    rc = ro.library().ro_events_host(C.c_void_p(recs.ctypes.data), stride, first_row, rows, C.byref(det),
                                     C.c_void_p(state.ctypes.data), C.c_void_p(events.ctypes.data), cap,
                                     C.c_void_p(summary.ctypes.data), C.c_void_p(detect.ctypes.data))
    assert rc == 0, ro.library().ro_last_error()
    total = int(summary["events"][0])
    written = min(total, cap)
    ev = events.view(ro.capi.EVENT_DTYPE)
    assert np.all(events[written * ro.capi.EVENT_DTYPE.itemsize:] == GUARD), "entries behind the events were touched"
    assert np.all(detect[rows:] == GUARD)
    return ev[:written].copy(), state, summary[0].copy(), detect[:rows].copy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
