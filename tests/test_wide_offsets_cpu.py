"""CPU-side checks of the wide-offset cases (tests/wide_offsets.py; tests/test_gpu_wide_offsets.py runs them on the device).

The layout: every extent of every case lies in front of the arena's end, and each of the four addresses a 32-bit slip would
compute for any element of it lies inside the arena -- so a slip on the device is a wrong value, never a memory fault.
The coverage: every listed entry point is crossed at 2^32 and at 2^33 bytes, every sample-reading one in every format it
accepts, and the int16 cases pass sample index 2^31.  Every sample-side case is a legal call of the ABI.

The long streams: ro_snapshots_host, ro_raw_host and ro_events_host and the numpy emulators of the first two give the same
answer K stream rows later (K = 2^33 + k for the snapshots, a multiple of the ring's rows; 2^36 for the raw capture, whose
first_sample rises by K x hop, 2^44 at a hop of 256), but for first_row, first_sample and the event rows, which rise with the
stream.  Nothing here has a tolerance."""
import numpy as np
import pytest

import rawlib
import snapshotslib
import wide_offsets as W
from eventslib import host_call as events_host_call, random_decisions, records_for, same_bytes


# ---- the layout ---------------------------------------------------------------------------------------------------------
def test_the_four_wrong_addresses_of_a_known_offset():
    o = (1 << 33) + 32                                     # the third strided row: float index 2^31 + 8
    assert W.wrong_addresses(o, 4) == (W.BASE + 32, W.BASE + 32, W.BASE + o, W.BASE + o - (1 << 34))
    o = (1 << 32) + 16                                     # the second: byte offset 2^32 + 16, float index 2^30 + 4
    assert W.wrong_addresses(o, 4) == (W.BASE + 16, W.BASE + 16, W.BASE + o, W.BASE + o)
    o = (1 << 31) + 8                                      # a byte offset whose bit 31 is set goes negative when sign-extended
    assert W.wrong_addresses(o, 8)[1] == W.BASE + o - (1 << 32)
    assert W.BASE + W.ROOM == W.ARENA_BYTES
    assert [e.lo for e in W.strided_extents(W.strided("run_resident: stft32k_kernel"))] == [0, (1 << 32) + 16, (1 << 33) + 32]
    assert [e.lo for e in W.strided_extents(W.strided("spectra_resident: spectra 256"))] == [0, (1 << 32) + 32, (1 << 33) + 64]


@pytest.mark.parametrize("kind", ["samples", "strided", "dense"])
def test_every_wrong_address_lands_inside_the_arena(kind):
    cases = {"samples": W.SAMPLE_CASES, "strided": W.STRIDED_CASES, "dense": W.DENSE_CASES}[kind]
    assert len(cases) >= 3
    probes = 0
    for c in cases:
        exts = W.extents(c)
        assert exts
        for e in exts:
            assert 0 <= e.lo < e.hi <= W.ROOM, (c, e)     # the true addresses: from BASE to the arena's end
            for offset, elem, four in W.landings(e):
                assert e.lo <= offset < e.hi
                assert all(W.inside_arena(a) for a in four), (c, e, offset, elem, four)
                probes += 1
    assert probes >= 2 * len(cases)


def test_extents_of_a_case_do_not_overlap():
    for c in W.all_cases():
        exts = sorted(W.extents(c), key=lambda e: e.lo)
        assert all(a.hi <= b.lo for a, b in zip(exts, exts[1:])), c


# ---- the coverage -------------------------------------------------------------------------------------------------------
def test_every_listed_entry_point_is_crossed_at_both_thresholds():
    by_samples = {(x.entry, x.threshold) for c in W.SAMPLE_CASES for x in W.crossings(c)}
    by_output = {(x.entry, x.threshold) for c in W.STRIDED_CASES + W.DENSE_CASES for x in W.crossings(c)}
    for t in W.THRESHOLDS:
        for entry in W.SAMPLE_ENTRIES:
            assert (entry, t) in by_samples, (entry, t)
        for entry in W.OUTPUT_ENTRIES:
            assert (entry, t) in by_output, (entry, t)
    # every strided case has a row beyond each threshold; every dense case passes 2^32 bytes with its rows
    for c in W.STRIDED_CASES:
        assert [x.threshold for x in W.crossings(c) if x.entry == c.entry] == list(W.THRESHOLDS), c
    for c in W.DENSE_CASES:
        assert W.dense_extents(c)[0].lo < (1 << 32) < W.dense_extents(c)[0].hi, c
        rows = W.dense_probe_rows(c)
        assert rows[1] * c.row_floats * 4 < (1 << 32) <= rows[2] * c.row_floats * 4 and rows[3] == c.rows - 1
    assert any(c.tile and W.dense_extents(c)[1].lo < (1 << 33) < W.dense_extents(c)[1].hi for c in W.DENSE_CASES)


def test_every_sample_reading_entry_point_is_crossed_in_every_format_it_accepts():
    seen = {(x.entry, x.fmt, x.threshold) for c in W.SAMPLE_CASES for x in W.crossings(c)}
    for entry, formats in W.ACCEPTS.items():
        for fmt in formats:
            for t in W.THRESHOLDS:
                assert (entry, fmt, t) in seen, (entry, fmt, t)
    # ... and every kernel in every format its handle takes
    for k in W.KERNELS:
        for fmt in k.formats:
            assert {c.threshold for c in W.SAMPLE_CASES if c.kernel is k and c.fmt == fmt} == set(W.THRESHOLDS), (k.name, fmt)
    # the kernels the issue names, by (path, bins, precision)
    named = {(k.path, k.bins, k.precision) for k in W.KERNELS}
    assert named >= {("rows", 256, W.F32), ("rows", 32768, W.F32), ("rows", 65536, W.F32), ("rows", 262144, W.F32),
                     ("rows", 258, W.F32), ("rows", 256, W.F64), ("rows", 4096, W.F64), ("rows", 65536, W.F64),
                     ("rows", 131072, W.F64), ("spectra", 256, W.F32), ("spectra", 65536, W.F32), ("band", 16384, W.F32),
                     ("windows", 16384, W.F32), ("band", 131072, W.F64), ("windows", 131072, W.F64)}
    # ... and the spectra of FP64 handles, one per branch of the register kernel's spectrum store (rows batched, D = 1, D > 1)
    assert named >= {("spectra", 256, W.F64), ("spectra", 4096, W.F64), ("spectra", 65536, W.F64)}
    assert all(W.IQ_F64 in k.formats for k in W.KERNELS if k.precision == W.F64 and (k.bins <= 65536 or k.path != "rows"))


def test_the_int16_cases_pass_sample_index_2_31():
    hits = [c for c in W.SAMPLE_CASES if c.fmt == W.IQ_I16 and c.threshold == 1 << 33]
    assert {c.kernel.name for c in hits} == {k.name for k in W.KERNELS}
    for c in hits:
        assert W.first_sample(c) < (1 << 31) < W.first_sample(c) + c.kernel.bins <= W.samples(c)
        assert any(x.quantity == "sample" and x.index == 1 << 31 for x in W.crossings(c))
    # float32 samples at 2^33 bytes: sample 2^30, number 2^31
    c = next(c for c in W.SAMPLE_CASES if c.fmt == W.IQ_F32 and c.threshold == 1 << 33)
    assert sorted((x.quantity, x.index) for x in W.crossings(c)) == [("number", 1 << 31), ("sample", 1 << 30)]


def test_every_sample_side_case_is_a_legal_call(ro):
    for c in W.SAMPLE_CASES:
        k = c.kernel
        assert ro.row_count(W.samples(c), k.bins, W.overlap(k)) == W.first_row(c) + W.ROWS, W.sample_id(c)
        assert W.first_row(c) + W.ROWS <= 0x0fffffff and 0 < W.overlap(k) < k.bins
        assert W.tail_samples(c) == k.bins + (W.ROWS - 1) * W.hop(k)
        assert ro.bins_supported(k.bins), k
        if k.windows:
            assert ro.band_windows_supported(k.bins, k.windows, k.precision), k
        bands, tile = W.bands_of(k.bins)
        assert bands[0] + bands[1] <= bands[2] - 2 and bands[2] + bands[3] + 2 <= k.bins and tile[0] + tile[1] <= k.bins
    assert len({W.sample_id(c) for c in W.SAMPLE_CASES}) == len(W.SAMPLE_CASES)


# ---- long streams: the snapshots ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snap_emu():
    return snapshotslib.load_emu()


def test_snapshot_shift_is_a_multiple_of_the_ring_beyond_2_33():
    for ring_rows in (1, 16, 48, 64, 255):
        k = W.snapshot_shift(ring_rows)
        assert k % ring_rows == 0 and (1 << 33) <= k < (1 << 33) + ring_rows


@pytest.mark.parametrize("case_fn", snapshotslib.TABLE, ids=lambda f: f.__name__)
def test_snapshots_decision_table_translated(ro, snap_emu, case_fn):
    """ro_snapshots_host and the emulator, each on the case and on the case K = 2^33 rows later (16 ring rows)"""
    counter = [0, 0]
    case_fn(ro, W.translating_snapshots(snapshotslib.host_vs_emu(ro, snap_emu), counter))
    # max(start_row, 0) does not move with the stream: the three table entries with a candidate in front of row 0 stay where
    # they are (the arena's prefix rule is translated by the random cases and by the ring of 255 rows below)
    if case_fn in (snapshotslib.case_negative_start, snapshotslib.case_arena_exact, snapshotslib.case_arena_short):
        assert counter[1] >= 1, counter                    # (case_arena_short's second call has none and is translated)
    else:
        assert counter[0] >= 1 and counter[1] == 0, counter


def test_snapshots_random_cases_translated(ro, snap_emu):
    rng = np.random.default_rng(2033)
    counter = [0, 0]
    call = W.translating_snapshots(snapshotslib.host_vs_emu(ro, snap_emu), counter)
    captured = pending = 0
    while counter[0] < 20:
        r = call(snapshotslib.case_from_emu(ro, snap_emu.random_case(rng)))
        captured, pending = captured + int(r.summary["captured"]), pending + int(r.summary["pending"])
        assert sum(counter) < 400
    assert captured > 0 and pending > 0


def test_snapshots_ring_of_255_rows_translated(ro, snap_emu):
    counter = [0, 0]
    call = W.translating_snapshots(snapshotslib.host_vs_emu(ro, snap_emu), counter)
    first, then = W.ring_255_cases(ro)
    assert W.snapshot_shift(255) % 255 == 0 and W.snapshot_shift(255) % 256 != 0
    r = call(first)
    assert snapshotslib.statuses(r) == [0, 0, 2, 0, 0] and r.pending_count.tolist() == [1, 0, 0, 0]
    snapshotslib.captured_ok(r, 0, 500, 20, cols=7)          # slots 245 ... 254, 0 ... 9
    snapshotslib.captured_ok(r, 1, 345, 7, cols=7)
    r2 = call(then(r))
    assert snapshotslib.statuses(r2) == [0, 0] and r2.dir["first_row"].tolist() == [590, 640]
    # one float short of the last capturable candidate: it waits, here and K rows later
    short, _ = W.ring_255_cases(ro)
    short.arena_floats = 7 * (20 + 7 + 9 + 2) - 1
    r3 = call(short)
    assert snapshotslib.statuses(r3) == [0, 0, 2, 0] and r3.pending_count.tolist() == [1, 0, 0, 1]
    assert counter == [3, 0]


# ---- long streams: the raw capture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", rawlib.TABLE, ids=lambda f: f.__name__)
def test_raw_decision_table_translated(ro, case_fn):
    """ro_raw_host and the emulator, each on the case and on the case K = 2^36 rows later: first_sample + K x hop"""
    counter = [0, 0]
    case_fn(ro, W.translating_raw(rawlib.host_vs_emu(ro), counter))
    # first_sample is 0 for every start_row below 1: the one table entry that is about it stays where it is
    assert counter[0] >= 1 or case_fn is rawlib.case_first_sample, counter


def test_raw_random_cases_translated(ro):
    rng = np.random.default_rng(2036)
    counter = [0, 0]
    call = W.translating_raw(rawlib.host_vs_emu(ro), counter)
    captured, hops = 0, set()
    while counter[0] < 16:
        case = rawlib.case_from_emu(ro, rawlib.EMU.random_case(rng))
        before = counter[0]
        captured += int(call(case).summary["captured"])
        if counter[0] > before:
            hops.add(W.raw_hop(case))
        assert sum(counter) < 400
    assert captured > 0 and len(hops) >= 2


@pytest.mark.parametrize("shape", W.ODD_HOP_SHAPES, ids=["hop 255", "overlap 0", "hop 3"])
def test_raw_odd_hop_and_no_overlap_translated(ro, shape):
    """an odd hop (f alternates even and odd) and overlap 0 (z = 1), two formats, a run across two spans; at a hop of 256
    the spans begin beyond sample 2^44"""
    counter = [0, 0]
    W.odd_hop_case(ro, shape, W.translating_raw(rawlib.host_vs_emu(ro), counter))
    assert counter == [1, 0]


# ---- long streams: the detector --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_events_across_a_call_boundary_translated(ro, seed):
    """ro_events_host over three calls with carried state, at first_row 0 and at 2^33 + 5: the same events and the same
    state after every call, the rows raised"""
    rng = np.random.default_rng(4000 + seed)
    rows = 3000
    decisions = random_decisions(rng, rows)
    recs = records_for(ro, decisions, seed=seed)
    detector = ((12, 4), (5, 30), (1, 2))[seed]
    detect_rows = np.flatnonzero(decisions)
    # one cut right behind a detect row, so that an open group is carried; one anywhere
    cuts = sorted({int(detect_rows[detect_rows.size // 3]) + 1, int(rng.integers(1, rows))})
    k = W.EVENTS_SHIFT
    states = [np.zeros(1, ro.capi.DETECT_STATE_DTYPE), np.zeros(1, ro.capi.DETECT_STATE_DTYPE)]
    fired = carried = 0
    for lo, hi in zip([0] + cuts, cuts + [rows]):
        ev0, states[0], sm0, det0 = events_host_call(ro, recs[lo:hi], detector, first_row=lo, state=states[0])
        ev1, states[1], sm1, det1 = events_host_call(ro, recs[lo:hi], detector, first_row=k + lo, state=states[1])
        back = ev1.copy()
        for f in ("fire_row", "start_row"):
            back[f] -= k
        assert same_bytes(back, ev0) and sm0.tobytes() == sm1.tobytes() and np.array_equal(det0, det1)
        st = states[1].copy()
        if st["open"][0]:
            st["first_detect_row"] -= k
            st["last_detect_row"] -= k
            carried += 1
        assert same_bytes(st, states[0]), (states[0], states[1])
        fired += ev0.size
    assert fired >= 3 and carried > 0
