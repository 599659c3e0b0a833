"""GPU checks of the detector on the device (csrc/ro_events.hip): events from scan records for up to 8 slots at once, against
ro_events_host per slot and, up to 20 000 rows, against oracle.BolidFsm with mark = row + 1 (BolidRecorder::update's state
machine, src/BolidRecorder.cpp:135, :171-267).  The records are uploaded directly, so no transform is needed -- except in
the last test, which goes from samples to events.  Events, states, summaries and decisions are compared as bytes; every
output has guard entries behind it.  Nothing here has a tolerance."""
import numpy as np
import pytest

from eventslib import (GUARD, bursts, header_constant, host_call, oracle_events, random_decisions, records_for, same_bytes)
from util import add_chirp, noise_iq

pytestmark = pytest.mark.gpu

T = header_constant("RO_EVENTS_TILE_ROWS")
CHUNK = header_constant("RO_EVENTS_CHUNK_ROWS")
NGUARD = 3                                                   # guard entries behind every output
DETECTORS = [(11, 29), (0, 0), (3, 1), (0, 2), (5, 3), (2, 7), (1, 64), (4, 2 * T + 7)]


def bands_for(ro, i):
    return ro.Bands(low_noise=4 + 20 * i, noise_width=16, low_detect=170 + 8 * i, detect_width=8, avg_bins=3)


def handle(ro, extras):
    return ro.Stft(bins=256, overlap=0, bands=bands_for(ro, 0), extra_bands=[bands_for(ro, 1 + i) for i in range(extras)])


def upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(torch, entries, itemsize):
    return torch.full(((entries + NGUARD) * itemsize,), GUARD, dtype=torch.uint8, device="cuda")


def fresh_state(ro, torch, slots):
    d = guarded(torch, slots, 32)
    d[:slots * 32] = 0
    return d


def device_call(ro, torch, st, primary, extra, detectors, d_state, first_row=0, capacity=None, want_detect=True):
    """one ro_stft_events_resident; primary: SCAN_DTYPE[rows] or None, extra: SCAN_DTYPE[rows, count] or None.  Returns
    (events [slot][capacity], written per slot, states, summaries, detect [row][slot]) as numpy, guards checked."""
    slots = 1 + st.extra_count
    rows = primary.shape[0] if primary is not None else extra.shape[0]
    cap = max(rows, 1) if capacity is None else capacity
    d_events = guarded(torch, slots * cap, 40)
    d_summary = guarded(torch, slots, 24)
    d_detect = guarded(torch, rows * slots, 1) if want_detect else None
    d_primary = upload(torch, primary) if primary is not None and rows else None
    d_extra = upload(torch, extra) if extra is not None and rows else None
    if rows == 0:                                            # (a pointer is still needed to say which slots are meant)
        d_primary = torch.zeros(16, dtype=torch.uint8, device="cuda") if primary is not None else None
        d_extra = torch.zeros(16, dtype=torch.uint8, device="cuda") if extra is not None else None
    st.events_resident(rows, detectors, d_state, d_records=d_primary, d_extra=d_extra, first_row=first_row,
                       d_events=d_events if cap else None, capacity=cap, d_summary=d_summary, d_detect=d_detect,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ev, sm, stt = d_events.cpu().numpy(), d_summary.cpu().numpy(), d_state.cpu().numpy()
    assert np.all(ev[slots * cap * 40:] == GUARD) and np.all(sm[slots * 24:] == GUARD) and np.all(stt[slots * 32:] == GUARD)
    detect = None
    if want_detect:
        dt = d_detect.cpu().numpy()
        assert np.all(dt[rows * slots:] == GUARD)
        detect = dt[:rows * slots].reshape(rows, slots)
    return (ev[:slots * cap * 40].reshape(slots, cap * 40), sm[:slots * 24].view(ro.capi.DETECT_SUMMARY_DTYPE),
            stt[:slots * 32].view(ro.capi.DETECT_STATE_DTYPE), detect)


def check_slot(ro, got, slot, recs, det, first_row=0, state=None, capacity=None, oracle=None):
    """slot `slot` of a device call against ro_events_host on the same records (and the oracle where given); returns the
    host's new state"""
    events, summaries, states, detect = got
    cap = events.shape[1] // 40
    want_ev, want_state, want_sum, want_det = host_call(ro, recs, det, first_row=first_row, state=state, capacity=cap)
    n = want_ev.size
    assert same_bytes(summaries[slot], np.array(want_sum)), (slot, summaries[slot], want_sum)
    assert events[slot, :n * 40].tobytes() == want_ev.tobytes(), (slot, events[slot, :n * 40].view(ro.capi.EVENT_DTYPE), want_ev)
    assert np.all(events[slot, n * 40:] == GUARD), "entries past the events written were touched"
    assert same_bytes(states[slot:slot + 1], want_state), (slot, states[slot], want_state)
    if detect is not None:
        assert np.array_equal(detect[:, slot], want_det)
    if oracle is not None:
        assert first_row == 0 and state is None
        ev, still_open = oracle_events(ro, oracle, recs, det[0], det[1])
        assert int(want_sum["events"]) == ev.size and same_bytes(want_ev, ev[:cap]) and bool(want_state["open"][0]) == still_open
    return want_state


@pytest.mark.parametrize("rows", [0, 1, 2, T - 1, T, T + 1, 3 * T + 5])
def test_row_counts_around_a_tile(ro, oracle, torch_cuda, rows):
    torch, rng = torch_cuda, np.random.default_rng(rows)
    det = (3, 3)
    with handle(ro, 0) as st:
        for trial in range(3):
            d = random_decisions(rng, rows, gaps=(1, 2, 2, 3, 4, 5, 40))
            if trial == 1 and rows:
                d[-1] = True                                 # a detect on the very last row: the state stays open
            recs = records_for(ro, d, seed=trial)
            got = device_call(ro, torch, st, recs, None, [det], fresh_state(ro, torch, 1))
            check_slot(ro, got, 0, recs, det, oracle=oracle)
        if rows == 0:                                        # nothing changes but the summary: an open state stays
            keep = np.zeros(1, ro.capi.DETECT_STATE_DTYPE)
            keep[0] = (4, 5, 1.0, 2, 3.0, 1)
            d_state = fresh_state(ro, torch, 1)
            d_state[:32] = upload(torch, keep)
            events, summaries, states, _ = device_call(ro, torch, st, records_for(ro, []), None, [det], d_state, first_row=900)
            assert same_bytes(states, keep) and summaries[0].tolist() == (0, 0, 0) and np.all(events == GUARD)


def seam_cases():
    """name -> (jitter, detect rows); G = max(2, jitter); the tile seam lies between rows T - 1 and T (and 2T - 1, 2T ...)"""
    rows = 5 * T + 9
    out = {}
    out["a group straddles a seam"] = (3, bursts(rows, [(T - 4, 9), (3 * T - 1, 2)]))
    for G in (2, 5, 29):
        for lo in range(G):                                  # the seam at every place inside the gap
            first_end = T - 1 - lo                           # last detect row of the first burst; the gap starts behind it
            out["gap G - 1 = %d merges, %d quiet rows before the seam" % (G - 1, lo)] = \
                (G, bursts(rows, [(first_end - 2, 3), (first_end + 1 + G - 1, 2)]))
            out["gap G = %d splits, %d quiet rows before the seam" % (G, lo)] = \
                (G, bursts(rows, [(first_end - 2, 3), (first_end + 1 + G, 2)]))
    J = 2 * T + 7                                            # whole tiles of silence inside one group
    out["jitter 2T + 7: one group over silent tiles"] = (J, bursts(rows, [(5, 2), (5 + 1 + J - 1, 1), (4 * T, 1)]))
    out["jitter 2T + 7: split by a gap of 2T + 7"] = (J, bursts(rows, [(5, 2), (7 + J, 1)]))
    out["jitter 2T + 7: fires in the last tile"] = (J, bursts(rows, [(2 * T + 1, 2)]))
    for G in (2, 3, 29):
        out["fire row on a tile's first row, G = %d" % G] = (G, bursts(rows, [(2 * T - G - 1, 2), (4 * T - G, 1)]))
        out["fire row on a tile's last row, G = %d" % G] = (G, bursts(rows, [(2 * T - 1 - G - 1, 2), (4 * T - 1 - G, 1)]))
    out["every row a detect"] = (3, np.ones(rows, bool))
    out["alternating rows"] = (2, np.arange(rows) % 2 == 0)
    out["every third row, G = 2: a fire between every two detects"] = (2, np.arange(rows) % 3 == 0)
    return out


SEAMS = seam_cases()


def test_tile_seams(ro, oracle, torch_cuda):
    torch = torch_cuda
    with handle(ro, 0) as st:
        for name, (jitter, d) in SEAMS.items():
            det = (7, jitter)
            recs = records_for(ro, d, seed=len(name))
            got = device_call(ro, torch, st, recs, None, [det], fresh_state(ro, torch, 1))
            try:
                check_slot(ro, got, 0, recs, det, oracle=oracle)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
    # the cases are what their names say
    G = 29
    ev = ro.events_host(records_for(ro, SEAMS["fire row on a tile's first row, G = 29"][1]), (0, G))[0]
    assert ev["fire_row"].tolist() == [2 * T, 4 * T]
    ev = ro.events_host(records_for(ro, SEAMS["fire row on a tile's last row, G = 29"][1]), (0, G))[0]
    assert ev["fire_row"].tolist() == [2 * T - 1, 4 * T - 1]
    ev = ro.events_host(records_for(ro, SEAMS["jitter 2T + 7: one group over silent tiles"][1]), (0, 2 * T + 7))[0]
    assert ev.size == 0
    ev = ro.events_host(records_for(ro, SEAMS["jitter 2T + 7: split by a gap of 2T + 7"][1]), (0, 2 * T + 7))[0]
    assert ev["fire_row"].tolist() == [6 + 2 * T + 7, 7 + 2 * (2 * T + 7)]


def eight_slot_records(ro, rows, seed):
    rng = np.random.default_rng(seed)
    recs = np.zeros((rows, 8), ro.capi.SCAN_DTYPE)
    for s in range(8):
        gaps = (1, 1, 2, 2, 3, 4, 5, 28, 29, 30, 70, 300) if s != 7 else (1, 5, 300, 2 * T + 6, 2 * T + 7, 3 * T)
        recs[:, s] = records_for(ro, random_decisions(rng, rows, gaps=gaps), seed=seed + s)
    recs["average"][::97, 3] = recs["noise"][::97, 3] * np.float32(2.0)          # some marginal rows in one slot
    return recs


def test_eight_slots_eight_detectors(ro, oracle, torch_cuda):
    torch = torch_cuda
    rows = 20000
    recs = eight_slot_records(ro, rows, 11)
    primary, extra = np.ascontiguousarray(recs[:, 0]), np.ascontiguousarray(recs[:, 1:])
    with handle(ro, 7) as st:
        got = device_call(ro, torch, st, primary, extra, DETECTORS, fresh_state(ro, torch, 8))
        for s in range(8):
            check_slot(ro, got, s, recs[:, s], DETECTORS[s], oracle=oracle)
        assert int(got[1]["marginal_rows"][3]) >= rows // 97 and int(got[1]["events"].min()) > 5
        # two launches give the same bytes
        again = device_call(ro, torch, st, primary, extra, DETECTORS, fresh_state(ro, torch, 8))
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
        # capacity smaller than the events: the first `capacity` are written, the total is in the summary
        small = device_call(ro, torch, st, primary, extra, DETECTORS, fresh_state(ro, torch, 8), capacity=5)
        for s in range(8):
            check_slot(ro, small, s, recs[:, s], DETECTORS[s])
            assert small[0][s].tobytes() == got[0][s, :5 * 40].tobytes()
        assert same_bytes(small[1], got[1]) and same_bytes(small[2], got[2])
        none = device_call(ro, torch, st, primary, extra, DETECTORS, fresh_state(ro, torch, 8), capacity=0, want_detect=False)
        assert same_bytes(none[1], got[1]) and same_bytes(none[2], got[2])


def test_a_null_pointer_leaves_its_slots_untouched(ro, torch_cuda):
    torch = torch_cuda
    rows = 2 * T + 3
    recs = eight_slot_records(ro, rows, 5)[:, :3]
    dets = DETECTORS[1:4]
    with handle(ro, 2) as st:
        for primary, extra, live in ((None, np.ascontiguousarray(recs[:, 1:]), (1, 2)), (np.ascontiguousarray(recs[:, 0]), None, (0,))):
            d_state = guarded(torch, 3, 32)                  # guard bytes in the slots that are not asked for, too
            for s in live:
                d_state[s * 32:(s + 1) * 32] = 0
            events, summaries, states, detect = got = device_call(ro, torch, st, primary, extra, dets, d_state)
            for s in range(3):
                if s in live:
                    check_slot(ro, got, s, recs[:, s], dets[s])
                else:
                    assert np.all(events[s] == GUARD) and np.all(summaries[s:s + 1].view(np.uint8) == GUARD)
                    assert np.all(states[s:s + 1].view(np.uint8) == GUARD) and np.all(detect[:, s] == GUARD)


def test_one_call_equals_three_uneven_calls(ro, torch_cuda):
    torch = torch_cuda
    rows = 7 * T + 11
    recs = eight_slot_records(ro, rows, 23)
    base = 2 ** 33 + 5                                       # stream rows far beyond int32
    with handle(ro, 7) as st:
        one = device_call(ro, torch, st, np.ascontiguousarray(recs[:, 0]), np.ascontiguousarray(recs[:, 1:]), DETECTORS,
                          fresh_state(ro, torch, 8), first_row=base)
        for s in range(8):
            check_slot(ro, one, s, recs[:, s], DETECTORS[s], first_row=base)
        d_state = fresh_state(ro, torch, 8)
        host_state = [None] * 8
        parts, totals = [[] for _ in range(8)], np.zeros((8, 3), np.int64)
        for lo, hi in ((0, T + 1), (T + 1, T + 2), (T + 2, rows)):
            part = recs[lo:hi]
            got = device_call(ro, torch, st, np.ascontiguousarray(part[:, 0]), np.ascontiguousarray(part[:, 1:]), DETECTORS,
                              d_state, first_row=base + lo)
            for s in range(8):
                host_state[s] = check_slot(ro, got, s, part[:, s], DETECTORS[s], first_row=base + lo, state=host_state[s])
                n = int(got[1]["events"][s])
                parts[s].append(got[0][s, :n * 40])
                totals[s] += np.array(got[1][s].tolist())
        for s in range(8):
            n = int(one[1]["events"][s])
            assert np.concatenate(parts[s]).tobytes() == one[0][s, :n * 40].tobytes()
            assert totals[s].tolist() == list(one[1][s].tolist())
        assert same_bytes(got[2], one[2])                    # the states behind the last call


@pytest.mark.parametrize("what", ["a group across the chunk seam", "a pending fire across the chunk seam"])
def test_more_rows_than_a_chunk(ro, torch_cuda, what):
    torch = torch_cuda
    rows = CHUNK + T + 3
    d = random_decisions(np.random.default_rng(3), rows, gaps=(5, 40, 300, 2000))
    d[CHUNK - 40:] = False
    d[CHUNK + 100:CHUNK + 103] = True                        # a group of the second chunk's own: fires at CHUNK + 131
    if what.startswith("a group"):
        d[CHUNK - 3:CHUNK + 2] = True                        # detect rows on both sides; G = 29 rows later it fires
        fire, start = CHUNK + 1 + 29, CHUNK - 3
    else:
        d[CHUNK - 9:CHUNK - 6] = True                        # the last detect row 7 rows before the seam, the fire row behind it
        fire, start = CHUNK - 7 + 29, CHUNK - 9
    recs = records_for(ro, d, seed=1)
    det = (11, 29)
    with handle(ro, 0) as st:
        got = device_call(ro, torch, st, recs, None, [det], fresh_state(ro, torch, 1), capacity=rows // 4)
        check_slot(ro, got, 0, recs, det)
    ev = got[0][0].view(ro.capi.EVENT_DTYPE)[:int(got[1]["events"][0])]
    i = int(np.searchsorted(ev["fire_row"], fire))
    assert ev["fire_row"][i] == fire and ev["start_row"][i] == start + 1 - 11 and ev["peak"][i] == recs["peak"][start]
    assert ev["fire_row"][-1] == CHUNK + 131 and ev["fire_row"][-2] == fire and np.all(np.diff(ev["fire_row"]) > 0)


def test_refusals(ro, torch_cuda):
    torch = torch_cuda
    recs = upload(torch, records_for(ro, bursts(10, [(2, 2)])))
    with handle(ro, 0) as st:
        d_state = fresh_state(ro, torch, 1)
        for kw, code, word in ((dict(d_extra=recs), -5, "extra"), (dict(rows=-1), -1, "rows"), (dict(capacity=-1), -1, "capacity"),
                               (dict(capacity=4), -1, "d_events"), (dict(detectors=[(-1, 2)]), -1, "set 0"),
                               (dict(d_state=None), -1, "d_state"), (dict(d_records=None), -1, "d_records")):
            args = dict(rows=10, detectors=[(1, 2)], d_state=d_state, d_records=recs)
            args.update(kw)
            with pytest.raises(ro.StftError) as e:
                st.events_resident(**args)
            assert e.value.code == code and word in str(e.value), (kw, str(e.value))
    with handle(ro, 2) as st:
        with pytest.raises(ro.StftError) as e:
            st.events_resident(10, [(1, 2), (1, 2), (1, -3)], fresh_state(ro, torch, 3), d_records=recs)
        assert e.value.code == -1 and "set 2" in str(e.value)
    torch.cuda.synchronize()


def test_samples_to_events_at_256_bins(ro, oracle, torch_cuda):
    """run_resident_events with one extra set: the rows and records are run_resident_sets' bits, the events are the
    oracle's machine over those records.  Two tone bursts in each set's detect band, the later one G - 1 rows after a
    third: the machine joins those two."""
    torch = torch_cuda
    bins, nrows, G = 256, 72, 4
    iq = noise_iq(np.random.default_rng(8), nrows * bins, sigma=0.05)
    hop_s = bins / 48000.0
    for first, n in ((10, 3), (40, 2), (42 + G - 1, 2)):                        # 6000 Hz: column 128 + 32
        add_chirp(iq, first * bins, n * hop_s, 6000.0, 0.0, 5.0)
    for first, n in ((5, 1), (20, 4), (24 + G - 1, 1)):                         # -9000 Hz: column 128 - 48
        add_chirp(iq, first * bins, n * hop_s, -9000.0, 0.0, 5.0)
    primary = ro.Bands(low_noise=20, noise_width=40, low_detect=150, detect_width=20, avg_bins=9)
    second = ro.Bands(low_noise=180, noise_width=40, low_detect=70, detect_width=20, avg_bins=9)
    dets = [(2, G), (1, G)]
    d_iq = torch.from_numpy(iq).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def buffers():
        return (torch.zeros((nrows, bins), dtype=torch.float32, device="cuda"), guarded(torch, nrows, 12),
                guarded(torch, nrows, 12))
    with ro.Stft(bins=bins, overlap=0, bands=primary, extra_bands=[second]) as st:
        want_rows, want_recs, want_extra = buffers()
        st.run_resident_sets(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, want_rows, d_records=want_recs, d_extra=want_extra, stream=s)
        got_rows, got_recs, got_extra = buffers()
        d_state, d_events, d_summary = fresh_state(ro, torch, 2), guarded(torch, 2 * 8, 40), guarded(torch, 2, 24)
        d_detect = guarded(torch, 2 * nrows, 1)
        st.run_resident_events(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, got_rows, dets, d_state, d_records=got_recs,
                               d_extra=got_extra, d_events=d_events, capacity=8, d_summary=d_summary, d_detect=d_detect, stream=s)
        torch.cuda.synchronize()
    assert torch.equal(got_rows.view(torch.int32), want_rows.view(torch.int32))
    assert torch.equal(got_recs, want_recs) and torch.equal(got_extra, want_extra)
    sets = [got_recs.cpu().numpy()[:nrows * 12].view(ro.capi.SCAN_DTYPE), got_extra.cpu().numpy()[:nrows * 12].view(ro.capi.SCAN_DTYPE)]
    events = d_events.cpu().numpy()
    summary = d_summary.cpu().numpy()
    assert np.all(events[16 * 40:] == GUARD) and np.all(summary[48:] == GUARD) and np.all(d_state.cpu().numpy()[64:] == GUARD)
    detect = d_detect.cpu().numpy()[:2 * nrows].reshape(nrows, 2)
    for slot, (recs, det) in enumerate(zip(sets, dets)):
        want, still_open = oracle_events(ro, oracle, recs, det[0], det[1])
        n = int(summary[:48].view(ro.capi.DETECT_SUMMARY_DTYPE)["events"][slot])
        print("slot %d: detect rows %s, events %s" % (slot, np.flatnonzero(detect[:, slot]).tolist(), want["fire_row"].tolist()))
        assert n == want.size and events[slot * 320:slot * 320 + n * 40].tobytes() == want.tobytes()
        assert bool(d_state.cpu().numpy()[:64].view(ro.capi.DETECT_STATE_DTYPE)["open"][slot]) == still_open
        assert want.size >= 2 and int(want["length"].max()) >= 2 * det[0] + G + 2      # the joined bursts, quiet rows included
