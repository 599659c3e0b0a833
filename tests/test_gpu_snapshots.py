"""GPU checks of the event snapshots on the device (csrc/ro_snapshots.hip): rows into a ring in HBM, and the rows of every
complete event's snapshot out of it into an arena with a directory -- against ro_snapshots_host byte for byte (summary,
directory, arena, pending lists and counts), with guard entries behind every output and the ring's padding floats checked.
The inputs are synthetic: slot r % ring_rows of the ring holds r * 1000 + column, so a wrong row or column names itself.
Only the last test runs a transform.  Nothing here has a tolerance."""
import numpy as np
import pytest

from eventslib import same_bytes
from snapshotslib import (CAPTURED, EMPTY, GUARD, LOST, PAD, TABLE, Case, Result, case_from_emu, events_of, header_constant,
                          host_call, image_of, load_emu, outputs_for, ring_desc, row_values)
from util import add_chirp, noise_iq

pytestmark = pytest.mark.gpu

TILE = header_constant("RO_SNAP_TILE")


def handle(ro):
    return ro.Stft(bins=256, overlap=0)


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def launch(ro, torch, st, case, d_ring, d_outs, d_events, d_summary):
    """one ro_stft_snapshots_resident on the current stream; nothing is waited for"""
    st.snapshots_resident(case.mask, case.snapshot_rows.tolist(), ring_desc(ro, case, d_ring.data_ptr()), case.head_row,
                          d_outs[2] if case.pcap else None, d_outs[3], case.pcap, d_outs[0],
                          d_outs[1] if case.arena_floats else None, case.arena_floats, d_outs[4],
                          d_events=d_events if case.capacity else None, capacity=case.capacity, d_summary=d_summary,
                          stream=stream_of(torch))


def device_call(ro, torch, st, case):
    d_ring = up(torch, case.ring)
    d_outs = [up(torch, o) for o in outputs_for(case)]
    d_events = up(torch, case.events) if case.capacity else None
    d_summary = up(torch, case.summary) if case.summary is not None else None
    launch(ro, torch, st, case, d_ring, d_outs, d_events, d_summary)
    torch.cuda.synchronize()
    assert d_ring.cpu().numpy().tobytes() == case.ring.tobytes(), "the ring was written"
    return Result(ro, case, *[o.cpu().numpy() for o in d_outs])


def device_vs_host(ro, torch, st, twice=False):
    def call(case):
        got, want = device_call(ro, torch, st, case), host_call(ro, case)
        assert got.summary.tobytes() == want.summary.tobytes(), (got.summary, want.summary)
        assert got.dir.tobytes() == want.dir.tobytes(), (got.dir, want.dir)
        assert got.same_bytes(want)
        if twice:
            assert device_call(ro, torch, st, case).same_bytes(got), "two runs differ"
        return got
    return call


# ---- 1. rows into the ring ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 256, 257])
def test_ring_put(ro, torch_cuda, cols):
    torch = torch_cuda
    stride = cols + 3
    with handle(ro) as st:
        for ring_rows in (1, 7, 64):
            first = 5 * ring_rows + max(ring_rows - 3, 0)
            to_wrap = ring_rows - first % ring_rows                              # rows up to and including the last slot
            for rows in sorted({0, to_wrap, to_wrap + 1, ring_rows, ring_rows + 1, 2 * ring_rows + 3}):
                for image_stride in (cols, cols + 5):
                    image = np.full((max(rows, 1), image_stride), 77.0, np.float32)
                    for i in range(rows):
                        image[i, :cols] = row_values(first + i, cols)
                    want = np.full((ring_rows, stride), PAD, np.float32)
                    want[:, :cols] = -1.0
                    start = want.copy()
                    for i in range(max(0, rows - ring_rows), rows):
                        want[(first + i) % ring_rows, :cols] = image[i, :cols]
                    runs = []
                    for _ in range(2):
                        d_ring = torch.full(((ring_rows * stride + 16) * 4,), GUARD, dtype=torch.uint8, device="cuda")
                        d_ring[:ring_rows * stride * 4] = up(torch, start)
                        d_image = up(torch, image)
                        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
                        st.ring_put_resident(d_image, first, rows, ring, image_stride=image_stride, stream=stream_of(torch))
                        torch.cuda.synchronize()
                        runs.append(d_ring.cpu().numpy())
                    got = runs[0][:ring_rows * stride * 4].view(np.float32).reshape(ring_rows, stride)
                    where = (cols, ring_rows, rows, image_stride)
                    assert np.array_equal(got[:, :cols], want[:, :cols]), where
                    assert np.all(got[:, cols:] == PAD), "padding floats of a slot were touched: %s" % (where,)
                    assert np.all(runs[0][ring_rows * stride * 4:] == GUARD), where
                    assert runs[0].tobytes() == runs[1].tobytes(), where
        # refusals, before anything is launched
        d = torch.zeros(64, dtype=torch.float32, device="cuda")
        good = ro.capi.RowRing(d.data_ptr(), 8, 4, 5, 0)
        for kw, word in ((dict(first_row=-1), "first_row"), (dict(rows=-1), "rows"), (dict(image_stride=4), "image_stride"),
                         (dict(d_image=None), "d_image"), (dict(ring=ro.capi.RowRing(d.data_ptr(), 4, 4, 5, 0)), "stride"),
                         (dict(ring=ro.capi.RowRing(d.data_ptr(), 8, 0, 5, 0)), "ring_rows"),
                         (dict(ring=ro.capi.RowRing(None, 8, 4, 5, 0)), "d_rows")):
            args = dict(d_image=d, first_row=0, rows=2, ring=good, image_stride=8)
            args.update(kw)
            with pytest.raises(ro.StftError) as e:
                st.ring_put_resident(**args)
            assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
        torch.cuda.synchronize()


# ---- 2. the snapshots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_on_the_device(ro, torch_cuda, case_fn):
    with handle(ro) as st:
        case_fn(ro, device_vs_host(ro, torch_cuda, st))


def spans_around(rng, n, head, ring_rows):
    start = head - rng.integers(-6, ring_rows + 12, n)
    return list(zip(start.tolist(), rng.integers(-1, 14, n).tolist()))


@pytest.mark.parametrize("arena_images", [10000, 120])
def test_300_events_in_one_slot_cross_the_plan_kernels_tile(ro, torch_cuda, arena_images):
    """300 events and 30 pending candidates in slot 0, 5 events in slot 3, cols = 3: snap_plan_kernel walks two tiles of
    slot 0 and carries the directory index, the packed rows and the pending index into the second and on into slot 3;
    with the small arena the room runs out inside a tile"""
    torch, rng = torch_cuda, np.random.default_rng(300)
    head, ring_rows, cols = 1000, 64, 3
    case = Case(ro, {0: spans_around(rng, 300, head, ring_rows), 3: spans_around(rng, 5, head, ring_rows)}, 9, ring_rows, cols,
                head, arena_images * cols * 4, pending={0: spans_around(rng, 30, head, ring_rows)}, pcap=80)
    assert case.mask == 0b1001 and case.capacity == 300
    with handle(ro) as st:
        r = device_vs_host(ro, torch, st, twice=True)(case)
    s = r.summary
    print(s)
    assert int(s["resolved"]) > TILE or arena_images == 120
    assert min(int(s[k]) for k in ("captured", "empty", "lost", "pending")) > 0
    assert (int(s["pending_dropped"]) > 0) == (arena_images == 120)
    # candidates of the second tile were captured, behind the packed rows of the first: their images are their rows
    late = [i for i in range(r.dir.size) if r.dir[i]["status"] == CAPTURED and
            r.dir[i]["event"]["peak"] in set(case.events[0, TILE:]["peak"].tolist())]
    assert late or arena_images == 120
    for i in list(range(0, r.dir.size, 17)) + late[-3:]:
        if r.dir[i]["status"] == CAPTURED:
            assert np.array_equal(r.image(i, cols), image_of(int(r.dir[i]["first_row"]), int(r.dir[i]["rows"]), cols)), i
    # (slot 3's candidates have rows: behind a full arena they can only wait)
    assert r.dir["slot"].tolist() == sorted(r.dir["slot"].tolist())
    assert set(r.dir["slot"].tolist()) == ({0, 3} if arena_images == 10000 else {0})


def test_eight_slots_holes_in_the_mask_and_no_events(ro, torch_cuda):
    torch, rng = torch_cuda, np.random.default_rng(8)
    head, ring_rows, cols = 500, 48, 70
    with handle(ro) as st:
        call = device_vs_host(ro, torch, st, twice=True)
        # all 8 slots at once, each with its own snapshot_rows
        every = {s: spans_around(rng, 20 + s, head, ring_rows) for s in range(8)}
        pend = {s: spans_around(rng, s, head, ring_rows) for s in range(1, 8)}
        r = call(Case(ro, every, list(range(3, 11)), ring_rows, cols, head, cols * 900, pending=pend, pcap=8))
        assert set(r.dir["slot"].tolist()) == set(range(8)) and int(r.summary["captured"]) > 20
        # a mask with holes: the slots outside it keep their pending lists and counts, whatever is in them
        case = Case(ro, {s: every[s] for s in (0, 2, 5, 7)}, 7, ring_rows, cols, head, cols * 300, pending={2: pend[2], 7: pend[7]},
                    pcap=8)
        assert case.mask == 0b10100101
        case.pending[1] = events_of(ro, spans_around(rng, 8, head, ring_rows))
        case.pending_count[[1, 3, 4, 6]] = [5, -3, 99, 8]
        r = call(case)
        assert set(r.dir["slot"].tolist()) <= {0, 2, 5, 7} and r.pending_count[[1, 3, 4, 6]].tolist() == [5, -3, 99, 8]
        assert r.pending[1].tobytes() == case.pending[1].tobytes()
        # capacity = 0 with a non-empty pending list: a call that only flushes
        flush = Case(ro, {}, 7, ring_rows, cols, head + 10, cols * 300, pcap=8, capacity=0, mask=case.mask,
                     with_summary=False).carry(r)
        assert flush.pending_count[[0, 2, 5, 7]].sum() > 0
        r2 = call(flush)
        assert int(r2.summary["resolved"]) > 0 and int(r2.summary["unlisted"]) == 0
    # the emulator's random shapes, a few of them, on the device
    emu = load_emu()
    rng = np.random.default_rng(77)
    with handle(ro) as st:
        call = device_vs_host(ro, torch, st)
        for _ in range(12):
            call(case_from_emu(ro, emu.random_case(rng)))


def test_refusals_with_a_handle(ro, torch_cuda):
    torch = torch_cuda
    case = Case(ro, {0: [(30, 4)]}, 5, 16, 5, 40, 100)
    d_ring, d_outs = up(torch, case.ring), [up(torch, o) for o in outputs_for(case)]
    d_events, d_summary = up(torch, case.events), up(torch, case.summary)
    ring = ring_desc(ro, case, d_ring.data_ptr())
    with handle(ro) as st:
        for kw, word in ((dict(d_events=None), "d_events"), (dict(d_summary=None), "d_summary"), (dict(d_arena=None), "d_arena"),
                         (dict(d_pending=None), "d_pending"), (dict(d_pending_count=None), "d_pending_count"),
                         (dict(d_dir=None), "d_dir"), (dict(d_snap_summary=None), "d_snap_summary"), (dict(head_row=-1), "head_row"),
                         (dict(slot_mask=0), "slot_mask"), (dict(slot_mask=256), "slot_mask"), (dict(snapshot_rows=[0]), "snapshot_rows[0]"),
                         (dict(capacity=-1), "capacity"), (dict(pending_capacity=-2), "pending_capacity"),
                         (dict(arena_floats=-1), "arena_floats"), (dict(capacity=1 << 25), "candidates"),
                         (dict(ring=ro.capi.RowRing(d_ring.data_ptr(), 4, 16, 5, 0)), "stride")):
            args = dict(slot_mask=1, snapshot_rows=5, ring=ring, head_row=40, d_pending=d_outs[2], d_pending_count=d_outs[3],
                        pending_capacity=case.pcap, d_dir=d_outs[0], d_arena=d_outs[1], arena_floats=100,
                        d_snap_summary=d_outs[4], d_events=d_events, capacity=1, d_summary=d_summary)
            args.update(kw)
            with pytest.raises(ro.StftError) as e:
                st.snapshots_resident(**args)
            assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    for o, before in zip(d_outs, outputs_for(case)):
        assert o.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"


# ---- 3. chained calls on one stream, nothing waited for in between -----------------------------------------------------------
def test_four_chunks_back_to_back_without_a_host_synchronisation(ro, torch_cuda):
    torch = torch_cuda
    chunk, chunks, ring_rows, cols, snap, pcap, cap = 50, 4, 96, 33, 20, 6, 12
    total = chunk * chunks
    stride = cols + 3
    rng = np.random.default_rng(4)
    # events of chunk k "fire" inside it; their snapshots begin up to 15 rows earlier and end up to 25 rows later, all by `total`
    per_chunk = []
    for k in range(chunks):
        slots = {}
        for s in (0, 2):
            fire = np.sort(rng.integers(k * chunk, (k + 1) * chunk, 7))
            spans = [(int(f) - int(rng.integers(0, 16)), int(rng.integers(1, 26))) for f in fire]
            slots[s] = [(a, min(n, total - a)) for a, n in spans]
        per_chunk.append(slots)
    image = np.stack([row_values(r, cols) for r in range(total)])
    cases, host = [], []
    for k in range(chunks):
        case = Case(ro, per_chunk[k], snap, ring_rows, cols, (k + 1) * chunk, cols * 400, pcap=pcap, capacity=cap, stride=stride)
        if host:
            case.carry(host[-1])
        cases.append(case)
        host.append(host_call(ro, case))
    # (what the case is meant to hold, said of the host twin's results: the device has to equal them below)
    assert sum(int(r.summary["captured"]) for r in host) > 30 and int(host[-1].summary["pending"]) == 0
    assert all(int(r.summary["lost"]) == 0 and int(r.summary["pending_dropped"]) == 0 for r in host)
    assert any(int(r.summary["pending"]) > 0 for r in host[:-1])
    with handle(ro) as st:
        s = stream_of(torch)
        d_image = up(torch, image)
        d_ring = torch.full((ring_rows * stride,), float(PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        outs = [[up(torch, o) for o in outputs_for(cases[0])] for _ in range(chunks)]
        d_events = [up(torch, c.events) for c in cases]
        d_summary = [up(torch, c.summary) for c in cases]
        d_pending, d_count = outs[0][2], outs[0][3]                              # one pair of lists for the whole stream
        torch.cuda.synchronize()
        for k in range(chunks):                                                  # ---- nothing below waits for the device
            st.ring_put_resident(d_image[k * chunk * cols * 4:], k * chunk, chunk, ring, stream=s)
            st.snapshots_resident(cases[k].mask, snap, ring, (k + 1) * chunk, d_pending, d_count, pcap, outs[k][0], outs[k][1],
                                  cases[k].arena_floats, outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k],
                                  stream=s)
        torch.cuda.synchronize()
        # the ring holds the last ring_rows rows, its padding is untouched
        got_ring = d_ring.cpu().numpy().reshape(ring_rows, stride)
        for r in range(total - ring_rows, total):
            assert np.array_equal(got_ring[r % ring_rows, :cols], row_values(r, cols)), r
        assert np.all(got_ring[:, cols:] == PAD)
        results = []
        for k in range(chunks):
            raw = [o.cpu().numpy() for o in outs[k]]
            raw[2], raw[3] = host[k].raw[2], host[k].raw[3]                      # (the lists exist once: checked behind the last call)
            results.append(Result(ro, cases[k], *raw))
            assert results[k].same_bytes(host[k]), k
        assert d_pending.cpu().numpy().tobytes() == host[-1].raw[2].tobytes()
        assert d_count.cpu().numpy().tobytes() == host[-1].raw[3].tobytes()
        # ... and what a single call over everything resolves: a ring that holds all rows, every event at once.  Per slot the
        # order is the events' order in both; the chained calls interleave the slots call by call.
        everything = {s_: np.concatenate([c.events[s_, :int(c.summary["events"][s_])] for c in cases]) for s_ in (0, 2)}
        one = Case(ro, everything, snap, 256, cols, total, cols * 800, pcap=pcap, stride=stride)
        single = device_vs_host(ro, torch, st)(one)
    assert int(single.summary["pending"]) == 0 and int(single.summary["lost"]) == 0
    for s_ in (0, 2):
        chained = [(e, r) for r in results for e in r.dir if e["slot"] == s_]
        alone = [e for e in single.dir if e["slot"] == s_]
        assert len(chained) == len(alone) == 7 * chunks
        key = lambda e: (int(e["event"]["fire_row"]), int(e["event"]["peak"]))
        assert sorted(key(e) for e, _ in chained) == sorted(key(e) for e in alone)
        by_key = {key(e): e for e in alone}
        for e, r in chained:
            o = by_key[key(e)]
            assert (e["event"].tobytes(), int(e["first_row"]), int(e["rows"]), int(e["status"])) == \
                   (o["event"].tobytes(), int(o["first_row"]), int(o["rows"]), int(o["status"]))
            n = int(e["rows"]) * cols
            assert np.array_equal(r.arena[int(e["offset"]):int(e["offset"]) + n],
                                  single.arena[int(o["offset"]):int(o["offset"]) + n])


# ---- 4. from samples to snapshots --------------------------------------------------------------------------------------------
def test_samples_to_snapshots_in_three_chunks(ro, torch_cuda):
    """1024 bins, 75 % overlap, 600 rows, two windows (40 and 25 columns), two detectors, three chunks of 200 rows:
    run_resident_windows -> ring_put_resident -> events_resident -> snapshots_resident per chunk, nothing waited for.  Tone
    bursts sit where the closed form puts one snapshot's start in the chunk before its fire row (detect rows from about 202:
    start = r0 + 1 - 12 < 200, fire row about 211) and one snapshot's end behind its fire row's chunk (last detect row about
    193: fire row 197 < 200 <= hi = last + 14).  Both are asserted from the per-call directories."""
    torch = torch_cuda
    bins, overlap, nrows, chunk = 1024, 768, 600, 200
    hop = bins - overlap
    samples = bins + hop * (nrows - 1)
    iq = noise_iq(np.random.default_rng(31), samples, sigma=0.05)
    for f, spans in ((6000.0, ((189, 191), (203, 206), (450, 452))), (-9000.0, ((100, 101), (393, 395), (520, 524)))):
        for a, b in spans:
            add_chirp(iq, a * hop + 384, ((b - a) * hop + 256) / 48000.0, f, 0.0, 5.0)
    windows = [(300, 40), (628, 25)]                         # -9000 Hz is column 320, 6000 Hz column 640
    cols = 65
    primary = ro.Bands(low_noise=100, noise_width=64, low_detect=630, detect_width=20, avg_bins=5)
    second = ro.Bands(low_noise=700, noise_width=64, low_detect=310, detect_width=20, avg_bins=5)
    dets = [(12, 4), (5, 3)]
    snap, ring_rows, cap, pcap = 40, 256, 24, 8              # the ring: a chunk + snapshot_rows + 2 advance + G, rounded up
    stride = cols + 3
    arena_floats = cols * snap * 12
    s = stream_of(torch)
    d_iq = torch.from_numpy(iq).cuda()
    proto = Case(ro, {0: [], 1: []}, snap, ring_rows, cols, 0, arena_floats, pcap=pcap, capacity=cap, stride=stride)
    with ro.Stft(bins=bins, overlap=overlap, bands=primary, extra_bands=[second]) as st:
        # the yardstick: one un-chunked run
        all_rows = torch.zeros((nrows, bins), dtype=torch.float32, device="cuda")
        all_image = torch.zeros((nrows, cols), dtype=torch.float32, device="cuda")
        all_recs = torch.zeros((nrows * 12,), dtype=torch.uint8, device="cuda")
        all_extra = torch.zeros((nrows * 12,), dtype=torch.uint8, device="cuda")
        st.run_resident_windows(d_iq, ro.RO_IQ_F32, samples, 0, nrows, all_rows, windows, all_image, d_records=all_recs,
                                d_extra=all_extra, stream=s)
        # the chunks
        d_rows = torch.zeros((chunk, bins), dtype=torch.float32, device="cuda")
        d_image = [torch.zeros((chunk, cols), dtype=torch.float32, device="cuda") for _ in range(3)]
        d_recs = torch.zeros((chunk * 12,), dtype=torch.uint8, device="cuda")
        d_extra = torch.zeros((chunk * 12,), dtype=torch.uint8, device="cuda")
        d_ring = torch.full((ring_rows * stride,), float(PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_state = torch.zeros((2 * 32,), dtype=torch.uint8, device="cuda")
        outs = [[up(torch, o) for o in outputs_for(proto)] for _ in range(3)]
        d_events = [torch.full((2 * cap * 40,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_summary = [torch.zeros((2 * 24,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_pending, d_count = outs[0][2], outs[0][3]
        torch.cuda.synchronize()
        for k in range(3):                                   # ---- nothing below waits for the device
            first = k * chunk
            st.run_resident_windows(d_iq, ro.RO_IQ_F32, samples, first, chunk, d_rows, windows, d_image[k], d_records=d_recs,
                                    d_extra=d_extra, stream=s)
            st.ring_put_resident(d_image[k], first, chunk, ring, stream=s)
            st.events_resident(chunk, dets, d_state, d_records=d_recs, d_extra=d_extra, first_row=first, d_events=d_events[k],
                               capacity=cap, d_summary=d_summary[k], stream=s)
            st.snapshots_resident(3, snap, ring, first + chunk, d_pending, d_count, pcap, outs[k][0], outs[k][1], arena_floats,
                                  outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k], stream=s)
        torch.cuda.synchronize()
    image = all_image.cpu().numpy()
    for k in range(3):
        assert torch.equal(d_image[k].view(torch.int32), all_image[k * chunk:(k + 1) * chunk].view(torch.int32)), k
    # the events of the three calls are ro_events_host's over all records
    recs = [all_recs.cpu().numpy().view(ro.capi.SCAN_DTYPE), all_extra.cpu().numpy().view(ro.capi.SCAN_DTYPE)]
    got_events = [[], []]
    for k in range(3):
        sm = d_summary[k].cpu().numpy().view(ro.capi.DETECT_SUMMARY_DTYPE)
        ev = d_events[k].cpu().numpy().view(ro.capi.EVENT_DTYPE).reshape(2, cap)
        for slot in range(2):
            assert int(sm["events"][slot]) <= cap
            got_events[slot].append(ev[slot, :int(sm["events"][slot])])
    want_events = []
    for slot in range(2):
        want, _, _, detect = ro.events_host(recs[slot], dets[slot], want_detect=True)
        print("slot %d: detect rows %s\n  fire rows %s" % (slot, np.flatnonzero(detect).tolist(), want["fire_row"].tolist()))
        assert same_bytes(np.concatenate(got_events[slot]), want)
        want_events.append(want)
    # every event whose snapshot was complete by row 600 is in exactly one directory, captured, with the un-chunked image's rows
    results, seen = [], [[], []]
    for k in range(3):
        raw = [o.cpu().numpy() for o in outs[k]]
        if k:                                                # (the lists exist once, in the first call's buffers)
            raw[2], raw[3] = outputs_for(proto)[2], outputs_for(proto)[3]
            raw[2][:], raw[3][:] = outs[0][2].cpu().numpy(), outs[0][3].cpu().numpy()
        r = Result(ro, proto, *raw)
        results.append(r)
        assert int(r.summary["lost"]) == 0 and int(r.summary["pending_dropped"]) == 0 and int(r.summary["unlisted"]) == 0
        for i, e in enumerate(r.dir):
            assert e["status"] == CAPTURED
            lo, n = int(e["first_row"]), int(e["rows"])
            assert lo == max(int(e["event"]["start_row"]), 0) and n == min(int(e["event"]["length"]), snap) - (lo - int(e["event"]["start_row"]))
            assert lo + n <= (k + 1) * chunk
            assert r.image(i, cols).tobytes() == image[lo:lo + n].tobytes(), (k, i, e)
            seen[int(e["slot"])].append(e["event"])
    for slot in range(2):
        done = want_events[slot][want_events[slot]["start_row"] + np.minimum(want_events[slot]["length"], snap) <= nrows]
        assert same_bytes(np.array(seen[slot], ro.capi.EVENT_DTYPE), done) and done.size >= 3
    # both seams happened: a snapshot that starts in the chunk before its fire row's ...
    starts_before = [(k, e) for k, r in enumerate(results) for e in r.dir
                     if int(e["first_row"]) < (int(e["event"]["fire_row"]) // chunk) * chunk]
    # ... and one that ends behind its fire row's chunk, and so was carried: resolved by a later call than the one that read it
    carried = [(k, e) for k, r in enumerate(results) for e in r.dir if int(e["event"]["fire_row"]) // chunk < k]
    print("start in the chunk before: %s\ncarried: %s" % ([(k, int(e["first_row"]), int(e["event"]["fire_row"])) for k, e in starts_before],
                                                         [(k, int(e["first_row"]), int(e["rows"]), int(e["event"]["fire_row"])) for k, e in carried]))
    assert starts_before and carried
    assert all(int(e["first_row"]) + int(e["rows"]) > (int(e["event"]["fire_row"]) // chunk + 1) * chunk for _, e in carried)
    assert any(e["slot"] == 0 and 205 <= int(e["event"]["fire_row"]) <= 215 and int(e["first_row"]) < 200 for _, e in starts_before)
    assert any(e["slot"] == 0 and 190 <= int(e["event"]["fire_row"]) < 200 for _, e in carried)
