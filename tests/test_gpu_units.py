"""GPU checks of the FITS data units on the device (csrc/ro_units.hip): the data unit of every captured snapshot, cut to its
recorder's columns, and of every captured raw run, byte-swapped and zero-padded to 2880 bytes -- against the host twins
(ro_snapshot_units_host, ro_raw_units_host) byte for byte in the unit directory, the summary and the units in use, with
guard bytes behind every output and the arena, the source directory and its summary checked unwritten.  The inputs are
synthetic (tests/unitslib.py): arena float i is i + 0.5, so a wrong float names itself.  The decision table holds the four
rooms (exactly the need, one block less, no multiple of 2880, none with d_units NULL).  Only the chain test runs a transform.
Nothing here has a tolerance."""
import numpy as np
import pytest

from rawlib import GUARD as RAW_GUARD
from rawlib import Case as RawCase
from rawlib import L_of
from rawlib import outputs_for as raw_outputs_for
from snapshotslib import PAD
from snapshotslib import Case as SnapCase
from snapshotslib import outputs_for as snap_outputs_for
from unitslib import (BLOCK, CAPTURED, EMPTY, EMU, GUARD, INVALID, LOST, NO_ROOM, SKIPPED, SLOTS, TABLE, WRITTEN, Case, Result,
                      blocks_of, case_from_emu, cut_bytes, host_call, images, outputs_for, refusals, runs, statuses, whole)
from util import add_chirp, noise_iq

pytestmark = pytest.mark.gpu


@pytest.fixture()
def st(ro, torch_cuda):
    with ro.Stft(bins=256, overlap=0) as handle:
        yield handle


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def launch(torch, st, case, d_dir, d_summary, d_arena, d_outs):
    """one resident call on the current stream; nothing is waited for"""
    head = (d_dir if case.dcap else None, case.dcap, d_summary, d_arena if case.arena.size else None, case.arena.size)
    tail = (d_outs[0], d_outs[1] if case.units_bytes else None, case.units_bytes, d_outs[2])
    if case.kind == "raw":
        st.raw_units_resident(*head, *tail, stream=stream_of(torch))
    else:
        st.snapshot_units_resident(*head, case.cols, case.windows, *tail, stream=stream_of(torch))


def device_call(ro, torch, st, case):
    d_dir = up(torch, case.directory) if len(case.directory) else None
    d_summary, d_arena = up(torch, case.summary), up(torch, case.arena) if case.arena.size else None
    d_outs = [up(torch, o) for o in outputs_for(case)]
    launch(torch, st, case, d_dir, d_summary, d_arena, d_outs)
    torch.cuda.synchronize()
    assert d_dir is None or d_dir.cpu().numpy().tobytes() == case.directory.tobytes(), "the source directory was written"
    assert d_summary.cpu().numpy().tobytes() == case.summary.tobytes()
    assert d_arena is None or d_arena.cpu().numpy().tobytes() == case.arena.tobytes(), "the arena was written"
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


# ---- 1. the decision table, the four rooms among it ---------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_on_the_device(ro, torch_cuda, st, case_fn):
    case_fn(ro, device_vs_host(ro, torch_cuda, st))


def test_random_emulator_cases_on_the_device(ro, torch_cuda, st):
    rng = np.random.default_rng(79)
    call = device_vs_host(ro, torch_cuda, st)
    written = 0
    for _ in range(16):
        written += int(call(case_from_emu(ro, EMU.random_case(rng))).summary["written"])
    assert written > 0


# ---- 2. sizes around the block ------------------------------------------------------------------------------------------------
SHAPES = [(1, 719), (1, 720), (1, 721), (3, 240), (3, 241), (65, 11), (65, 12), (64, 45), (64, 46), (719, 1), (720, 1), (721, 1),
          (720, 2)]


@pytest.mark.parametrize("place", ["the whole row", "an odd first column", "the last columns of 1365"])
def test_images_around_the_block(ro, torch_cuda, st, place):
    """units that end just in front of, at and just behind a block's end, as the whole arena row (the contiguous path), from
    column 1 of an arena one column wider, and as the last columns of a 1365-column image; two entries per call, so that the
    second unit starts behind the first one's padding; run twice"""
    call = device_vs_host(ro, torch_cuda, st, twice=True)
    for naxis1, naxis2 in SHAPES:
        cols, first = {"the whole row": (naxis1, 0), "an odd first column": (naxis1 + 1, 1)}.get(place, (1365, 1365 - naxis1))
        d, floats = images(ro, [(naxis2, 3), (naxis2, 3)], cols, pad=5)
        d["offset"] += 5                                          # (the images need not start the arena)
        case = Case(ro, "image", d, floats, 2 * BLOCK * blocks_of(naxis1, naxis2), cols, [(0, 0)] * 3 + [(first, naxis1)] + [(0, 0)] * 4)
        r = call(case)
        assert statuses(r) == [WRITTEN, WRITTEN] and r.dir["naxis1"].tolist() == [naxis1] * 2, (naxis1, naxis2, r.dir)
        for i in range(2):
            assert r.unit(i).tobytes() == cut_bytes(case, i), (place, naxis1, naxis2, i)


def test_raw_runs_around_the_block(ro, torch_cuda, st):
    """samples in {1, 359, 360, 361, 720, 721}: 360 pairs are one block; every run starts an odd multiple of 2 floats into
    the arena, where a 16-byte load would be misaligned; run twice"""
    call = device_vs_host(ro, torch_cuda, st, twice=True)
    sizes = [1, 359, 360, 361, 720, 721]
    d, _ = runs(ro, sizes)
    offset = 2
    for i, n in enumerate(sizes):
        d[i]["offset"] = offset
        offset += 2 * n + (4 if n % 2 == 0 else 2)                # the next odd multiple of 2 behind the run
    assert all((int(o) // 2) % 2 == 1 for o in d["offset"])
    case = Case(ro, "raw", d, offset, BLOCK * sum(blocks_of(2, n) for n in sizes))
    r = call(case)
    assert statuses(r) == [WRITTEN] * 6 and r.dir["naxis2"].tolist() == sizes
    assert r.dir["offset"].tolist() == [0, BLOCK, 2 * BLOCK, 3 * BLOCK, 5 * BLOCK, 7 * BLOCK]
    for i in range(6):
        assert r.unit(i).tobytes() == cut_bytes(case, i), i


# ---- 3. crossing the plan kernel's tile ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", ["everything", "ends at entry 270"])
def test_300_entries_cross_the_plan_kernels_tile(ro, torch_cuda, st, room):
    """300 entries of all four statuses in eight slots: units_plan_kernel walks two tiles and carries the block prefix into the
    second; with the room ending at entry 270, that entry and every writable one behind it are NO_ROOM, the smaller ones
    too; needed_bytes is the room that holds everything, and a second call with it writes all"""
    torch, rng = torch_cuda, np.random.default_rng(300)
    cols = 96
    windows = [(0, 96), (1, 33), (40, 56), (0, 0), (95, 1), (7, 64), (0, 5), (31, 65)]
    items = [(int(r), int(s), int(k)) for r, s, k in zip(rng.integers(1, 40, 300), rng.integers(0, SLOTS, 300),
                                                        rng.choice([CAPTURED] * 8 + [EMPTY, LOST], 300))]
    items[270] = (30, 0, CAPTURED)                                # (writable, and larger than what follows it)
    d, floats = images(ro, items, cols)
    bad = np.flatnonzero(d["status"] == CAPTURED)[5::17]
    bad = bad[bad != 270]
    d["rows"][bad[0::3]] = 0
    d["slot"][bad[1::3]] = 8
    d["offset"][bad[2::3]] = floats
    case = Case(ro, "image", d, floats, 0, cols, windows)
    everything = host_call(ro, case.with_room(1 << 26))
    need = int(everything.summary["needed_bytes"])
    s = everything.summary
    assert min(int(s[k]) for k in ("written", "skipped", "invalid")) > 5 and int(s["no_room"]) == 0 and int(s["units_bytes"]) == need
    assert {int(e["naxis1"]) for e in everything.dir if e["status"] == WRITTEN} == {96, 33, 56, 1, 64, 5, 65}
    call = device_vs_host(ro, torch, st, twice=True)
    if room == "everything":
        r = call(case.with_room(need))
        assert statuses(r) == statuses(everything)
    else:
        at = int(everything.dir[270]["offset"])
        assert everything.dir[270]["status"] == WRITTEN and at > 0
        r = call(case.with_room(at + 3 * BLOCK))                  # 30 rows x 96 columns are four blocks: one short
        assert int(r.summary["needed_bytes"]) == need and int(r.summary["units_bytes"]) == at
        for i in range(300):
            want = everything.dir[i]["status"]
            assert r.dir[i]["status"] == (NO_ROOM if want == WRITTEN and i >= 270 else want), i
        behind = r.dir[271:]
        assert (behind["status"] == NO_ROOM).sum() > 5 and (behind["bytes"][behind["status"] == NO_ROOM] < 3 * BLOCK).any()
        assert (behind["status"] == SKIPPED).any() and (behind["status"] == INVALID).any()
        again = call(case.with_room(int(r.summary["needed_bytes"])))
        assert statuses(again) == statuses(everything)
        r = again
    for i in list(range(0, 300, 11)) + [255, 256, 270, 299]:
        if r.dir[i]["status"] == WRITTEN:
            assert r.unit(i).tobytes() == cut_bytes(case, i), i


# ---- 4. the chain, nothing waited for in between -------------------------------------------------------------------------------
def test_samples_to_units_in_two_chunks(ro, torch_cuda):
    """the shape of test_gpu_raw.py::test_samples_to_raw_in_three_chunks -- 1024 bins, 75 % overlap, two windows, two detectors
    whose recorders keep different windows of the image -- in two chunks of 200 rows: run_resident_windows ->
    ring_put_resident -> events_resident -> snapshots_resident -> raw_resident -> snapshot_units_resident ->
    raw_units_resident per chunk, nothing waited for.  Every output of the two new calls equals the twins applied to the
    downloaded directories and arenas."""
    torch = torch_cuda
    bins, overlap, nrows, chunk, chunks = 1024, 768, 400, 200, 2
    hop = bins - overlap
    shape = (bins, overlap, 48000)
    samples = bins + hop * (nrows - 1)
    iq = noise_iq(np.random.default_rng(31), samples, sigma=0.05)
    for f, spans in ((6000.0, ((60, 62), (189, 191), (203, 206))), (-9000.0, ((100, 101), (250, 253)))):
        for a, b in spans:
            add_chirp(iq, a * hop + 384, ((b - a) * hop + 256) / 48000.0, f, 0.0, 5.0)
    windows = [(300, 40), (628, 25)]
    cols = 65
    slot_windows = [(40, 25), (0, 40)]                       # the primary detects in the second window, the second in the first
    primary = ro.Bands(low_noise=100, noise_width=64, low_detect=630, detect_width=20, avg_bins=5)
    second = ro.Bands(low_noise=700, noise_width=64, low_detect=310, detect_width=20, avg_bins=5)
    dets = [(12, 4), (5, 3)]
    snap, ring_rows, cap, pcap = 40, 256, 24, 8
    stride = cols + 3
    arena_floats = cols * snap * 12
    dcap = 2 * (cap + pcap)
    rcap = pcap + dcap
    raw_arena = 2 * L_of(shape, snap) * 8
    image_room, raw_room = 24 * BLOCK, 8 * BLOCK * blocks_of(2, L_of(shape, snap))
    s = stream_of(torch)
    chunk_samples = (chunk - 1) * hop + bins
    d_iq = [torch.from_numpy(iq[k * chunk * hop:k * chunk * hop + chunk_samples].copy()).cuda() for k in range(chunks)]
    proto = SnapCase(ro, {0: [], 1: []}, snap, ring_rows, cols, 0, arena_floats, pcap=pcap, capacity=cap, stride=stride)
    raw_proto = RawCase(ro, shape, np.zeros(dcap, ro.capi.SNAPSHOT_DTYPE), [(0, 1, 0)], raw_arena, pcap=pcap)
    image_case = Case(ro, "image", np.zeros(dcap, ro.capi.SNAPSHOT_DTYPE), 0, image_room, cols, whole(cols))
    raw_case = Case(ro, "raw", np.zeros(rcap, ro.capi.RAW_CAPTURE_DTYPE), 0, raw_room)
    with ro.Stft(bins=bins, overlap=overlap, bands=primary, extra_bands=[second]) as st:
        d_rows = torch.zeros((chunk, bins), dtype=torch.float32, device="cuda")
        d_image = torch.zeros((chunk, cols), dtype=torch.float32, device="cuda")
        d_recs = torch.zeros((chunk * 12,), dtype=torch.uint8, device="cuda")
        d_extra = torch.zeros((chunk * 12,), dtype=torch.uint8, device="cuda")
        d_ring = torch.full((ring_rows * stride,), float(PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_state = torch.zeros((2 * 32,), dtype=torch.uint8, device="cuda")
        outs = [[up(torch, o) for o in snap_outputs_for(proto)] for _ in range(chunks)]
        raw_outs = [[up(torch, o) for o in raw_outputs_for(raw_proto)] for _ in range(chunks)]
        image_units = [[up(torch, o) for o in outputs_for(image_case)] for _ in range(chunks)]
        raw_units = [[up(torch, o) for o in outputs_for(raw_case)] for _ in range(chunks)]
        d_events = [torch.full((2 * cap * 40,), RAW_GUARD, dtype=torch.uint8, device="cuda") for _ in range(chunks)]
        d_summary = [torch.zeros((2 * 24,), dtype=torch.uint8, device="cuda") for _ in range(chunks)]
        d_pending, d_count = outs[0][2], outs[0][3]
        d_raw_pending, d_raw_count = raw_outs[0][2], raw_outs[0][3]
        torch.cuda.synchronize()
        for k in range(chunks):                              # ---- nothing below waits for the device
            first = k * chunk
            st.run_resident_windows(d_iq[k], ro.RO_IQ_F32, chunk_samples, 0, chunk, d_rows, windows, d_image, d_records=d_recs,
                                    d_extra=d_extra, stream=s)
            st.ring_put_resident(d_image, first, chunk, ring, stream=s)
            st.events_resident(chunk, dets, d_state, d_records=d_recs, d_extra=d_extra, first_row=first, d_events=d_events[k],
                               capacity=cap, d_summary=d_summary[k], stream=s)
            st.snapshots_resident(3, snap, ring, first + chunk, d_pending, d_count, pcap, outs[k][0], outs[k][1], arena_floats,
                                  outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k], stream=s)
            spans = [(d_iq[j], j * chunk * hop, chunk_samples, ro.RO_IQ_F32) for j in range(max(k - 1, 0), k + 1)]
            st.raw_resident(outs[k][0], dcap, outs[k][4], spans, d_raw_pending, d_raw_count, pcap, raw_outs[k][0], raw_outs[k][1],
                            raw_arena, raw_outs[k][4], stream=s)
            st.snapshot_units_resident(outs[k][0], dcap, outs[k][4], outs[k][1], arena_floats, cols, slot_windows,
                                       image_units[k][0], image_units[k][1], image_room, image_units[k][2], stream=s)
            st.raw_units_resident(raw_outs[k][0], rcap, raw_outs[k][4], raw_outs[k][1], raw_arena, raw_units[k][0],
                                  raw_units[k][1], raw_room, raw_units[k][2], stream=s)
        torch.cuda.synchronize()
    written = np.zeros(2, np.int64)
    slots_seen = set()
    for k in range(chunks):
        # the image units against the twin over what the snapshots call left
        snap_dir = outs[k][0].cpu().numpy()[:dcap * 72].view(ro.capi.SNAPSHOT_DTYPE)
        snap_sm = outs[k][4].cpu().numpy()[:64].view(ro.capi.SNAP_SUMMARY_DTYPE)
        arena = outs[k][1].cpu().numpy()[:arena_floats * 4].view(np.float32)
        got = Result(ro, image_case, *[o.cpu().numpy() for o in image_units[k]])
        want_dir, want_units, want_sm = ro.snapshot_units_host(snap_dir, snap_sm, arena, cols, slot_windows, image_room)
        assert got.summary.tobytes() == want_sm.tobytes() and got.dir.tobytes() == want_dir.tobytes(), (k, got.summary, want_sm)
        assert got.units.tobytes() == want_units.tobytes()
        assert int(got.summary["entries"]) == int(snap_sm["resolved"][0]) and int(got.summary["no_room"]) == 0
        for e, u in zip(snap_dir, got.dir):
            assert (u["status"] == WRITTEN) == (e["status"] == CAPTURED)
            if u["status"] == WRITTEN:
                assert (int(u["naxis1"]), int(u["naxis2"])) == (slot_windows[int(e["slot"])][1], int(e["rows"]))
                first_col = slot_windows[int(e["slot"])][0]
                image = arena[int(e["offset"]):int(e["offset"]) + int(e["rows"]) * cols].reshape(-1, cols)
                data = image[:, first_col:first_col + int(u["naxis1"])].astype(">f4").tobytes()
                assert got.units[int(u["offset"]):int(u["offset"]) + len(data)].tobytes() == data
                slots_seen.add(int(e["slot"]))
        written[0] += int(got.summary["written"])
        # the raw units against the twin over what the raw call left
        raw_dir = raw_outs[k][0].cpu().numpy()[:rcap * 72].view(ro.capi.RAW_CAPTURE_DTYPE)
        raw_sm = raw_outs[k][4].cpu().numpy()[:64].view(ro.capi.RAW_SUMMARY_DTYPE)
        arena = raw_outs[k][1].cpu().numpy()[:raw_arena * 4].view(np.float32)
        got = Result(ro, raw_case, *[o.cpu().numpy() for o in raw_units[k]])
        want_dir, want_units, want_sm = ro.raw_units_host(raw_dir, raw_sm, arena, raw_room)
        assert got.summary.tobytes() == want_sm.tobytes() and got.dir.tobytes() == want_dir.tobytes(), (k, got.summary, want_sm)
        assert got.units.tobytes() == want_units.tobytes()
        assert int(got.summary["entries"]) == int(raw_sm["resolved"][0]) and int(got.summary["no_room"]) == 0
        written[1] += int(got.summary["written"])
    print("units written: images %d, raw %d; slots %s" % (written[0], written[1], sorted(slots_seen)))
    assert written[0] >= 3 and written[1] >= 2 and slots_seen == {0, 1}


# ---- 5. beyond 2^32 bytes ------------------------------------------------------------------------------------------------------
def test_units_and_sources_beyond_4_gib(ro, torch_cuda, st):
    """one arena and one units buffer of a little over 4 GiB each: a raw run of 2^29 + 1 pairs whose unit crosses byte 2^32, a
    run of 361 pairs behind it whose unit lies beyond 2^32 bytes, and an image of 3 rows x 615 columns, window (1, 613), whose
    source lies beyond 2^32 bytes of the same arena.  The large unit is compared on the device in three slices of 2^20
    floats -- its head, across byte 2^32, its tail with the padding -- the small ones against the twins"""
    torch = torch_cuda
    big, small, cols, rows = (1 << 29) + 1, 361, 615, 3
    off_big, off_small = 2, 2 + 2 * big + 2
    off_image = off_small + 2 * small + 3
    floats = off_image + rows * cols + 7
    assert 4 * off_small > 1 << 32 and off_big // 2 % 2 == 1
    d_arena = torch.arange(floats, dtype=torch.int32, device="cuda")          # (a bit copy: any pattern will do)
    d_arena[off_small:] += 0x3f000000                                           # ... the small sources: floats around 0.5
    blocks_big, blocks_small = blocks_of(2, big), blocks_of(2, small)
    room = (blocks_big + blocks_small) * BLOCK
    guard = 4096
    d_units = torch.full((room + guard,), GUARD, dtype=torch.uint8, device="cuda")
    raw_dir = np.zeros(3, ro.capi.RAW_CAPTURE_DTYPE)
    raw_dir["samples"], raw_dir["offset"], raw_dir["status"] = [big, 5, small], [off_big, 0, off_small], [CAPTURED, LOST, CAPTURED]
    raw_sm = np.zeros(1, ro.capi.RAW_SUMMARY_DTYPE)
    raw_sm["resolved"] = 3
    d_unit_dir = up(torch, np.full(3 * 32 + 64, GUARD, np.uint8))
    d_unit_sm = up(torch, np.full(64 + 64, GUARD, np.uint8))
    d_dir, d_sm = up(torch, raw_dir), up(torch, raw_sm)
    st.raw_units_resident(d_dir, 3, d_sm, d_arena, floats, d_unit_dir, d_units, room, d_unit_sm, stream=stream_of(torch))
    torch.cuda.synchronize()
    unit_dir = d_unit_dir.cpu().numpy()
    sm = d_unit_sm.cpu().numpy()
    assert np.all(unit_dir[96:] == GUARD) and np.all(sm[64:] == GUARD)
    unit_dir, sm = unit_dir[:96].view(ro.capi.FITS_UNIT_DTYPE), sm[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
    assert unit_dir["status"].tolist() == [WRITTEN, SKIPPED, WRITTEN] and unit_dir["offset"].tolist() == [0, 0, blocks_big * BLOCK]
    assert unit_dir["bytes"].tolist() == [8 * big, 0, 8 * small] and unit_dir["naxis2"].tolist() == [big, 0, small]
    assert blocks_big * BLOCK > 1 << 32 and [int(sm[k]) for k in ("written", "skipped", "units_bytes", "needed_bytes")] == [2, 1, room, room]
    assert bool((d_units[room:] == GUARD).all()), "bytes behind the units were touched"
    words = d_units[:room].view(torch.int32)

    def swapped(t):
        return t.contiguous().view(torch.uint8).reshape(-1, 4).flip(1).contiguous().view(torch.int32).reshape(-1)
    n, data = 1 << 20, 2 * big                                                  # floats of a slice, floats of the large unit
    assert torch.equal(words[:n], swapped(d_arena[off_big:off_big + n])), "the head"
    line = (1 << 30) - n // 2                                                   # unit float 2^30 is byte 2^32
    across = torch.zeros(n, dtype=torch.int32, device="cuda")
    across[:data - line] = swapped(d_arena[off_big + line:off_big + data])
    assert data - line == n // 2 + 2
    end = blocks_big * BLOCK // 4                                               # the unit's end in floats, padding included
    assert torch.equal(words[line:min(line + n, end)], across[:min(n, end - line)]), "across byte 2^32, and the padding behind"
    tail = torch.zeros(n, dtype=torch.int32, device="cuda")
    tail[:data - (end - n)] = swapped(d_arena[off_big + end - n:off_big + data])
    assert 0 < end - data < 720 and torch.equal(words[end - n:end], tail), "the tail with its padding"
    # the small run against the twin over its own floats
    own = d_arena[off_small:off_small + 2 * small].cpu().numpy().view(np.float32)
    one, _ = runs(ro, [small])
    want = host_call(ro, Case(ro, "raw", one, own, BLOCK * blocks_small))
    got = d_units[blocks_big * BLOCK:room].cpu().numpy()
    assert got.tobytes() == want.units.tobytes() and unit_dir[2:].tobytes()[8:] == want.dir.tobytes()[8:]
    # the image: its source beyond 2^32 bytes of the same arena, its unit at the front of the same buffer
    snap_dir = np.zeros(1, ro.capi.SNAPSHOT_DTYPE)
    snap_dir["rows"], snap_dir["offset"], snap_dir["slot"], snap_dir["status"] = rows, off_image, 6, CAPTURED
    snap_sm = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
    snap_sm["resolved"] = 1
    d_unit_dir = up(torch, np.full(32 + 64, GUARD, np.uint8))
    d_units[:] = GUARD
    d_dir, d_sm = up(torch, snap_dir), up(torch, snap_sm)
    st.snapshot_units_resident(d_dir, 1, d_sm, d_arena, floats, cols, [None] * 6 + [(1, 613)], d_unit_dir, d_units, room,
                               d_unit_sm, stream=stream_of(torch))
    torch.cuda.synchronize()
    own = d_arena[off_image:off_image + rows * cols].cpu().numpy().view(np.float32)
    one, _ = images(ro, [(rows, 6)], cols)
    want = host_call(ro, Case(ro, "image", one, own, 3 * BLOCK, cols, [(0, 0)] * 6 + [(1, 613), (0, 0)]))
    assert statuses(want) == [WRITTEN] and len(want.units) == 3 * BLOCK and 4 * off_image > 1 << 32
    assert d_units[:3 * BLOCK].cpu().numpy().tobytes() == want.units.tobytes()
    assert bool((d_units[3 * BLOCK:] == GUARD).all()), "bytes behind the image's unit were touched"
    assert d_unit_dir.cpu().numpy()[:32].tobytes() == want.dir.tobytes()
    assert d_unit_sm.cpu().numpy()[:64].tobytes() == want.summary.tobytes()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["images", "raw"])
def test_refusals_with_a_handle(ro, torch_cuda, st, raw):
    torch = torch_cuda
    lib = ro.library()
    cols = 10
    d, floats = runs(ro, [30]) if raw else images(ro, [(6, 0)], cols)
    case = Case(ro, "raw", d, floats, 2 * BLOCK) if raw else Case(ro, "image", d, floats, 2 * BLOCK, cols, whole(cols))
    d_dir, d_sum, d_arena = up(torch, case.directory), up(torch, case.summary), up(torch, case.arena)
    d_outs = [up(torch, o) for o in outputs_for(case)]
    ptr = lambda t: t.data_ptr()
    who = "ro_stft_raw_units_resident" if raw else "ro_stft_snapshot_units_resident"

    def call(**kw):
        a = dict(dir=ptr(d_dir), dcap=1, summary=ptr(d_sum), arena=ptr(d_arena), arena_floats=floats, cols=cols,
                 windows=case.windows, unit_dir=ptr(d_outs[0]), units=ptr(d_outs[1]), units_bytes=2 * BLOCK, out=ptr(d_outs[2]))
        a.update(kw)
        if a["units"] == "arena":
            a["units"] = ptr(d_arena) + 4 * floats - 8 - (ptr(d_arena) + 4 * floats - 8) % 16        # inside the arena, aligned
        elif a["units"] == "arena end":
            a["units"] = ptr(d_arena) - 2 * BLOCK + 16                # its last 16 bytes are the arena's first
        if raw:
            return lib.ro_stft_raw_units_resident(st._h, a["dir"], a["dcap"], a["summary"], a["arena"], a["arena_floats"],
                                                  a["unit_dir"], a["units"], a["units_bytes"], a["out"], stream_of(torch))
        w = a["windows"]
        if isinstance(w, dict):
            w = [w.get(i, case.windows[i]) for i in range(SLOTS)]
        arr = None if w is None else (ro.capi.BandWindow * SLOTS)(*[ro.capi.BandWindow(*x) for x in w])
        return lib.ro_stft_snapshot_units_resident(st._h, a["dir"], a["dcap"], a["summary"], a["arena"], a["arena_floats"],
                                                   a["cols"], arr, a["unit_dir"], a["units"], a["units_bytes"], a["out"],
                                                   stream_of(torch))
    for kw, word in refusals("d_", raw) + [(dict(units=ptr(d_outs[1]) + 8), "d_units is not aligned")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith(who + ":"), (kw, text)
    torch.cuda.synchronize()
    for o, before in zip(d_outs, outputs_for(case)):
        assert o.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"
    assert call(units=None, units_bytes=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert d_outs[2].cpu().numpy()[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)["written"][0] == 1
