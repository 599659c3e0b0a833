"""GPU checks of the grey-level previews on the device (csrc/ro_levels.hip): each snapshot's ln image as uint8, for the event
snapshots of an arena and for the periodic snapshots of a plan.  Every WRITTEN image is held to two yardsticks.
A, exact: the image's rows uploaded contiguously (a ring image un-wrapped on the host first) through the existing
ro_stft_ln_tile_resident over its rectangle -- d_u8 and d_minmax equal the new call's levels and range byte for byte (an
all-zero image: the old call pins no range; the new one gives {+inf, -inf} and zeros).
B, the twin (ro_snapshot_levels_host, ro_periodic_levels_host): directory, summary, padding, guards, the untouched tail and
the unwritten sources byte for byte; ranges within 2 ulp (test_gpu_ln_tile.ln_close); levels within 1 wherever the image's ln
span is at least 1 -- two logf that differ by 2 ulp of a |ln| below 40 are at most 1e-5 apart, 2.6e-3 levels at that span, so
no level moves by more than one; flat and narrower images are held to A only -- and the share of differing pixels per test
below 2e-3, the bar tests/test_gpu_ln_tile.py holds for the same two logf on the same kind of data: the pixels of every
test here are magnitudes of noise plus a tone (levelslib.magnitudes), and every test asserts the share over the images it
held to the twin.  Every case runs twice with equal bytes."""
import ctypes as C

import numpy as np
import pytest

import periodiclib as P
import unitslib as U
from levelslib import (GUARD, LBLOCK, NGUARD, PERIODIC_TABLE, TABLE, WRITTEN, PeriodicResult, Result, blocks_of, host_call, magnitudes,
                       outputs_for, pcase, periodic_host_call, periodic_outputs_for, periodic_refusals, ring_image, room_of, snapshot_refusals,
                       source_image)
from snapshotslib import Case as SnapCase
from snapshotslib import outputs_for as snap_outputs_for
from test_gpu_ln_tile import ln_close
from test_gpu_units import SHAPES
from util import add_chirp, noise_iq

pytestmark = pytest.mark.gpu

YARD_BINS = 2048                                          # the yardstick handle: rows of up to 2048 columns
SPAN_FOR_B = 1.0                                          # ln span from which the levels are held to the twin's (see above)
SHARE = 2e-3


@pytest.fixture()
def st(ro, torch_cuda):
    with ro.Stft(bins=256, overlap=0) as handle:
        yield handle


@pytest.fixture(scope="module")
def yard(ro, torch_cuda):
    with ro.Stft(bins=YARD_BINS, overlap=0) as handle:
        yield handle


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


class Tally:
    """pixels compared against the twin and how many of them differ, over one test"""

    def __init__(self):
        self.pixels = self.differing = self.images = 0

    def share(self):
        return self.differing / max(self.pixels, 1)


def yardstick_a(torch, yard, image):
    """(levels uint8 [rows, cols], minmax float32 [2]) of ro_stft_ln_tile_resident over the image's rectangle"""
    rows, cols = image.shape
    assert cols <= YARD_BINS
    d_rows = torch.zeros((rows, YARD_BINS), dtype=torch.float32, device="cuda")
    d_rows[:, :cols] = torch.from_numpy(image).cuda()
    d_u8 = torch.full((rows, cols), 77, dtype=torch.uint8, device="cuda")
    d_mm = torch.zeros(2, dtype=torch.float32, device="cuda")
    yard.ln_tile_resident(d_rows, rows, 0, cols, d_u8=d_u8, d_minmax=d_mm, stream=stream_of(torch))
    torch.cuda.synchronize()
    return d_u8.cpu().numpy(), d_mm.cpu().numpy()


def hold_image(torch, yard, tally, image, got_px, got_range, want_px, want_range, what):
    """one WRITTEN image against both yardsticks"""
    u8, mm = yardstick_a(torch, yard, image)
    rng = np.array([got_range["ln_min"], got_range["ln_max"]], np.float32)
    if image.any():
        assert rng.tobytes() == mm.tobytes(), (what, rng, mm)
    else:
        assert rng[0] == np.inf and rng[1] == -np.inf and not got_px.any(), what
    assert np.array_equal(got_px, u8), what
    want = np.array([want_range["ln_min"], want_range["ln_max"]], np.float32)
    if image.any():
        assert ln_close(rng, want), (what, rng, want)
    else:
        assert rng.tobytes() == want.tobytes()
    if image.any() and rng[1] - rng[0] >= SPAN_FOR_B:
        d = np.abs(got_px.astype(np.int16) - want_px.astype(np.int16))
        assert d.max() <= 1, (what, int(d.max()))
        tally.pixels += d.size
        tally.differing += int((d != 0).sum())
        tally.images += 1


# ---- event snapshots -----------------------------------------------------------------------------------------------------------
def launch(torch, st, case, d_dir, d_summary, d_arena, d_outs):
    st.snapshot_levels_resident(d_dir if case.dcap else None, case.dcap, d_summary, d_arena if case.arena.size else None,
                                case.arena.size, case.cols, case.windows, d_outs[0], d_outs[1], d_outs[2] if case.units_bytes else None,
                                case.units_bytes, d_outs[3], stream=stream_of(torch))


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


def hold_result(torch, yard, tally, case, got, want):
    """a device Result against the twin's and, image by image, against both yardsticks"""
    assert got.summary.tobytes() == want.summary.tobytes(), (got.summary, want.summary)
    assert got.dir.tobytes() == want.dir.tobytes(), (got.dir, want.dir)
    assert got.raw[0].tobytes() == want.raw[0].tobytes() and got.raw[3].tobytes() == want.raw[3].tobytes()
    assert len(got.levels) == len(want.levels)
    for d in got.written():
        hold_image(torch, yard, tally, source_image(case, d), got.pixels(d), got.ranges[d], want.pixels(d), want.ranges[d], d)


def device_checked(ro, torch, st, yard, tally):
    def call(case):
        got = device_call(ro, torch, st, case)
        hold_result(torch, yard, tally, case, got, host_call(ro, case))
        assert device_call(ro, torch, st, case).same_bytes(got), "two runs differ"
        return got
    return call


@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_snapshot_decision_table_on_the_device(ro, torch_cuda, st, yard, case_fn):
    tally = Tally()
    case_fn(ro, device_checked(ro, torch_cuda, st, yard, tally))
    print("%s: %d of %d pixels differ from the twin's in %d images" % (case_fn.__name__, tally.differing, tally.pixels, tally.images))
    assert tally.images >= 1 and tally.share() < SHARE, tally.share()


@pytest.mark.parametrize("place", ["the whole row", "an odd first column", "the last columns of 1365"])
def test_snapshot_images_around_the_block(ro, torch_cuda, st, yard, place):
    """pixel counts just below, at and just above a multiple of 720 (test_gpu_units.SHAPES), as the whole arena row, from
    column 1 of a cols + 4 stride, and as the last columns of a 1365-column row; two images per call, so that the second
    starts behind the first one's padding"""
    tally = Tally()
    call = device_checked(ro, torch_cuda, st, yard, tally)
    rng = np.random.default_rng(len(place))
    for naxis1, naxis2 in SHAPES:
        cols, first = {"the whole row": (naxis1, 0), "an odd first column": (naxis1 + 4, 1)}.get(place, (1365, 1365 - naxis1))
        d, floats = U.images(ro, [(naxis2, 3), (naxis2, 3)], cols, pad=5)
        d["offset"] += 5
        case = U.Case(ro, "image", d, magnitudes(rng, floats), 2 * LBLOCK * blocks_of(naxis1, naxis2), cols,
                      [(0, 0)] * 3 + [(first, naxis1)] + [(0, 0)] * 4)
        r = call(case)
        assert r.dir["status"].tolist() == [WRITTEN, WRITTEN] and r.dir["offset"].tolist() == [0, LBLOCK * blocks_of(naxis1, naxis2)]
    print("%s: %d of %d pixels differ from the twin's in %d images" % (place, tally.differing, tally.pixels, tally.images))
    assert tally.images == 2 * len(SHAPES) and tally.share() < SHARE, tally.share()


@pytest.mark.parametrize("order", ["min first, max last", "max first, min last"])
def test_snapshot_fold_across_blocks(ro, torch_cuda, st, yard, order):
    """an image of six blocks whose minimum lies in the first block and whose maximum in the last, and the reverse; and,
    in the same call, a one-block image: the fold of one image does not read another's blocks"""
    cols, rows = 100, 40
    d, floats = U.images(ro, [(7, 0), (rows, 0), (7, 0)], cols)
    arena = magnitudes(np.random.default_rng(44), floats)
    lo, hi = 7 * cols, (7 + rows) * cols - 1
    arena[lo], arena[hi] = (1e-4, 1e4) if order.startswith("min") else (1e4, 1e-4)
    tally = Tally()
    r = device_checked(ro, torch_cuda, st, yard, tally)(U.Case(ro, "image", d, arena, 8 * LBLOCK, cols, U.whole(cols)))
    assert r.dir["status"].tolist() == [WRITTEN] * 3 and blocks_of(cols, rows) == 6
    assert abs(r.ranges[1]["ln_min"] - np.log(1e-4)) < 1e-5 and abs(r.ranges[1]["ln_max"] - np.log(1e4)) < 1e-5
    px = r.pixels(1).reshape(-1)
    assert (px[0], px[-1]) == ((0, 255) if order.startswith("min") else (255, 0))
    assert r.ranges[0]["ln_min"] > -5 and r.ranges[2]["ln_max"] < 5 and tally.share() < SHARE


def test_snapshot_refusals_with_a_handle(ro, torch_cuda, st):
    torch = torch_cuda
    lib = ro.library()
    cols = 10
    d, floats = U.images(ro, [(6, 0)], cols)
    case = U.Case(ro, "image", d, floats, 2 * LBLOCK, cols, U.whole(cols))
    d_dir, d_sum, d_arena = up(torch, case.directory), up(torch, case.summary), up(torch, case.arena)
    d_outs = [up(torch, o) for o in outputs_for(case)]
    ptr = lambda t: t.data_ptr()

    def call(**kw):
        a = dict(dir=ptr(d_dir), dcap=1, summary=ptr(d_sum), arena=ptr(d_arena), arena_floats=floats, cols=cols, windows=case.windows,
                 level_dir=ptr(d_outs[0]), ranges=ptr(d_outs[1]), levels=ptr(d_outs[2]), levels_bytes=2 * LBLOCK, out=ptr(d_outs[3]))
        a.update(kw)
        if a["levels"] == "arena":
            a["levels"] = ptr(d_arena) + 4 * floats - 8 - (ptr(d_arena) + 4 * floats - 8) % 16        # inside the arena, aligned
        elif a["levels"] == "arena end":
            a["levels"] = ptr(d_arena) - 2 * LBLOCK + 16              # its last 16 bytes are the arena's first
        w = a["windows"]
        if isinstance(w, dict):
            w = [w.get(i, case.windows[i]) for i in range(U.SLOTS)]
        arr = None if w is None else (ro.capi.BandWindow * U.SLOTS)(*[ro.capi.BandWindow(*x) for x in w])
        return lib.ro_stft_snapshot_levels_resident(st._h, a["dir"], a["dcap"], a["summary"], a["arena"], a["arena_floats"], a["cols"],
                                                    arr, a["level_dir"], a["ranges"], a["levels"], a["levels_bytes"], a["out"],
                                                    stream_of(torch))
    for kw, word in snapshot_refusals("d_") + [(dict(levels=ptr(d_outs[2]) + 8), "d_levels is not aligned")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_stft_snapshot_levels_resident:"), (kw, text)
    torch.cuda.synchronize()
    for o, before in zip(d_outs, outputs_for(case)):
        assert o.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"
    assert call(levels=None, levels_bytes=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert d_outs[3].cpu().numpy()[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)["written"][0] == 1


# ---- periodic snapshots --------------------------------------------------------------------------------------------------------
def periodic_device_call(ro, torch, st, case, directory):
    d_ring = up(torch, case.ring)
    d_outs = [up(torch, o) for o in periodic_outputs_for(case, directory)]
    ring = case.ring_struct(ro, d_ring.data_ptr())
    st.periodic_levels_resident(ring, case.recorders, directory, d_outs[0], d_outs[1] if room_of(case) else None, room_of(case),
                                stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_ring.cpu().numpy().tobytes() == case.ring.tobytes(), "the ring was written"
    return PeriodicResult(ro, case, directory, *[o.cpu().numpy() for o in d_outs])


def hold_periodic(torch, yard, tally, case, got, want):
    assert len(got.levels) == len(want.levels)
    for d in got.written():
        hold_image(torch, yard, tally, ring_image(case, got.dir[d]), got.pixels(d), got.ranges[d], want.pixels(d), want.ranges[d], d)


def periodic_device_checked(ro, torch, st, yard, tally):
    def call(case):
        directory, _, _ = P.plan_call(ro, case)
        got = periodic_device_call(ro, torch, st, case, directory)
        hold_periodic(torch, yard, tally, case, got, periodic_host_call(ro, case, directory))
        assert periodic_device_call(ro, torch, st, case, directory).same_bytes(got), "two runs differ"
        return got
    return call


@pytest.mark.parametrize("case_fn", PERIODIC_TABLE, ids=lambda f: f.__name__)
def test_periodic_decision_table_on_the_device(ro, torch_cuda, st, yard, case_fn):
    tally = Tally()
    case_fn(ro, periodic_device_checked(ro, torch_cuda, st, yard, tally))
    print("%s: %d of %d pixels differ from the twin's in %d images" % (case_fn.__name__, tally.differing, tally.pixels, tally.images))
    assert tally.images >= 1 and tally.share() < SHARE, tally.share()


@pytest.mark.parametrize("place", ["the whole row", "an odd first column", "the last columns of 1365"])
def test_periodic_images_around_the_block(ro, torch_cuda, st, yard, place):
    """test_gpu_units.SHAPES as the whole ring row, from column 1 of a ring with stride = cols + 3, and as the last columns of a
    1365-column row; two snapshots per call, the second of which straddles nothing but starts behind the first one's padding"""
    tally = Tally()
    call = periodic_device_checked(ro, torch_cuda, st, yard, tally)
    rng = np.random.default_rng(len(place) + 1)
    for naxis1, S in SHAPES:
        cols, first, stride = {"the whole row": (naxis1, 0, naxis1), "an odd first column": (naxis1 + 1, 1, naxis1 + 4)}.get(
            place, (1365, 1365 - naxis1, 1365))
        ring = np.full((2 * S + 3, stride), P.PAD, np.float32)
        ring[:, :cols] = magnitudes(rng, (2 * S + 3) * cols).reshape(-1, cols)
        r = call(P.Case([(S, first, naxis1)], 2 * S + 2, 2 * S + 3, cols, 2 * P.BLOCK * P.blocks_of(naxis1, S), ring=ring))
        assert r.dir["status"].tolist() == [P.WRITTEN] * 2 and r.dir["offset"].tolist() == [0, P.BLOCK * P.blocks_of(naxis1, S)]
    print("%s: %d of %d pixels differ from the twin's in %d images" % (place, tally.differing, tally.pixels, tally.images))
    assert tally.images == 2 * len(SHAPES) and tally.share() < SHARE, tally.share()


@pytest.mark.parametrize("order", ["min first, max last", "max first, min last"])
def test_periodic_fold_across_blocks(ro, torch_cuda, st, yard, order):
    """a ring image of six blocks that straddles the ring's last slot, its minimum in the first block and its maximum in the
    last, and the reverse, in front of two one-block images of another recorder"""
    cols, S, ring_rows = 100, 40, 64
    H = 2 * S + 2                                            # snapshot 1 is rows [40, 80): slots 40 ... 63, 0 ... 15
    ring = magnitudes(np.random.default_rng(45), ring_rows * cols).reshape(ring_rows, cols)
    ring[40 % ring_rows, 0], ring[79 % ring_rows, cols - 1] = (1e-4, 1e4) if order.startswith("min") else (1e4, 1e-4)
    tally = Tally()
    case = P.Case([(S, 0, cols), (7, 10, 80)], H, ring_rows, cols, 16 * P.BLOCK, next_index=[1, 9], ring=ring)
    r = periodic_device_checked(ro, torch_cuda, st, yard, tally)(case)
    assert r.dir["status"].tolist() == [P.WRITTEN] * 3 and r.dir["rows"].tolist() == [S, 7, 7]
    assert abs(r.ranges[0]["ln_min"] - np.log(1e-4)) < 1e-5 and abs(r.ranges[0]["ln_max"] - np.log(1e4)) < 1e-5
    px = r.pixels(0).reshape(-1)
    assert (px[0], px[-1]) == ((0, 255) if order.startswith("min") else (255, 0)) and tally.share() < SHARE


@pytest.mark.parametrize("base", [(1 << 31) + 5, (1 << 33) + 5], ids=["2^31", "2^33"])
def test_periodic_row_indices_beyond_int32(ro, torch_cuda, st, yard, base):
    """the case of test_gpu_periodic.py::test_row_indices_beyond_int32: next_index x S just behind 2^31 + 5 and 2^33 + 5 in a
    23-slot ring, two full snapshots and a final one of 2 rows for two recorders, their slots from int64 rows"""
    S = 7
    k = -(-base // S)
    while (k * S) % 23 + 2 * S + 2 <= 23:
        k += 1
    H = (k + 2) * S + 2
    case = pcase(base % 1000, [(S, 1, 9), (S, 0, 12)], H, 23, 12, 8 * P.BLOCK, final=True, next_index=[k, k + 1], stride=15)
    tally = Tally()
    r = periodic_device_checked(ro, torch_cuda, st, yard, tally)(case)
    print("%d of %d pixels differ from the twin's in %d images" % (tally.differing, tally.pixels, tally.images))
    assert tally.images >= 1 and tally.share() < SHARE, tally.share()
    assert r.dir["first_row"].tolist() == [k * S, (k + 1) * S, (k + 2) * S, (k + 1) * S, (k + 2) * S] and len(r.written()) == 5
    assert base <= k * S < base + 23 * S


def test_periodic_refusals_with_a_handle(ro, torch_cuda, st):
    torch = torch_cuda
    lib = ro.library()
    case = P.Case([(4, 1, 6), (3, 0, 2)], 11, 12, 10, 5 * P.BLOCK)
    directory, _, _ = P.plan_call(ro, case)
    assert directory["status"].tolist() == [P.WRITTEN] * 5
    d_ring = up(torch, case.ring)
    before, ranges_before = P.guarded(5 * LBLOCK, 64), P.guarded(40, 64)
    d_levels, d_ranges = up(torch, before), up(torch, ranges_before)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(**kw):
        a = dict(ring_rows_ptr=d_ring.data_ptr(), recorders=True, count=2, dir=True, entries=5, ranges=d_ranges.data_ptr(),
                 levels=d_levels.data_ptr(), levels_bytes=5 * LBLOCK)
        a.update(kw)
        desc = ro.capi.RowRing(a["ring_rows_ptr"], 10, 12, 10, 0)
        for k, v in a.get("ring_fields", {}).items():
            setattr(desc, k, v)
        recs = ro.periodic_recorders(case.recorders)
        for i, r in a.get("recs", {}).items():
            recs[i] = r
        d = directory.copy()
        for i, fields in a.get("entry", {}).items():
            for k, v in fields.items():
                d[i][k] = v
        if a["levels"] == "ring":
            a["levels"] = d_ring.data_ptr() + 4 * 120 - 16                            # inside the ring, aligned
        elif a["levels"] == "ring end":
            a["levels"] = d_ring.data_ptr() - 5 * LBLOCK + 16                         # its last 16 bytes are the ring's first
        return lib.ro_stft_periodic_levels_resident(st._h, None if "ring" in kw and kw["ring"] is None else C.byref(desc),
                                                    p(recs) if a["recorders"] else None, a["count"], p(d) if a["dir"] else None,
                                                    a["entries"], a["ranges"], a["levels"], a["levels_bytes"], stream_of(torch))
    for kw, word in periodic_refusals("d_") + [(dict(levels=d_levels.data_ptr() + 8), "d_levels is not aligned")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_stft_periodic_levels_resident:"), (kw, text)
    torch.cuda.synchronize()
    assert d_levels.cpu().numpy().tobytes() == before.tobytes() and d_ranges.cpu().numpy().tobytes() == ranges_before.tobytes()
    assert call(dir=None, entries=0, ranges=None) == 0 and call(levels=None, levels_bytes=0, entries=0) == 0
    torch.cuda.synchronize()
    assert d_levels.cpu().numpy().tobytes() == before.tobytes(), "a call without a WRITTEN entry launched something"
    assert call() == 0
    torch.cuda.synchronize()
    want = periodic_host_call(ro, case, directory)
    got = PeriodicResult(ro, case, directory, d_ranges.cpu().numpy()[:40 + NGUARD * 8], d_levels.cpu().numpy()[:5 * LBLOCK + 64])
    assert len(got.levels) == len(want.levels) == 5 * LBLOCK and all(got.pixels(i).shape == want.pixels(i).shape for i in range(5))


# ---- the chain, nothing waited for in between ----------------------------------------------------------------------------------
def test_samples_to_levels_in_three_chunks(ro, torch_cuda, yard):
    """256 bins, overlap 192, 200 rows of noise, a tone and two bursts in chunks of 61, 90 and 49 rows: run_resident_windows ->
    ring_put_resident -> events_resident -> snapshots_resident -> snapshot_levels_resident, and the host plan ->
    periodic_units_resident -> periodic_levels_resident, per chunk on one stream, nothing waited for.  Every chunk's levels
    are held to both yardsticks over what the chain left: the downloaded directories, arenas and image rows"""
    torch = torch_cuda
    bins, overlap, total = 256, 192, 200
    hop = bins - overlap
    chunks = [(0, 61), (61, 90), (151, 49)]
    iq, windows, cols, primary, det, snap = chain_input(ro)
    stride, ring_rows, cap, pcap = cols + 3, 128, 8, 4
    recorders = [(7, 0, 30), (5, 31, 20)]
    slot_windows = [(30, 21)]                                # the event recorder keeps the second window
    room = 40 * P.BLOCK
    arena_floats = cols * snap * 6
    dcap = cap + pcap
    levels_room = 8 * LBLOCK
    s = stream_of(torch)
    d_iq = [torch.from_numpy(iq[a * hop:a * hop + (n - 1) * hop + bins].copy()).cuda() for a, n in chunks]
    nxt = np.zeros(2, np.int64)
    plans = []
    proto = SnapCase(ro, {0: []}, snap, ring_rows, cols, 0, arena_floats, pcap=pcap, capacity=cap, stride=stride)
    level_case = U.Case(ro, "image", np.zeros(dcap, ro.capi.SNAPSHOT_DTYPE), 0, levels_room, cols, slot_windows + [(0, 0)] * 7)
    with ro.Stft(bins=bins, overlap=overlap, bands=primary) as st:
        d_rows = torch.zeros((90, bins), dtype=torch.float32, device="cuda")
        d_image = [torch.zeros((n, cols), dtype=torch.float32, device="cuda") for _, n in chunks]
        d_recs = torch.zeros((90 * 12,), dtype=torch.uint8, device="cuda")
        d_ring = torch.full((ring_rows * stride,), float(P.PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_state = torch.zeros((32,), dtype=torch.uint8, device="cuda")
        outs = [[up(torch, o) for o in snap_outputs_for(proto)] for _ in chunks]
        d_events = [torch.full((cap * 40,), GUARD, dtype=torch.uint8, device="cuda") for _ in chunks]
        d_summary = [torch.zeros((24,), dtype=torch.uint8, device="cuda") for _ in chunks]
        d_pending, d_count = outs[0][2], outs[0][3]
        d_levels = [[up(torch, o) for o in outputs_for(level_case)] for _ in chunks]
        d_units = [up(torch, P.guarded(room, NGUARD * 64)) for _ in chunks]
        d_plevels = [up(torch, P.guarded(room // 4, NGUARD * 64)) for _ in chunks]
        d_pranges = [up(torch, P.guarded(64 * 8, NGUARD * 8)) for _ in chunks]
        torch.cuda.synchronize()
        for k, (first, n) in enumerate(chunks):              # ---- nothing below waits for the device
            st.run_resident_windows(d_iq[k], ro.RO_IQ_F32, (n - 1) * hop + bins, 0, n, d_rows, windows, d_image[k], d_records=d_recs,
                                    stream=s)
            st.ring_put_resident(d_image[k], first, n, ring, stream=s)
            st.events_resident(n, [det], d_state, d_records=d_recs, first_row=first, d_events=d_events[k], capacity=cap,
                               d_summary=d_summary[k], stream=s)
            st.snapshots_resident(1, snap, ring, first + n, d_pending, d_count, pcap, outs[k][0], outs[k][1], arena_floats,
                                  outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k], stream=s)
            st.snapshot_levels_resident(outs[k][0], dcap, outs[k][4], outs[k][1], arena_floats, cols, slot_windows, d_levels[k][0],
                                        d_levels[k][1], d_levels[k][2], levels_room, d_levels[k][3], stream=s)
            directory, sm = ro.periodic_plan(recorders, nxt, first + n, k == len(chunks) - 1, ring_rows, cols, room, 64)
            st.periodic_units_resident(ring, recorders, directory, d_units[k], room, stream=s)
            st.periodic_levels_resident(ring, recorders, directory, d_pranges[k], d_plevels[k], room // 4, stream=s)
            plans.append((directory, sm))
        torch.cuda.synchronize()
        image = np.concatenate([d.cpu().numpy() for d in d_image])
    assert image.shape == (total, cols) and np.isfinite(image).all() and (image > 0).all()
    tally, events_written, periodic_written = Tally(), 0, 0
    for k, (first, n) in enumerate(chunks):
        # the event snapshots' levels against the twin over what the snapshots call left
        case = U.Case.__new__(U.Case)
        case.__dict__.update(level_case.__dict__)
        case.directory = outs[k][0].cpu().numpy()[:dcap * 72].view(ro.capi.SNAPSHOT_DTYPE).copy()
        case.summary = outs[k][4].cpu().numpy()[:64].view(ro.capi.SNAP_SUMMARY_DTYPE).copy()
        case.arena = outs[k][1].cpu().numpy()[:arena_floats * 4].view(np.float32).copy()
        got = Result(ro, case, *[o.cpu().numpy() for o in d_levels[k]])
        hold_result(torch, yard, tally, case, got, host_call(ro, case))
        assert int(got.summary["entries"]) == int(case.summary["resolved"][0]) and int(got.summary["no_room"]) == 0
        events_written += len(got.written())
        # the periodic levels against the twin over the ring as it stood behind this chunk
        directory, sm = plans[k]
        head = first + n
        host_ring = np.full((ring_rows, stride), P.PAD, np.float32)
        for r in range(max(head - ring_rows, 0), head):
            host_ring[r % ring_rows, :cols] = image[r]
        pcase = P.Case(recorders, head, ring_rows, cols, room, ring=host_ring)
        pgot = PeriodicResult(ro, pcase, directory, d_pranges[k].cpu().numpy()[:len(directory) * 8 + NGUARD * 8],
                              d_plevels[k].cpu().numpy())
        hold_periodic(torch, yard, tally, pcase, pgot, periodic_host_call(ro, pcase, directory))
        assert len(pgot.levels) == int(sm["units_bytes"]) // 4
        assert d_units[k].cpu().numpy()[:int(sm["units_bytes"])].tobytes() == ro.periodic_units_host(host_ring, recorders, directory, room, cols=cols).tobytes()
        periodic_written += len(pgot.written())
    print("levels written: %d event images, %d periodic images; %d of %d pixels differ from the twin's"
          % (events_written, periodic_written, tally.differing, tally.pixels))
    assert events_written >= 1 and periodic_written >= 3 and tally.share() < SHARE


def chain_input(ro):
    """the chain test's samples and shape: noise, a weak tone in the first window, two bursts in the second"""
    bins, overlap, total = 256, 192, 200
    hop = bins - overlap
    iq = noise_iq(np.random.default_rng(41), bins + hop * (total - 1), sigma=0.05)
    add_chirp(iq, 0, len(iq) / 48000.0, -13500.0, 0.0, 0.2)                    # -13500 Hz is column 56: image column 16
    for a, b in ((30, 33), (100, 104)):
        add_chirp(iq, a * hop + 96, ((b - a) * hop + 64) / 48000.0, 6000.0, 0.0, 5.0)     # 6000 Hz is column 160: image column 40
    windows = [(40, 30), (150, 21)]
    primary = ro.Bands(low_noise=20, noise_width=32, low_detect=155, detect_width=10, avg_bins=5)
    return iq, windows, 51, primary, (6, 2), 20
