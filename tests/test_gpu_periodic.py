"""GPU checks of the periodic snapshots' data units on the device (csrc/ro_periodic.hip): one launch from the ring's slots to
the big-endian, padded units of every snapshot ro_periodic_plan lists as WRITTEN -- against the host twin
(ro_periodic_units_host) byte for byte in the units in use, with guard bytes behind d_units and the ring checked unwritten;
every case runs twice.  The rings are synthetic (tests/periodiclib.py): a ring float names its (row, column), so a wrong float
names itself.  The decision table holds the four rooms (exactly needed_bytes, one block less, no multiple of 2880, none with
d_units NULL), LOST at ring_rows = S + 1 and captured at S + 2, a capacity below the due count, `final` with 1 and with S
rows, the ring's wrap, eight recorders in one launch and the bit copy.  Only the chain test runs a transform.  Nothing here
has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from periodiclib import (BLOCK, EMU, GUARD, NGUARD, PAD, TABLE, WRITTEN, Case, Result, blocks_of, case_from_emu, check_cuts, guarded,
                         host_units, plan_call, statuses, unit_refusals)
from test_gpu_units import SHAPES
from test_periodic_cpu import GPU_SEED
from util import add_tone, noise_iq

pytestmark = pytest.mark.gpu


@pytest.fixture()
def st(ro, torch_cuda):
    with ro.Stft(bins=256, overlap=0) as handle:
        yield handle


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def device_units(ro, torch, st, case, directory):
    """the resident call on the current stream over an upload of the case's ring; returns d_units with its guards.  The ring
    must come back unwritten"""
    d_ring = up(torch, case.ring)
    d_units = up(torch, guarded(case.units_bytes, NGUARD * 64))
    ring = case.ring_struct(ro, d_ring.data_ptr())
    st.periodic_units_resident(ring, case.recorders, directory, d_units if case.units_bytes else None, case.units_bytes,
                               stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_ring.cpu().numpy().tobytes() == case.ring.tobytes(), "the ring was written"
    return d_units.cpu().numpy()


def device_vs_host(ro, torch, st):
    def call(case):
        directory, summary, nxt = plan_call(ro, case)
        got = Result(case, directory, summary, nxt, device_units(ro, torch, st, case, directory))
        want = Result(case, directory, summary, nxt, host_units(ro, case, directory))
        assert got.raw.tobytes() == want.raw.tobytes(), (case.recorders, got.dir)
        assert device_units(ro, torch, st, case, directory).tobytes() == got.raw.tobytes(), "two runs differ"
        return got
    return call


# ---- 1. the decision table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_on_the_device(ro, torch_cuda, st, case_fn):
    case_fn(ro, device_vs_host(ro, torch_cuda, st))


def test_random_emulator_cases_on_the_device(ro, torch_cuda, st):
    rng = np.random.default_rng(GPU_SEED)
    call = device_vs_host(ro, torch_cuda, st)
    written = 0
    for _ in range(16):
        written += int(call(case_from_emu(EMU.random_case(rng))).summary["written"])
    assert written > 0


# ---- 2. shapes around the block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["the whole row", "an odd first column", "the last columns of 1365"])
def test_units_around_the_block(ro, torch_cuda, st, place):
    """units that end just in front of, at and just behind a block's end, as the whole ring row, from column 1 of a ring with
    stride = cols + 3, and as the last columns of a 1365-column row; two snapshots per call, so that the second unit starts
    behind the first one's padding"""
    call = device_vs_host(ro, torch_cuda, st)
    for naxis1, S in SHAPES:
        cols, first, stride = {"the whole row": (naxis1, 0, naxis1), "an odd first column": (naxis1 + 1, 1, naxis1 + 4)}.get(
            place, (1365, 1365 - naxis1, 1365))
        case = Case([(S, first, naxis1)], 2 * S + 2, 2 * S + 3, cols, 2 * BLOCK * blocks_of(naxis1, S), stride=stride)
        r = call(case)
        assert statuses(r) == [WRITTEN, WRITTEN] and r.dir["naxis1"].tolist() == [naxis1] * 2, (naxis1, S, r.dir)
        assert r.dir["offset"].tolist() == [0, BLOCK * blocks_of(naxis1, S)]
        check_cuts(case, r)


# ---- 3. row indices beyond 2^31 and 2^33 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [(1 << 31) + 5, (1 << 33) + 5], ids=["2^31", "2^33"])
def test_row_indices_beyond_int32(ro, torch_cuda, st, base):
    """next_index x S just behind 2^31 + 5 and 2^33 + 5 in a 23-slot ring: two full snapshots and a final one of 2 rows, their
    slots from int64 rows; the ring's floats count the rows from H - 23"""
    S = 7
    k = -(-base // S)
    while (k * S) % 23 + 2 * S + 2 <= 23:                            # (the three snapshots shall cross the ring's last slot)
        k += 1
    H = (k + 2) * S + 2
    case = Case([(S, 1, 9), (S, 0, 12)], H, 23, 12, 8 * BLOCK, final=True, next_index=[k, k + 1], stride=15, row_base=H - 23)
    r = device_vs_host(ro, torch_cuda, st)(case)
    assert r.shape() == [(0, k, k * S, S, (k + 1) * S + 1, WRITTEN), (0, k + 1, (k + 1) * S, S, (k + 2) * S + 1, WRITTEN),
                         (0, k + 2, (k + 2) * S, 2, H - 1, WRITTEN), (1, k + 1, (k + 1) * S, S, (k + 2) * S + 1, WRITTEN),
                         (1, k + 2, (k + 2) * S, 2, H - 1, WRITTEN)]
    assert base <= k * S < base + 23 * S
    check_cuts(case, r)


# ---- 4. the chain, nothing waited for in between -------------------------------------------------------------------------------
def test_samples_to_periodic_units_in_three_chunks(ro, torch_cuda):
    """256 bins, overlap 192, 200 rows of noise and a tone in chunks of 61, 90 and 49 rows: run_resident_windows ->
    ring_put_resident -> periodic_units_resident per chunk on one stream, nothing waited for; the plans are host arithmetic.
    Two recorders (S = 7 and 5) keep different columns of a 51-column image in a ring of 128 slots with stride 54.  Each
    chunk's units equal the twin's over the downloaded image, and the older route's: the same rows packed by hand, a
    directory built by hand, then snapshot_units_resident"""
    torch = torch_cuda
    bins, overlap, total = 256, 192, 200
    hop = bins - overlap
    chunks = [(0, 61), (61, 90), (151, 49)]
    iq = add_tone(noise_iq(np.random.default_rng(41), bins + hop * (total - 1), sigma=0.05), 6000.0, 0.5)
    windows = [(40, 30), (150, 21)]
    cols, stride, ring_rows = 51, 54, 128
    recorders = [(7, 0, 30), (5, 31, 20)]
    room = 40 * BLOCK
    s = stream_of(torch)
    d_iq = [torch.from_numpy(iq[a * hop:a * hop + (n - 1) * hop + bins].copy()).cuda() for a, n in chunks]
    nxt = np.zeros(2, np.int64)
    plans = []
    with ro.Stft(bins=bins, overlap=overlap) as st:
        d_rows = torch.zeros((90, bins), dtype=torch.float32, device="cuda")
        d_image = [torch.zeros((n, cols), dtype=torch.float32, device="cuda") for _, n in chunks]
        d_ring = torch.full((ring_rows * stride,), PAD, dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_units = [up(torch, guarded(room, NGUARD * 64)) for _ in chunks]
        torch.cuda.synchronize()
        for k, (first, n) in enumerate(chunks):              # ---- nothing below waits for the device
            st.run_resident_windows(d_iq[k], ro.RO_IQ_F32, (n - 1) * hop + bins, 0, n, d_rows, windows, d_image[k], stream=s)
            st.ring_put_resident(d_image[k], first, n, ring, stream=s)
            directory, sm = ro.periodic_plan(recorders, nxt, first + n, k == len(chunks) - 1, ring_rows, cols, room, 64)
            st.periodic_units_resident(ring, recorders, directory, d_units[k], room, stream=s)
            plans.append((directory, sm))
        torch.cuda.synchronize()
        image = np.concatenate([d.cpu().numpy() for d in d_image])
        assert image.shape == (total, cols) and np.isfinite(image).all() and image.max() > 10 * np.median(image)
        written, seen, short = 0, set(), 0
        for k, (first, n) in enumerate(chunks):
            directory, sm = plans[k]
            head = first + n
            assert directory["status"].tolist() == [WRITTEN] * len(directory) and int(sm["unlisted"]) == 0
            host_ring = np.full((ring_rows, stride), PAD, np.float32)
            for r in range(max(head - ring_rows, 0), head):
                host_ring[r % ring_rows, :cols] = image[r]
            want = ro.periodic_units_host(host_ring, recorders, directory, room, cols=cols)
            got = d_units[k].cpu().numpy()
            used = int(sm["units_bytes"])
            assert len(want) == used and got[:used].tobytes() == want.tobytes() and np.all(got[used:] == GUARD), k
            # the older route: the same rows packed by hand, a hand-built directory, snapshot_units_resident
            snap = np.zeros(len(directory), ro.capi.SNAPSHOT_DTYPE)
            arena, offset = [], 0
            for i, e in enumerate(directory):
                a, b = int(e["first_row"]), int(e["first_row"]) + int(e["rows"])
                snap[i]["first_row"], snap[i]["rows"], snap[i]["slot"], snap[i]["offset"] = a, b - a, int(e["recorder"]), offset
                arena.append(image[a:b].reshape(-1))
                offset += (b - a) * cols
                seen.add(int(e["recorder"]))
                short += int(e["rows"]) < recorders[int(e["recorder"])][0]
            snap_sm = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
            snap_sm["resolved"] = len(directory)
            d_old = [up(torch, guarded(len(directory) * 32, 64)), up(torch, guarded(room, NGUARD * 64)), up(torch, guarded(64, 64))]
            st.snapshot_units_resident(up(torch, snap), len(directory), up(torch, snap_sm), up(torch, np.concatenate(arena)), offset,
                                       cols, [(f, c) for _, f, c in recorders], d_old[0], d_old[1], room, d_old[2], stream=s)
            torch.cuda.synchronize()
            old_sm = d_old[2].cpu().numpy()[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
            assert int(old_sm["written"]) == len(directory) and int(old_sm["units_bytes"]) == used
            assert d_old[1].cpu().numpy()[:used].tobytes() == want.tobytes(), k
            old_dir = d_old[0].cpu().numpy()[:len(directory) * 32].view(ro.capi.FITS_UNIT_DTYPE)
            assert old_dir["offset"].tolist() == directory["offset"].tolist() and old_dir["bytes"].tolist() == directory["bytes"].tolist()
            written += len(directory)
        ring_now = d_ring.cpu().numpy().reshape(ring_rows, stride)
        assert ring_now.tobytes() == host_ring.tobytes(), "the ring is what ring_put_resident left"
    print("periodic units written: %d in %s; short final ones %d" % (written, [len(p[0]) for p in plans], short))
    assert written == 29 + 40 and seen == {0, 1} and short == 1 and nxt.tolist() == [29, 40]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_handle(ro, torch_cuda, st):
    torch = torch_cuda
    lib = ro.library()
    case = Case([(4, 1, 6), (3, 0, 2)], 11, 12, 10, 5 * BLOCK)
    directory, _, _ = plan_call(ro, case)
    assert directory["status"].tolist() == [WRITTEN] * 5
    d_ring = up(torch, case.ring)
    before = guarded(5 * BLOCK, 64)
    d_units = up(torch, before)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(**kw):
        a = dict(ring_rows_ptr=d_ring.data_ptr(), recorders=True, count=2, dir=True, entries=5, units=d_units.data_ptr(),
                 units_bytes=5 * BLOCK)
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
        if a["units"] == "ring":
            a["units"] = d_ring.data_ptr() + 4 * 120 - 16                             # inside the ring, aligned
        elif a["units"] == "ring end":
            a["units"] = d_ring.data_ptr() - 5 * BLOCK + 16                           # its last 16 bytes are the ring's first
        return lib.ro_stft_periodic_units_resident(st._h, None if "ring" in kw and kw["ring"] is None else C.byref(desc),
                                                   p(recs) if a["recorders"] else None, a["count"], p(d) if a["dir"] else None,
                                                   a["entries"], a["units"], a["units_bytes"], stream_of(torch))
    for kw, word in unit_refusals("d_") + [(dict(units=d_units.data_ptr() + 8), "d_units is not aligned")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_stft_periodic_units_resident:"), (kw, text)
    torch.cuda.synchronize()
    assert d_units.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"
    assert call(dir=None, entries=0) == 0 and call(units=None, units_bytes=0, entries=0) == 0
    torch.cuda.synchronize()
    assert d_units.cpu().numpy().tobytes() == before.tobytes()
    assert call() == 0
    torch.cuda.synchronize()
    got = d_units.cpu().numpy()
    assert got.tobytes() == host_units(ro, case, directory)[:len(got)].tobytes()
