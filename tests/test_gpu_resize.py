"""GPU checks of the resized previews on the device (csrc/ro_resize.hip): fits2png's --width over every level image a resize
plan has a job for.  The yardstick is the twin, ro_levels_resize_host, which tests/test_resize_cpu.py holds to resizelib's
restatement and that to Pillow: from the same plan the device call's out levels equal the twin's byte for byte -- every image,
the pad behind each, the guards, the untouched tail -- and the sources come back unwritten.  Every case runs twice with equal
bytes.  No tolerance anywhere."""
import numpy as np
import pytest

import periodiclib as P
import pnglib as G
import resizelib as R
from resizelib import CONTENTS, GUARD, LBLOCK, NGUARD, SHAPES, TABLE, WRITTEN
from test_gpu_levels import chain_input

pytestmark = pytest.mark.gpu


@pytest.fixture()
def st(ro, torch_cuda):
    with ro.Stft(bins=256, overlap=0) as handle:
        yield handle


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def device_call(ro, torch, st, case, plan):
    d_plan, d_levels = up(torch, plan.blob), up(torch, case.levels) if case.levels.size else None
    d_out = up(torch, G.guarded(case.out_bytes, NGUARD * 64))
    st.levels_resize_resident(plan.info, d_plan, d_levels, case.levels.size, d_out if case.out_bytes else None, case.out_bytes,
                              stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_plan.cpu().numpy().tobytes() == plan.blob.tobytes(), "the plan was written"
    assert d_levels is None or d_levels.cpu().numpy().tobytes() == case.levels.tobytes(), "the levels were written"
    return R.Result(ro, case, plan, d_out.cpu().numpy())


def device_checked(ro, torch, st, want=None):
    def call(case):
        plan = R.Plan(ro, case)
        got = device_call(ro, torch, st, case, plan)
        twin = R.host_call(ro, case, plan)
        for d in got.written():
            assert np.array_equal(got.image(d), twin.image(d)), "image %d differs from the twin's in %d pixels" % (
                d, int((got.image(d) != twin.image(d)).sum()))
        assert got.same_bytes(twin), "an output differs from the twin's"
        assert device_call(ro, torch, st, case, plan).same_bytes(got), "two runs differ"
        if want is not None:
            R.check_images(case, got, want)
        return got
    return call


@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_on_the_device(ro, torch_cuda, st, case_fn):
    case_fn(ro, device_checked(ro, torch_cuda, st))


# (the long shape runs once: a span longer than any tile does not depend on the content)
@pytest.mark.parametrize("shape,content", [(s, c) for s in SHAPES for c in CONTENTS if s != R.LONG or c == "random"],
                         ids=lambda v: R.shape_id(v) if isinstance(v, tuple) else v)
def test_shape_table_on_the_device(ro, torch_cuda, st, shape, content):
    case, want = R.shape_case(ro, shape, content)
    r = device_checked(ro, torch_cuda, st, want)(case)
    assert R.statuses(r) == [WRITTEN, WRITTEN] and r.image(1).shape == want[1].shape


@pytest.mark.parametrize("width", [1, 100, 256])
def test_all_shapes_in_one_call(ro, torch_cuda, st, width):
    """all shapes under one width -- the long one, whose pixels' spans pass any tile, at its own width 256: jobs of several
    images share the two launches, the work items are numbered across jobs, the tables are shared"""
    shapes = R.one_call_shapes(width)
    assert width != 256 or R.LONG in shapes
    r = device_checked(ro, torch_cuda, st)(R.all_shapes_case(ro, shapes, width))
    assert WRITTEN in R.statuses(r) and int(r.summary["no_room"]) == 0


def test_refusals_with_a_handle(ro, torch_cuda, st):
    torch = torch_cuda
    lib = ro.library()
    d, levels = G.images(ro, [R.small(1, 30, 10)])
    case = R.Case(ro, d, levels, 10, LBLOCK)
    plan = R.Plan(ro, case)
    d_plan = up(torch, np.concatenate([plan.blob, np.zeros(2 * LBLOCK, np.uint8)]))
    d_both = up(torch, np.concatenate([levels, G.guarded(LBLOCK, LBLOCK)]))       # the levels, then the out levels
    before = d_both.cpu().numpy()
    ptr = lambda t: t.data_ptr()

    def call(**kw):
        a = dict(h=st._h, info=plan.info.ctypes.data, plan=ptr(d_plan), levels=ptr(d_both), levels_bytes=LBLOCK, out=ptr(d_both) + LBLOCK,
                 out_bytes=LBLOCK)
        a.update(kw)
        info = plan.info.copy()
        if a["info"] == "negative":
            info["h_items"] = -1
            a["info"] = info.ctypes.data
        if a["out"] == "levels":
            a["out"] = ptr(d_both) + LBLOCK - 16
        elif a["out"] == "levels end":
            a["out"] = ptr(d_both) - LBLOCK + 16
        elif a["out"] == "plan":
            a["out"] = ptr(d_plan) + plan.blob.size - 16
        return lib.ro_stft_levels_resize_resident(a["h"], a["info"], a["plan"], a["levels"], a["levels_bytes"], a["out"], a["out_bytes"],
                                                  stream_of(torch))
    assert ptr(d_both) % 16 == 0 and ptr(d_plan) % 16 == 0
    more = [(dict(h=None), "handle"), (dict(plan=ptr(d_plan) + 8), "d_plan is not aligned"), (dict(levels=ptr(d_both) + 8), "d_levels is not aligned"),
            (dict(out=ptr(d_both) + LBLOCK + 8), "d_out_levels is not aligned")]
    for kw, word in R.resize_refusals("d_") + more:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_stft_levels_resize_resident:"), (kw, text)
    torch.cuda.synchronize()
    assert d_both.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    got = d_both.cpu().numpy()
    assert np.array_equal(got[LBLOCK:LBLOCK + 30].reshape(3, 10), R.resize(R.source_pixels(case, 0), 10)) and not got[LBLOCK + 30:2 * LBLOCK].any()
    assert np.all(got[2 * LBLOCK:] == GUARD)


# ---- the chain, nothing waited for in between ----------------------------------------------------------------------------------
def test_samples_to_resized_png_files(ro, torch_cuda):
    """one small chunk of the periodic chain: samples -> rows -> the ring -> the host plan -> periodic_levels_resident ->
    periodic_level_dir -> resize_plan -> one upload (the blob, the out directory, its summary) -> levels_resize_resident ->
    levels_png_resident, on one stream, nothing waited for, then one download.  Every file walks against the restatement's resize
    of the full-size level image the device left, and equals the host chain's file"""
    torch = torch_cuda
    bins, overlap, n, width = 256, 192, 90, 12
    hop = bins - overlap
    iq, windows, cols, primary, det, snap = chain_input(ro)
    stride, ring_rows, pdcap = cols + 3, 128, 64
    recorders = [(7, 0, 30), (5, 31, 20)]
    room = 40 * P.BLOCK
    levels_room, out_room, png_room = room // 4, 40 * LBLOCK, 16384
    s = stream_of(torch)
    d_iq = torch.from_numpy(iq[:(n - 1) * hop + bins].copy()).cuda()
    nxt = np.zeros(2, np.int64)
    with ro.Stft(bins=bins, overlap=overlap, bands=primary) as st:
        d_rows = torch.zeros((n, bins), dtype=torch.float32, device="cuda")
        d_image = torch.zeros((n, cols), dtype=torch.float32, device="cuda")
        d_recs = torch.zeros((n * 12,), dtype=torch.uint8, device="cuda")
        d_ring = torch.full((ring_rows * stride,), float(P.PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_levels = up(torch, G.guarded(levels_room, NGUARD * 64))
        d_ranges = torch.zeros((pdcap * 8,), dtype=torch.uint8, device="cuda")
        d_out = up(torch, G.guarded(out_room, NGUARD * 64))
        d_png = [up(torch, o) for o in (G.guarded(pdcap * 32, NGUARD * 32), G.guarded(png_room, NGUARD * 64), G.guarded(64, NGUARD * 64))]
        plan_room = 1 << 16
        d_up = torch.zeros((plan_room + pdcap * 32 + 64,), dtype=torch.uint8, device="cuda")     # the blob, the directory, the summary
        h_up = torch.zeros((plan_room + pdcap * 32 + 64,), dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        # ---- nothing below waits for the device
        st.run_resident_windows(d_iq, ro.RO_IQ_F32, (n - 1) * hop + bins, 0, n, d_rows, windows, d_image, d_records=d_recs, stream=s)
        st.ring_put_resident(d_image, 0, n, ring, stream=s)
        directory, sm = ro.periodic_plan(recorders, nxt, n, True, ring_rows, cols, room, pdcap)
        st.periodic_levels_resident(ring, recorders, directory, d_ranges, d_levels, levels_room, stream=s)
        level_dir, level_sm = ro.periodic_level_dir(directory)
        out_dir, out_sm, blob, info = ro.resize_plan(level_dir, np.array([level_sm]), levels_room, width, out_room)
        assert blob.size <= plan_room and len(out_dir) == len(level_dir) <= pdcap
        h = h_up.numpy()
        h[:blob.size] = blob
        h[plan_room:plan_room + len(out_dir) * 32] = out_dir.view(np.uint8)
        h[plan_room + pdcap * 32:] = np.array([out_sm]).view(np.uint8)
        d_up.copy_(h_up, non_blocking=True)
        st.levels_resize_resident(info, d_up, d_levels, levels_room, d_out, out_room, stream=s)
        st.levels_png_resident(d_up[plan_room:], pdcap, d_up[plan_room + pdcap * 32:], d_out, out_room, d_png[0], d_png[1], png_room,
                               d_png[2], stream=s)
        torch.cuda.synchronize()
    full = d_levels.cpu().numpy()[:levels_room]
    written = [int(d) for d in np.flatnonzero(level_dir["status"] == WRITTEN)]
    assert len(written) >= 3 and int(out_sm["written"]) == len(written) == int(info["jobs"][0]) and int(out_sm["no_room"]) == 0
    # the host chain from the same full-size levels
    resized = ro.levels_resize_host(info, blob, full, out_room)
    got_out = d_out.cpu().numpy()
    assert got_out[:out_room].tobytes()[:int(out_sm["units_bytes"])] == resized.tobytes()[:int(out_sm["units_bytes"])]
    assert np.all(got_out[int(out_sm["units_bytes"]):] == GUARD), "bytes of the out levels past the ones in use were touched"
    full_dir = np.zeros(pdcap, ro.capi.FITS_UNIT_DTYPE)
    full_dir[:len(out_dir)] = out_dir
    pcase = G.Case(ro, full_dir, resized, png_room, dcap=pdcap)
    pcase.summary = np.array([out_sm])
    pgot = G.Result(ro, pcase, *[o.cpu().numpy() for o in d_png])
    assert pgot.same_bytes(G.host_call(ro, pcase)), "the files differ from the host chain's"
    assert pgot.written() == written
    for d in written:
        e = level_dir[d]
        px = full[int(e["offset"]):int(e["offset"]) + int(e["bytes"])].reshape(int(e["naxis2"]), int(e["naxis1"]))
        want = R.resize(px, width)
        assert want.shape == (R.out_shape(px.shape[1], px.shape[0], width)[1], width)
        G.walk(pgot.file(d), want)
    print("files written: %d resized periodic snapshots of %s" % (len(written), sorted({(int(level_dir[d]["naxis1"]), int(level_dir[d]["naxis2"])) for d in written})))
