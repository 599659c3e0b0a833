"""CPU checks of the resized previews (csrc/ro_resize.cpp): fits2png's --width.  Three links, each exact: resizelib's
restatement equals Pillow's resize(..., Image.LANCZOS) byte for byte on every shape and content; ro_resize_shape equals
fits2png's int(height * ratio); and the host twin -- ro_resize_plan, then ro_levels_resize_host -- equals the restatement on the
same table, on the decision table and through to the .png files, which Pillow opens.  tests/test_gpu_resize.py holds the
device call to the twin."""
import ctypes as C
import io
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import pnglib as G
import resizelib as R
from resizelib import CONTENTS, LBLOCK, SHAPES, TABLE, WRITTEN, shape_id


def pillow(px, width):
    h, w = px.shape
    w2, h2 = R.out_shape(w, h, width)
    return np.asarray(Image.fromarray(px).resize((w2, h2), Image.LANCZOS)) if (w2, h2) != (w, h) else px


# ---- the restatement against Pillow ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_restatement_is_pillows_resize(shape, content):
    px, got = R.reference(content, shape)
    want = pillow(px, shape[2])
    assert got.shape == want.shape
    assert np.array_equal(got, want), "%d pixels differ from Pillow's" % int((got != want).sum())


# ---- the shape rule ----------------------------------------------------------------------------------------------------------------
def test_shape_rule_is_fits2pngs(ro):
    rng = np.random.default_rng(11)
    cases = [(9, 2, 4), (2, 2, 1), (5120, 1757, 1024), (615, 352, 200), (7, 1, 6), (1 << 30, 3, 1), (3, 1 << 40, 2), (10, 10, 10),
             (10, 10, 11), (10, 10, 1 << 30), (1, 1, 1), (49, 49, 7), (3, 3, 1), (1000, 999, 999)]
    cases += [tuple(int(v) for v in rng.integers(1, 3000, 3)) for _ in range(2000)]
    cases += [(int(w), 1 + i % 3, 1 + i % 5) for i, w in enumerate(rng.integers(20, 3000, 50))]           # H' = 0
    zero = same = 0
    for w, h, width in cases:
        want = (width, int(float(h) * (float(width) / float(w)))) if width < w else (w, h)
        assert ro.resize_shape(w, h, width) == want == R.out_shape(w, h, width), (w, h, width)
        zero += want[1] == 0
        same += want == (w, h)
    assert zero >= 10 and same >= 100
    for bad in ((0, 5, 3), (5, 0, 3), (5, 5, 0), (5, 5, -1), (-2, 5, 3)):
        with pytest.raises(ro.StftError) as e:
            ro.resize_shape(*bad)
        assert e.value.code == -1 and "ro_resize_shape" in str(e.value)
    lib = ro.library()
    w, h = C.c_int32(), C.c_int64()
    assert lib.ro_resize_shape(5, 5, 3, None, C.byref(h)) == -1 and "out_naxis1" in lib.ro_last_error().decode()
    assert lib.ro_resize_shape(5, 5, 3, C.byref(w), None) == -1 and "out_naxis2" in lib.ro_last_error().decode()


# ---- the host twin against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_host_twin_is_the_restatement(ro, shape, content):
    case, want = R.shape_case(ro, shape, content)
    r = R.host_call(ro, case)
    assert R.statuses(r) == [WRITTEN, WRITTEN] and r.image(1).shape == want[1].shape
    R.check_images(case, r, want)
    assert np.array_equal(r.image(0), R.source_pixels(case, 0))                     # the one-pixel image is a copy
    short = R.host_call(ro, case.with_room(case.out_bytes - 1))
    assert R.statuses(short) == [WRITTEN, R.NO_ROOM] and short.dir["naxis1"].tolist()[1] == want[1].shape[1]


@pytest.mark.parametrize("width", [1, 100, 256])
def test_all_shapes_in_one_call(ro, width):
    """all shapes under one width -- the long one, whose pixels' spans pass any tile, at its own width 256: several jobs share
    the two passes, the work items are numbered across jobs, a table serves several jobs"""
    shapes = R.one_call_shapes(width)
    r = R.host_vs_python(ro)(R.all_shapes_case(ro, shapes, width))
    want = [WRITTEN if R.out_shape(w, h, width)[1] else R.SKIPPED for w, h, _ in shapes]
    assert R.statuses(r) == want and WRITTEN in want and (width != 256 or R.LONG in shapes)


# ---- the decision table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table(ro, case_fn):
    case_fn(ro, R.host_vs_python(ro))


def test_the_plan_does_not_depend_on_the_pixels_and_tables_are_shared(ro):
    """two images of one shape share both tables; a square image's two axes share one"""
    one, _ = G.images(ro, [R.small(1, 40, 30)])
    two, levels = G.images(ro, [R.small(1, 40, 30), R.small(2, 40, 30)])
    a = R.Plan(ro, R.Case(ro, one, levels, 20, 4 * LBLOCK))
    b = R.Plan(ro, R.Case(ro, two, levels, 20, 4 * LBLOCK))
    assert int(b.info["plan_bytes"][0]) - int(a.info["plan_bytes"][0]) == 80        # one more job, no more taps
    square, levels = G.images(ro, [R.small(3, 40, 40)])
    sq = R.Plan(ro, R.Case(ro, square, levels, 20, 4 * LBLOCK))
    wide, levels = G.images(ro, [R.small(3, 40, 30)])
    assert int(sq.info["plan_bytes"][0]) < int(R.Plan(ro, R.Case(ro, wide, levels, 20, 4 * LBLOCK)).info["plan_bytes"][0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_plan_refusals(ro):
    lib = ro.library()
    d, levels = G.images(ro, [R.small(1, 30, 10)])
    summary = np.zeros(1, ro.capi.UNIT_SUMMARY_DTYPE)
    summary["entries"] = 1
    out_dir, out, info = np.zeros(1, ro.capi.FITS_UNIT_DTYPE), np.zeros(1, ro.capi.UNIT_SUMMARY_DTYPE), np.zeros(1, ro.capi.RESIZE_INFO_DTYPE)
    plan = np.zeros(1 << 12, np.uint64).view(np.uint8)
    p = lambda a: a.ctypes.data

    def call(**kw):
        a = dict(level_dir=p(d), dcap=1, summary=p(summary), levels_bytes=levels.size, width=10, out_dir=p(out_dir), out_bytes=LBLOCK,
                 out=p(out), plan=p(plan), plan_bytes=plan.size, info=p(info))
        a.update(kw)
        if a["plan"] == "odd":
            a["plan"] = p(plan) + 4
        return lib.ro_resize_plan(a["level_dir"], a["dcap"], a["summary"], a["levels_bytes"], a["width"], a["out_dir"], a["out_bytes"],
                                  a["out"], a["plan"], a["plan_bytes"], a["info"])
    for kw, word in R.plan_refusals():
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_resize_plan:"), (kw, text)
    assert call() == 0 and int(info["jobs"][0]) == 1 and 64 < int(info["plan_bytes"][0]) <= plan.size
    # a plan too small is refused with what it takes
    assert call(plan_bytes=int(info["plan_bytes"][0]) - 16) == -1 and str(int(info["plan_bytes"][0])) in lib.ro_last_error().decode()


def test_resize_refusals(ro):
    lib = ro.library()
    d, levels = G.images(ro, [R.small(1, 30, 10)])
    case = R.Case(ro, d, levels, 10, LBLOCK)
    plan = R.Plan(ro, case)
    blob = np.concatenate([plan.blob, np.zeros(2 * LBLOCK, np.uint8)])
    both = np.zeros(3 * LBLOCK, np.uint8)                    # the levels, then the out levels
    both[:LBLOCK] = levels
    p = lambda a: a.ctypes.data

    def call(**kw):
        a = dict(info=p(plan.info), plan=p(blob), levels=p(both), levels_bytes=LBLOCK, out=p(both) + LBLOCK, out_bytes=LBLOCK)
        a.update(kw)
        info = plan.info.copy()
        if a["info"] == "negative":
            info["mid_bytes"] = -1
            a["info"] = p(info)
        if a["out"] == "levels":
            a["out"] = p(both) + LBLOCK - 1
        elif a["out"] == "levels end":
            a["out"] = p(both) - LBLOCK + 1
        elif a["out"] == "plan":
            a["out"] = p(blob) + plan.blob.size - 1
        return lib.ro_levels_resize_host(a["info"], a["plan"], a["levels"], a["levels_bytes"], a["out"], a["out_bytes"])
    for kw, word in R.resize_refusals("") + [(dict(plan=p(blob) + 4), "aligned"), (dict(plan=p(blob) + 16), "not the plan")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_levels_resize_host:"), (kw, text)
    assert not both[LBLOCK:].any(), "a refused call wrote something"
    assert call() == 0
    assert np.array_equal(both[LBLOCK:LBLOCK + 30].reshape(3, 10), R.resize(R.source_pixels(case, 0), 10))


def test_a_plan_that_does_not_fit_the_buffers_writes_nothing(ro):
    """the plan is the caller's memory: a job is checked against the rooms of the CALL before anything of it is touched"""
    d, levels = G.images(ro, [R.small(1, 30, 10), R.small(2, 64, 64)])
    case = R.Case(ro, d, levels, 16, 2 * LBLOCK)
    plan = R.Plan(ro, case)
    lib = ro.library()
    out = G.guarded(LBLOCK, 64)                              # room for the first image only
    assert lib.ro_levels_resize_host(G.ptr(plan.info), G.ptr(plan.blob), G.ptr(levels), levels.size, G.ptr(out), LBLOCK) == 0
    assert np.all(out[LBLOCK:] == R.GUARD) and np.array_equal(out[:16 * 5].reshape(5, 16), R.resize(R.source_pixels(case, 0), 16))
    out = G.guarded(2 * LBLOCK, 64)                          # levels cut short: the second image's pixels are not all there
    assert lib.ro_levels_resize_host(G.ptr(plan.info), G.ptr(plan.blob), G.ptr(levels), levels.size - LBLOCK, G.ptr(out), 2 * LBLOCK) == 0
    assert np.all(out[LBLOCK:] == R.GUARD)


def test_a_job_of_one_pass_alone_is_left_out(ro):
    """width < W makes H' < H too, so a job of ro_resize_plan runs both passes or is a copy; a blob that says otherwise is not
    followed"""
    d, levels = G.images(ro, [R.small(1, 30, 10)])
    plan = R.Plan(ro, R.Case(ro, d, levels, 10, LBLOCK))
    lib = ro.library()
    shape = plan.blob[64 + 56:64 + 72].view(np.int32)        # w, h, w_out, h_out of job 0
    assert shape.tolist() == [30, 10, 10, 3]
    for at, value in ((3, 10), (2, 30)):                     # the horizontal pass alone; the vertical pass alone
        blob = plan.blob.copy()
        blob[64 + 56:64 + 72].view(np.int32)[at] = value
        out = G.guarded(LBLOCK, 64)
        assert lib.ro_levels_resize_host(G.ptr(plan.info), G.ptr(blob), G.ptr(levels), levels.size, G.ptr(out), LBLOCK) == 0
        assert np.all(out == R.GUARD)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stored", "deflate"])
def test_resized_levels_to_png_files(ro, kind):
    """resized levels -> the PNG twin, the plan's out directory and summary read unchanged: Pillow opens every file and its
    pixels are Pillow's resize of the source"""
    shapes = [(615, 352, 200), (410, 37, 128), (721, 9, 100), (100, 50, 3), (5000, 30, 4)]
    width = 100
    case = R.all_shapes_case(ro, shapes, width)
    r = R.host_call(ro, case)
    assert R.statuses(r) == [WRITTEN] * 4 + [R.SKIPPED]
    call = ro.levels_png_host if kind == "stored" else ro.levels_png_deflate_host
    png_dir, png, summary = call(r.dir, np.array([r.summary]), r.levels, sum(G.room_of(int(e["naxis1"]), int(e["naxis2"])) for e in r.dir[:4]))
    assert png_dir["status"].tolist() == [WRITTEN] * 4 + [R.SKIPPED] and int(summary["written"]) == 4
    for d in range(4):
        data = png[int(png_dir["offset"][d]):int(png_dir["offset"][d]) + int(png_dir["bytes"][d])].tobytes()
        want = pillow(R.source_pixels(case, d), width)
        with Image.open(io.BytesIO(data)) as im:
            assert im.mode == "L" and im.size == want.shape[::-1]
            assert np.array_equal(np.asarray(im), want), d
        if kind == "stored":
            G.walk(data, want)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_exports(ro):
    lib = ro.library()
    assert lib.ro_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", ro.capi.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (ro_[a-z0-9_]+)$", out, flags=re.M))
    for name in ("ro_resize_shape", "ro_resize_plan", "ro_stft_levels_resize_resident", "ro_levels_resize_host"):
        assert name in exported and name in ro.capi.exported_symbols(), name
    assert ro.capi.RESIZE_INFO_DTYPE.itemsize == 64
    assert lib.ro_stft_levels_resize_resident(None, None, None, None, 0, None, 0, None) == -1
    assert "null handle" in lib.ro_last_error().decode()
