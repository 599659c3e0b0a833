"""CPU-side checks of the preview files (csrc/ro_png.hip, ro_levels_png_host, ro_periodic_level_dir, ro_png_bytes): the four
entry points exist, are declared and bound, RO_PNG_ALIGN is in the header and the ABI is still 5; ro_png_bytes against the
formula and against built files; the host twin against tests/pnglib.py's file -- built with struct and zlib, walked chunk by
chunk with zlib and opened with Pillow -- byte for byte over the shape table and the decision table, with guard bytes behind
every output; every refusal names its argument and writes nothing; ro_periodic_level_dir over periodiclib's cases; the two
chains on the host, whose decoded files are the oracle's grey images; the kernels' emitted metadata.  Every comparison is
exact."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import levelslib as L
import periodiclib as P
import pnglib as G
from pnglib import GUARD, LBLOCK, NGUARD, SHAPES, TABLE, WRITTEN, ptr
from unitslib import ROOT, SKIPPED

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_png_bytes", "ro_stft_levels_png_resident", "ro_levels_png_host", "ro_periodic_level_dir")


def test_exports_and_abi(ro, tmp_path):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    assert C.sizeof(ro.capi.Config) == 96
    assert ro.capi.RO_PNG_ALIGN == 16 == ro.RO_PNG_ALIGN and ro.capi.FITS_UNIT_DTYPE.itemsize == 32
    assert callable(ro.png_bytes) and callable(ro.levels_png_host) and callable(ro.periodic_level_dir)
    assert callable(ro.Stft.levels_png_resident)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ro_stft.h"\n'
                   'extern int64_t ro_png_bytes(int32_t, int64_t);\n'          # (compiles only next to the same declaration)
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d\\n", sizeof(ro_fits_unit_t), sizeof(ro_unit_summary_t), sizeof(ro_stft_config_t),\n'
                   '         RO_PNG_ALIGN, RO_LEVEL_BLOCK, RO_ABI_VERSION);\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 64, 96, 16, 720, 5]


def test_png_bytes(ro):
    lib = ro.library()
    for w, h in SHAPES + [(65535, 1), (65534, 1), (3, 7), (1, 32767), (1, 32768), (2, 1 << 20)]:
        assert ro.png_bytes(w, h) == G.file_bytes(w, h), (w, h)
    assert ro.png_bytes(1, 1) == 70
    for w, h in [(1, 1), (4368, 15), (255, 256), (65535, 1), (300, 3)]:
        assert ro.png_bytes(w, h) == len(G.expected_file(G.pixels_of("random", w, h)))
    # the largest IDAT: 6 + 5 nblk + R <= 2^31 - 1
    h = ((1 << 31) - 1 - 6) // 2
    while 6 + 5 * -(-2 * h // 65535) + 2 * h > (1 << 31) - 1:
        h -= 1
    assert ro.png_bytes(1, h) == G.file_bytes(1, h) and lib.ro_png_bytes(1, h + 1) == -1
    for w, h in [(0, 5), (5, 0), (-1, 5), (5, -1), (1 << 30, 2), (2, 1 << 30), (1, 1 << 62), ((1 << 31) - 1, (1 << 63) - 1)]:
        assert lib.ro_png_bytes(w, h) == -1, (w, h)
        assert lib.ro_last_error().decode().startswith("ro_png_bytes:")
        with pytest.raises(ro.StftError):
            ro.png_bytes(w, h)


# ---- the twin against the Python builder ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", G.CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shape_table_twin_against_python(ro, shape, content):
    case = G.shape_case(ro, *shape, content)
    r = G.host_vs_python(ro)(case)
    assert G.statuses(r) == [WRITTEN, WRITTEN] and len(r.file(1)) == G.file_bytes(*shape)
    short = G.host_call(ro, case.with_room(case.png_bytes - 1))
    assert G.statuses(short) == [WRITTEN, G.NO_ROOM] and short.png.tobytes() == r.png[:len(short.png)].tobytes()


@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_twin_against_python(ro, case_fn):
    case_fn(ro, G.host_vs_python(ro))


def test_the_checker_sees_a_flipped_bit():
    """the walk is not optional: it refuses a file whose IDAT CRC, Adler-32, block header or pixel is off by a bit"""
    px = G.pixels_of("random", 300, 250)
    good = G.expected_file(px)
    G.walk(good, px)
    n = len(good)
    for at in (n - 13, n - 17, 43, 44, 46, 48 + 70000, 20, 30):      # IDAT CRC, Adler-32, BFINAL, LEN, ~LEN, a pixel, IHDR, its CRC
        bad = bytearray(good)
        bad[at] ^= 0x04
        with pytest.raises(Exception):
            G.walk(bad, px)


def test_the_wrappers_return_what_the_calls_write(ro):
    d, levels = G.images(ro, [G.small(1, 5, 3), (None, SKIPPED), G.small(2, 700, 100), G.small(3, 2, 2)])
    case = G.Case(ro, d, levels, G.room_of(5, 3) + G.room_of(700, 100) + 3)
    want = G.host_call(ro, case)
    png_dir, png, sm = ro.levels_png_host(d, case.summary, levels, case.png_bytes)
    assert png_dir.tobytes() == want.dir.tobytes() and png.tobytes() == want.png.tobytes() and sm.tobytes() == want.summary.tobytes()
    assert png_dir["status"].tolist() == [0, 1, 0, 2] and int(sm["needed_bytes"]) == int(sm["units_bytes"]) + G.room_of(2, 2)
    with pytest.raises(ro.StftError) as e:
        ro.levels_png_host(d, case.summary, levels, -1)
    assert e.value.code == -1 and "png_bytes" in str(e.value)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_twin(ro):
    lib = ro.library()
    d, levels = G.images(ro, [G.small(1, 6, 10)])
    room = G.room_of(6, 10)
    case = G.Case(ro, d, np.concatenate([levels, np.zeros(room, np.uint8)]), room)      # (room behind the levels for files that touch them)
    src = case.levels
    outs = G.outputs_for(case)
    before = [o.copy() for o in outs]
    src_before = src.copy()

    def call(**kw):
        a = dict(level_dir=ptr(d), dcap=1, summary=ptr(case.summary), levels=ptr(src), levels_bytes=LBLOCK, png_dir=ptr(outs[0]),
                 png=ptr(outs[1]), png_bytes=room, out=ptr(outs[2]))
        a.update(kw)
        if a["png"] == "levels":
            a["png"] = C.c_void_p(src.ctypes.data + LBLOCK - 1)                       # its first byte is the levels' last
        elif a["png"] == "levels end":
            a["png"] = C.c_void_p(src.ctypes.data - room + 1)                         # its last byte is the levels' first
        return lib.ro_levels_png_host(a["level_dir"], a["dcap"], a["summary"], a["levels"], a["levels_bytes"], a["png_dir"], a["png"],
                                      a["png_bytes"], a["out"])
    for kw, word in G.refusals(""):
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_levels_png_host:"), (kw, text)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), "a refused call wrote something"
        assert src.tobytes() == src_before.tobytes()
    assert call(level_dir=None, dcap=0) == 0 and call(levels=None, levels_bytes=0) == 0 and call(png=None, png_bytes=0) == 0
    assert call(png=C.c_void_p(src.ctypes.data + LBLOCK)) == 0 and src[:LBLOCK].tobytes() == src_before[:LBLOCK].tobytes()
    assert call() == 0 and outs[2][:64].view(ro.capi.UNIT_SUMMARY_DTYPE)["written"][0] == 1


def test_refusal_of_the_resident_call_without_a_handle(ro):
    lib = ro.library()
    one = C.c_void_p(16)
    assert lib.ro_stft_levels_png_resident(None, one, 4, one, one, 720, one, one, 4096, one, None) == -1
    assert b"ro_stft_levels_png_resident: null handle" in lib.ro_last_error()


# ---- a periodic plan's directory in level form ---------------------------------------------------------------------------------
def check_level_dir(ro, directory, summary):
    lib = ro.library()
    n = len(directory)
    out, sm = G.guarded(n * 32, NGUARD * 32), G.guarded(64, NGUARD * 64)
    src = directory.copy()
    assert lib.ro_periodic_level_dir(ptr(src) if n else None, n, ptr(out), ptr(sm)) == 0, lib.ro_last_error()
    assert src.tobytes() == directory.tobytes() and np.all(out[n * 32:] == GUARD) and np.all(sm[64:] == GUARD)
    level_dir, s = out[:n * 32].view(ro.capi.FITS_UNIT_DTYPE), sm[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
    for e, lv in zip(directory, level_dir):
        if e["status"] == P.WRITTEN:
            assert (int(lv["offset"]), int(lv["bytes"]), int(lv["naxis2"]), int(lv["naxis1"]), int(lv["status"])) == \
                (int(e["offset"]) // 4, int(e["naxis1"]) * int(e["rows"]), int(e["rows"]), int(e["naxis1"]), WRITTEN)
        else:
            assert lv.tobytes() == bytes(28) + bytes([SKIPPED, 0, 0, 0])
    written = int((directory["status"] == P.WRITTEN).sum())
    assert [int(s[k]) for k in ("entries", "written", "skipped", "no_room", "invalid", "reserved")] == [n, written, n - written, 0, 0, 0]
    assert int(s["units_bytes"]) == int(s["needed_bytes"]) == int(summary["units_bytes"]) // 4
    wrapped, wsm = ro.periodic_level_dir(directory)
    assert wrapped.tobytes() == level_dir.tobytes() and wsm.tobytes() == s.tobytes()
    return level_dir, s


@pytest.mark.parametrize("case_fn", P.TABLE, ids=lambda f: f.__name__)
def test_periodic_level_dir_over_the_plans_cases(ro, case_fn):
    seen = []

    def call(case):
        got = P.host_call(ro, case)
        check_level_dir(ro, got.dir, got.summary)
        seen.append(len(got.dir))
        return got
    case_fn(ro, call)
    assert seen


def test_refusals_of_periodic_level_dir(ro):
    lib = ro.library()
    case = P.Case([(4, 1, 6), (3, 0, 2)], 11, 12, 10, 5 * P.BLOCK)
    directory, _, _ = P.plan_call(ro, case)
    out, sm = G.guarded(5 * 32, 64), G.guarded(64, 64)
    bad = directory.copy()
    bad["status"][3] = 3
    for args, word in (((ptr(directory), -1, ptr(out), ptr(sm)), "entries"), ((None, 5, ptr(out), ptr(sm)), "null dir"),
                       ((ptr(directory), 5, None, ptr(sm)), "null level_dir"), ((ptr(directory), 5, ptr(out), None), "null level_summary"),
                       ((ptr(bad), 5, ptr(out), ptr(sm)), "dir[3].status")):
        assert lib.ro_periodic_level_dir(*args) == -1, word
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_periodic_level_dir:"), text
        assert np.all(out == GUARD) and np.all(sm == GUARD), "a refused call wrote something"
    assert lib.ro_periodic_level_dir(None, 0, None, ptr(sm)) == 0 and sm[:64].tobytes() == bytes(64)


# ---- the chains on the host -----------------------------------------------------------------------------------------------------
def decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(bytes(data))) as im:
        return np.asarray(im).copy()


@pytest.mark.parametrize("case_fn", L.TABLE, ids=lambda f: f.__name__)
def test_chain_of_the_event_snapshots_on_the_host(ro, oracle, case_fn):
    """ro_snapshot_levels_host -> ro_levels_png_host: every decoded file is the oracle's grey image of the cut"""
    files = []

    def call(case):
        r = L.host_call(ro, case)
        pcase = G.Case(ro, r.dir, r.levels, int(r.summary["units_bytes"]) * 2 + 128 * len(r.dir), entries=int(r.summary["entries"]))
        pcase.summary = np.array([r.summary])
        png = G.host_vs_python(ro)(pcase)
        assert G.statuses(png) == [WRITTEN if s == WRITTEN else SKIPPED for s in L.statuses(r)]
        for d in png.written():
            _, u8, _ = oracle.ln_levels(L.source_image(case, d))
            assert np.array_equal(decode(png.file(d)), u8), d
            files.append(d)
        return r
    case_fn(ro, call)
    assert files


@pytest.mark.parametrize("case_fn", L.PERIODIC_TABLE, ids=lambda f: f.__name__)
def test_chain_of_the_periodic_snapshots_on_the_host(ro, oracle, case_fn):
    """ro_periodic_levels_host -> ro_periodic_level_dir -> ro_levels_png_host, the same"""
    files = []

    def call(case):
        directory, summary, _ = P.plan_call(ro, case)
        r = L.periodic_host_call(ro, case, directory)
        level_dir, sm = check_level_dir(ro, directory, summary)
        assert int(sm["units_bytes"]) == len(r.levels)
        pcase = G.Case(ro, level_dir.copy(), r.levels, len(r.levels) * 2 + 128 * len(directory))
        pcase.summary = np.array([sm])
        png = G.host_vs_python(ro)(pcase)
        assert G.statuses(png) == [WRITTEN if s == P.WRITTEN else SKIPPED for s in directory["status"]]
        for d in png.written():
            _, u8, _ = oracle.ln_levels(L.ring_image(case, directory[d]))
            assert np.array_equal(decode(png.file(d)), u8), d
            files.append(d)
        return r
    case_fn(ro, call)
    assert files


# ---- the kernels' metadata -------------------------------------------------------------------------------------------------------
def test_png_kernels_build_pin(tmp_path):
    """three kernels (plan, blocks, finish); none spills or uses scratch memory; no atomics; the blocks' LDS is the checksum
    tables and the waves' sums; read from the compiler's resource remarks"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_png.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_png.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = re.findall(r"Function Name: (\S+)[\s\S]*?VGPRs: (\d+)[\s\S]*?ScratchSize \[bytes/lane\]: (\d+)[\s\S]*?"
                         r"SGPRs Spill: (\d+)[\s\S]*?VGPRs Spill: (\d+)[\s\S]*?LDS Size \[bytes/block\]: (\d+)", r.stderr)
    seen = {}
    for name, vgprs, scratch, sspill, vspill, lds in remarks:
        short = re.search(r"png_(plan|blocks|finish)_kernel", name).group(0)
        print("%s: %s VGPRs, LDS %s, scratch %s, spills %s + %s" % (short, vgprs, lds, scratch, sspill, vspill))
        assert (int(scratch), int(sspill), int(vspill)) == (0, 0, 0), short
        seen[short] = (int(vgprs), int(lds))
    assert sorted(seen) == ["png_blocks_kernel", "png_finish_kernel", "png_plan_kernel"]
    assert all(v <= 128 for v, _ in seen.values()), seen
    assert seen["png_finish_kernel"][1] == 0 and seen["png_plan_kernel"][1] <= 1024 and seen["png_blocks_kernel"][1] <= 16384, seen
    isa = open(out).read()
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_", isa)
