"""CPU-side checks of the compressed preview files (csrc/ro_png_deflate.hip, ro_levels_png_deflate_host): the two entry points
exist, are declared and bound, and the ABI is still 5; the host twin against tests/pngdeflatelib.py's restatement of the stream
-- two-queue Huffman construction, the 15-bit limit, canonical codes, built with struct and zlib -- byte for byte over the shape
table times the content table and over the decision table, every file walked chunk by chunk with zlib and opened with Pillow,
with guard bytes behind every output; the limit rule seen firing; files whose blocks are all stored equal the stored call's;
every refusal names its argument and writes nothing; the kernels' emitted metadata.  Every comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pngdeflatelib as D
import pnglib as G
from pnglib import LBLOCK, SHAPES, WRITTEN, ptr
from unitslib import ROOT, SKIPPED

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_stft_levels_png_deflate_resident", "ro_levels_png_deflate_host")


def test_exports_and_abi(ro):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    assert C.sizeof(ro.capi.Config) == 96
    assert callable(ro.levels_png_deflate_host) and callable(ro.Stft.levels_png_deflate_resident)


def test_the_restatement_inflates():
    """the yardstick itself: zlib and Pillow accept the restatement's stream -- the distance code of length 0, the empty stored
    blocks between Huffman blocks -- for every shape and content; a flat image goes to about one bit per pixel"""
    for shape in SHAPES:
        for content in D.CONTENTS:
            px = D.pixels_of(content, *shape)
            data, report = D.expected_cached(px)
            D.walk(data, px)
            assert len(report) == -(-(shape[1] * (shape[0] + 1)) // G.STORED)
    flat, _ = D.expected_cached(D.pixels_of("zeros", 615, 352))
    assert len(flat) < 615 * 352 // 8 + 4 * 160 + 100


# ---- the twin against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", D.CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shape_table_twin_against_python(ro, shape, content):
    case = D.shape_case(ro, *shape, content)
    r = D.host_vs_python(ro)(case)
    assert G.statuses(r) == [WRITTEN, WRITTEN]
    px = G.source_pixels(case, 1)
    _, report = D.expected_cached(px)
    forms = [form for form, _ in report]
    fired = [f for _, f in report]
    if content == "random":
        # uniform bytes do not compress, but for the filter bytes of one-pixel scanlines
        assert all(form == ("huffman" if shape == (1, 70000) else "stored") for form in forms), forms
    if content in ("ones", "zeros") and shape != (1, 1):
        assert forms[0] == "huffman" and len(r.file(1)) < G.file_bytes(*shape) // (2 if shape[0] == 1 else 7)
    if content in ("noise", "fib") and shape != (1, 1):
        assert any(fired), "the limit to 15 bits never fired"
    if content == "mixed" and shape in ((4368, 30), (65534, 2), (615, 352)):
        assert forms[0] == "stored" and forms[-1] == "huffman"
    if all(form == "stored" for form in forms):
        # every block stored: the file is the stored call's, byte for byte
        assert r.file(1).tobytes() == G.host_call(ro, case).file(1).tobytes()
    else:
        assert len(r.file(1)) < G.file_bytes(*shape)
    # one byte short of the actual sum: the last entry has no room, the first file is the same
    need = int(r.summary["needed_bytes"])
    assert need == int(r.summary["units_bytes"]) <= case.png_bytes
    short = D.host_call(ro, case.with_room(need - 1))
    assert G.statuses(short) == [WRITTEN, G.NO_ROOM] and short.png.tobytes() == r.png[:len(short.png)].tobytes()
    assert short.dir["bytes"].tolist() == r.dir["bytes"].tolist()
    exact = D.host_call(ro, case.with_room(need))
    assert G.statuses(exact) == [WRITTEN, WRITTEN] and exact.png.tobytes() == r.png.tobytes()
    assert D.host_call(ro, case).same_bytes(r), "two runs differ"


def test_stored_and_huffman_blocks_in_both_orders(ro):
    """zeros, a block of random rows, zeros in one image: Huffman, stored, Huffman; and a stored final block behind a Huffman
    one in a second image"""
    w, h = 615, 352
    a = G.pixels_of("random", w, h, 3)
    a[:100] = 0                                            # (block 1 is the raw bytes of rows 106 ... 212)
    a[220:] = 0
    b = G.pixels_of("random", w, h, 4)
    b[:h // 2] = 0
    d, levels = G.images(ro, [a, b])
    r = D.host_vs_python(ro)(G.Case(ro, d, levels, 2 * G.room_of(w, h)))
    assert [f for f, _ in D.expected_cached(a)[1]] == ["huffman", "stored", "huffman", "huffman"]
    assert [f for f, _ in D.expected_cached(b)[1]] == ["huffman", "huffman", "stored", "stored"]
    assert G.statuses(r) == [WRITTEN, WRITTEN]


@pytest.mark.parametrize("case_fn", D.TABLE, ids=lambda f: f.__name__)
def test_decision_table_twin_against_python(ro, case_fn):
    case_fn(ro, D.host_vs_python(ro))


def test_overlapping_images_beyond_the_block_bound(ro):
    """the one clause the compressed call adds to rule 2: the blocks that are measured are bounded from the arguments, and
    entries that name the same levels over and over are INVALID from the first one on that passes the bound"""
    px = D.pixels_of("noise", 300, 250)
    d, levels = G.images(ro, [px])
    bound = len(levels) // 65535 * 2 + 1 + 9
    many = np.repeat(d, 9)
    r = D.host_vs_python(ro)(G.Case(ro, many, levels, 9 * G.room_of(300, 250)))
    per = -(-250 * 301 // 65535)
    fit = bound // per
    assert 0 < fit < 9 and G.statuses(r) == [WRITTEN] * fit + [G.INVALID] * (9 - fit)


def test_the_checker_sees_a_flipped_bit():
    """the walk is not optional: it refuses a file whose IDAT CRC, Adler-32, header bits, code bits or IHDR is off by a bit"""
    px = D.pixels_of("noise", 300, 250)
    good, report = D.expected_cached(px)
    assert report[0][0] == "huffman"
    D.walk(good, px)
    n = len(good)
    for at in (n - 13, n - 17, 43, 45, 60, 43 + 139 + 5000, n - 30, 20, 30):
        bad = bytearray(good)
        bad[at] ^= 0x04
        with pytest.raises(Exception):
            D.walk(bad, px)
    with pytest.raises(Exception):
        D.walk(G.expected_file(px) + b"\0", px)              # larger than ro_png_bytes


def test_the_wrapper_returns_what_the_call_writes(ro):
    d, levels = G.images(ro, [G.small(1, 5, 3), (None, SKIPPED), D.pixels_of("noise", 700, 100), G.small(3, 2, 2)])
    case = G.Case(ro, d, levels, G.room_of(5, 3) + G.room_of(700, 100))
    want = D.host_call(ro, case)
    png_dir, png, sm = ro.levels_png_deflate_host(d, case.summary, levels, case.png_bytes)
    assert png_dir.tobytes() == want.dir.tobytes() and png.tobytes() == want.png.tobytes() and sm.tobytes() == want.summary.tobytes()
    assert png_dir["status"].tolist() == [0, 1, 0, 0] and int(png_dir["bytes"][2]) < G.file_bytes(700, 100)
    _, _, sizing = ro.levels_png_deflate_host(d, case.summary, levels, 0)
    assert int(sizing["needed_bytes"]) == int(sm["needed_bytes"]) == int(sm["units_bytes"]) and int(sizing["no_room"]) == 3
    with pytest.raises(ro.StftError) as e:
        ro.levels_png_deflate_host(d, case.summary, levels, -1)
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
        return lib.ro_levels_png_deflate_host(a["level_dir"], a["dcap"], a["summary"], a["levels"], a["levels_bytes"], a["png_dir"],
                                              a["png"], a["png_bytes"], a["out"])
    for kw, word in G.refusals(""):
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_levels_png_deflate_host:"), (kw, text)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), "a refused call wrote something"
        assert src.tobytes() == src_before.tobytes()
    assert call(level_dir=None, dcap=0) == 0 and call(levels=None, levels_bytes=0) == 0 and call(png=None, png_bytes=0) == 0
    assert call() == 0 and outs[2][:64].view(ro.capi.UNIT_SUMMARY_DTYPE)["written"][0] == 1


def test_refusal_of_the_resident_call_without_a_handle(ro):
    lib = ro.library()
    one = C.c_void_p(16)
    assert lib.ro_stft_levels_png_deflate_resident(None, one, 4, one, one, 720, one, one, 4096, one, None) == -1
    assert b"ro_stft_levels_png_deflate_resident: null handle" in lib.ro_last_error()


# ---- the kernels' metadata -------------------------------------------------------------------------------------------------------
def test_png_deflate_kernels_build_pin(tmp_path):
    """six kernels; none uses scratch memory or spills a VGPR (the uniform values the measure and the emit hold beyond the
    scalar file go to VGPR lanes, which the remarks count as SGPR spills); no global atomics; the emit's LDS is one staged
    block and the tables, two workgroups to a CU; read from the compiler's resource remarks.  (The source has no floating
    point; the ISA has the compiler's reciprocal in its exact expansion of the 32-bit division by a scanline's length, as
    ro_png.hip's has.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc on this box"
    out = str(tmp_path / "ro_png_deflate.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_png_deflate.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = re.findall(r"Function Name: (\S+)[\s\S]*?VGPRs: (\d+)[\s\S]*?ScratchSize \[bytes/lane\]: (\d+)[\s\S]*?"
                         r"SGPRs Spill: (\d+)[\s\S]*?VGPRs Spill: (\d+)[\s\S]*?LDS Size \[bytes/block\]: (\d+)", r.stderr)
    seen = {}
    for name, vgprs, scratch, sspill, vspill, lds in remarks:
        short = re.search(r"deflate_(want|measure|sum|place|emit|finish)_kernel", name).group(0)
        print("%s: %s VGPRs, LDS %s, scratch %s, spills %s + %s" % (short, vgprs, lds, scratch, sspill, vspill))
        assert (int(scratch), int(vspill)) == (0, 0), short
        seen[short] = (int(vgprs), int(lds))
    assert sorted(seen) == ["deflate_%s_kernel" % k for k in ("emit", "finish", "measure", "place", "sum", "want")]
    assert all(v <= 128 for v, _ in seen.values()), seen
    assert seen["deflate_finish_kernel"][1] == 0 and seen["deflate_sum_kernel"][1] == 0
    assert seen["deflate_emit_kernel"][1] <= 80 * 1024 and seen["deflate_measure_kernel"][1] <= 16384, seen
    isa = open(out).read()
    assert not re.search(r"\b(global|flat|buffer)_atomic", isa)
