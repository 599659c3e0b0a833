"""CPU-side checks of the FITS data units (csrc/ro_units.hip, ro_snapshot_units_host, ro_raw_units_host): the four entry points
exist, are declared and bound, and the two structs have their ABI sizes in the header and in the binding; the host twins
against the numpy restatement of the rules (tools/units/emu_units.py) on the decision table and on 200 seeded random
directories, with guard bytes behind every output; every refusal names its argument and writes nothing; the host mirror's
blid and raws files behind their headers against the twins' units of the same event, with and without overlap; the kernels'
emitted metadata.  Every comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hostlib import BolidEvent
from test_host_cpu import H, manual, read_fits  # noqa: F401  (H is the harness fixture)
from unitslib import (BLOCK, CAPTURED, EMU, INVALID, NO_ROOM, ROOT, SKIPPED, SLOTS, TABLE, WRITTEN, Case, case_from_emu,
                      host_call, host_vs_emu, images, outputs_for, refusals, runs, whole)

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_stft_snapshot_units_resident", "ro_stft_raw_units_resident", "ro_snapshot_units_host", "ro_raw_units_host")


def test_exports_and_abi(ro, tmp_path):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("ro_fits_unit_t", "ro_unit_summary_t"):
        assert re.search(r"\}\s*%s;" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    assert C.sizeof(ro.capi.Config) == 96
    assert ro.capi.FITS_UNIT_DTYPE.itemsize == 32 and ro.capi.UNIT_SUMMARY_DTYPE.itemsize == 64 and ro.capi.RO_FITS_BLOCK == 2880
    assert ro.FITS_UNIT_DTYPE is ro.capi.FITS_UNIT_DTYPE and ro.UNIT_SUMMARY_DTYPE is ro.capi.UNIT_SUMMARY_DTYPE
    assert callable(ro.snapshot_units_host) and callable(ro.raw_units_host)
    assert callable(ro.Stft.snapshot_units_resident) and callable(ro.Stft.raw_units_resident)
    assert (ro.RO_UNIT_WRITTEN, ro.RO_UNIT_SKIPPED, ro.RO_UNIT_NO_ROOM, ro.RO_UNIT_INVALID) == (0, 1, 2, 3)
    # the header's own sizes and offsets, through a tiny compiled probe
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ro_stft.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", sizeof(ro_fits_unit_t),\n'
                   '         sizeof(ro_unit_summary_t), offsetof(ro_fits_unit_t, offset), offsetof(ro_fits_unit_t, bytes),\n'
                   '         offsetof(ro_fits_unit_t, naxis2), offsetof(ro_fits_unit_t, naxis1), offsetof(ro_fits_unit_t, status),\n'
                   '         offsetof(ro_unit_summary_t, units_bytes), offsetof(ro_unit_summary_t, needed_bytes),\n'
                   '         sizeof(ro_stft_config_t), RO_FITS_BLOCK, RO_UNIT_WRITTEN, RO_UNIT_SKIPPED, RO_UNIT_NO_ROOM,\n'
                   '         RO_UNIT_INVALID, 1 + RO_MAX_EXTRA_BANDS, RO_ABI_VERSION);\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 64, 0, 8, 16, 24, 28, 40, 48, 96, 2880, 0, 1, 2, 3, SLOTS, 5]
    d = ro.capi.FITS_UNIT_DTYPE
    assert [d.fields[n][1] for n in ("offset", "bytes", "naxis2", "naxis1", "status")] == [0, 8, 16, 24, 28]
    assert list(ro.capi.UNIT_SUMMARY_DTYPE.names) == ["entries", "written", "skipped", "no_room", "invalid", "units_bytes",
                                                      "needed_bytes", "reserved"]


# ---- the rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_host_twins_against_the_emulator(ro, case_fn):
    case_fn(ro, host_vs_emu(ro))


def test_random_directories_host_twins_against_the_emulator(ro):
    rng = np.random.default_rng(2026)
    call = host_vs_emu(ro)
    seen = np.zeros(4, np.int64)
    kinds, counts = set(), []
    for _ in range(200):
        args = EMU.random_case(rng)
        s = call(case_from_emu(ro, args)).summary
        seen += [int(s[k]) for k in ("written", "skipped", "no_room", "invalid")]
        kinds.add(args["windows"] is None)
        counts.append((args["resolved"], len(args["directory"])))
    assert seen.all(), seen                                  # every outcome turned up
    assert kinds == {True, False} and any(r > n for r, n in counts) and any(r < 0 for r, _ in counts)


def test_the_emulator_of_the_kernels_runs_green(capsys):
    assert EMU.main(60) == 0
    assert capsys.readouterr().out.startswith("ok: 60 cases")


def test_the_wrappers_return_what_the_calls_write(ro):
    cols = 11
    d, floats = images(ro, [(4, 0), (2, 1, 1), (300, 2), (3, 0)], cols)
    windows = [(1, 9), None, (0, 11)]                        # (slot 1 and the slots behind 2: not wanted)
    case = Case(ro, "image", d, floats, 3 * BLOCK, cols, [(1, 9), (0, 0), (0, 11)] + [(0, 0)] * 5)
    want = host_call(ro, case)
    unit_dir, units, sm = ro.snapshot_units_host(d, case.summary, case.arena, cols, windows, 3 * BLOCK)
    assert unit_dir.tobytes() == want.dir.tobytes() and units.tobytes() == want.units.tobytes() and sm.tobytes() == want.summary.tobytes()
    assert unit_dir["status"].tolist() == [WRITTEN, SKIPPED, NO_ROOM, NO_ROOM] and int(sm["needed_bytes"]) == 7 * BLOCK
    d, floats = runs(ro, [400, (5, 2), 3])
    case = Case(ro, "raw", d, floats, 4 * BLOCK)
    want = host_call(ro, case)
    unit_dir, units, sm = ro.raw_units_host(d, case.summary, case.arena, 4 * BLOCK)
    assert unit_dir.tobytes() == want.dir.tobytes() and units.tobytes() == want.units.tobytes() and sm.tobytes() == want.summary.tobytes()
    assert unit_dir["status"].tolist() == [WRITTEN, SKIPPED, WRITTEN] and unit_dir["offset"].tolist() == [0, 0, 2 * BLOCK]
    with pytest.raises(ro.StftError) as e:
        ro.snapshot_units_host(d.view(ro.capi.SNAPSHOT_DTYPE), case.summary, case.arena, 0, [], BLOCK)
    assert e.value.code == -1 and "cols" in str(e.value)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["images", "raw"])
def test_refusals_of_the_host_twins(ro, raw):
    lib = ro.library()
    cols = 10
    d, floats = runs(ro, [30]) if raw else images(ro, [(6, 0)], cols)
    case = Case(ro, "raw", d, floats, 2 * BLOCK) if raw else Case(ro, "image", d, floats, 2 * BLOCK, cols, whole(cols))
    outs = outputs_for(case)
    before = [o.copy() for o in outs]
    arena = case.arena.copy()
    p = lambda a: C.c_void_p(a.ctypes.data)
    who = "ro_raw_units_host" if raw else "ro_snapshot_units_host"

    def call(**kw):
        a = dict(dir=p(case.directory), dcap=1, summary=p(case.summary), arena=p(arena), arena_floats=floats, cols=cols,
                 windows=case.windows, unit_dir=p(outs[0]), units=p(outs[1]), units_bytes=2 * BLOCK, out=p(outs[2]))
        a.update(kw)
        if a["units"] == "arena":
            a["units"] = C.c_void_p(arena.ctypes.data + 4 * floats - 1)               # its first byte is the arena's last
        elif a["units"] == "arena end":
            a["units"] = C.c_void_p(arena.ctypes.data - 2 * BLOCK + 1)                # its last byte is the arena's first
        if raw:
            return lib.ro_raw_units_host(a["dir"], a["dcap"], a["summary"], a["arena"], a["arena_floats"], a["unit_dir"], a["units"],
                                         a["units_bytes"], a["out"])
        w = a["windows"]
        if isinstance(w, dict):
            w = [w.get(i, case.windows[i]) for i in range(SLOTS)]
        arr = None if w is None else (ro.capi.BandWindow * SLOTS)(*[ro.capi.BandWindow(*x) for x in w])
        return lib.ro_snapshot_units_host(a["dir"], a["dcap"], a["summary"], a["arena"], a["arena_floats"], a["cols"], arr,
                                          a["unit_dir"], a["units"], a["units_bytes"], a["out"])
    for kw, word in refusals("", raw):
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith(who + ":"), (kw, text)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), "a refused call wrote something"
    # what is allowed: no directory without entries, no arena without floats, no units without room; units that touch the arena
    assert call(dir=None, dcap=0) == 0 and call(arena=None, arena_floats=0) == 0 and call(units=None, units_bytes=0) == 0
    touching = np.zeros(floats + 2 * BLOCK // 4, np.float32)
    touching[:floats] = arena
    assert call(arena=p(touching), units=C.c_void_p(touching.ctypes.data + 4 * floats)) == 0
    assert call() == 0 and outs[2][:64].view(ro.capi.UNIT_SUMMARY_DTYPE)["written"][0] == 1


def test_refusal_of_the_resident_calls_without_a_handle(ro):
    lib = ro.library()
    one = C.c_void_p(16)
    windows = (ro.capi.BandWindow * SLOTS)()
    assert lib.ro_stft_snapshot_units_resident(None, one, 4, one, one, 100, 5, windows, one, one, 2880, one, None) == -1
    assert b"ro_stft_snapshot_units_resident: null handle" in lib.ro_last_error()
    assert lib.ro_stft_raw_units_resident(None, one, 4, one, one, 100, one, one, 2880, one, None) == -1
    assert b"ro_stft_raw_units_resident: null handle" in lib.ro_last_error()


# ---- the mirror: the reference's files through the host mirror, against the host twins ----------------------------------------
@pytest.mark.parametrize("overlap", [2048, 0])
def test_the_host_mirrors_files_behind_their_headers_are_the_twins_units(ro, H, oracle, tmp_path, overlap):  # noqa: F811
    """driven exactly as test_host_cpu.py::test_bolid_event_writes_band_snapshot_and_raw_iq drives it: the bytes of the blid
    file (the event's snapshot) behind its header are the image unit of the same event as a CAPTURED directory entry over the
    same rows, cut to the recorder's columns [leftBin, rightBin), padding included; the bytes of the raws file behind its
    header are the raw unit over the same samples; NAXIS1 / NAXIS2 of the headers are the entries'"""
    bins, rate = 4096, 48000
    hop = bins - overlap
    m, info = manual(H, tmp_path, bins=bins, overlap=overlap, snap_len=4, lo=9000.0, hi=12000.0, adv=0.1, jit=0.3)
    raw_cap = H.ro_host_manual_raw_capacity(m)
    assert raw_cap > 0
    H.ro_host_manual_set_clock(m, 1700000000 + 2 * 3600 + 17, 123456)
    fft_rate = oracle.lib().ro_oracle_fft_sample_rate(rate, bins, overlap)
    lbin = oracle.lib().ro_oracle_frequency_to_bin(bins, rate, 9000.0)
    rbin = oracle.lib().ro_oracle_frequency_to_bin(bins, rate, 12000.0)
    adv = int(0.1 * fft_rate)
    rng = np.random.default_rng(11)
    total = 80
    rows = rng.random((total, bins)).astype(np.float32)
    iq = rng.standard_normal((bins + total * hop, 2))
    detect = np.zeros(total, bool)
    detect[30:36] = True
    t0 = 1700000000
    fed = 0
    for r in range(total):
        need = bins + r * hop                                     # the samples row r ends at
        blk = np.ascontiguousarray(iq[fed:need])
        H.ro_host_manual_push_samples(m, blk.ctypes.data_as(C.POINTER(C.c_double)), len(blk))
        fed = need
        es, eu = C.c_int64(), C.c_int64()
        oracle.lib().ro_oracle_wftime_add_samples(t0, 0, r * hop, rate, C.byref(es), C.byref(eu))
        mark = (r + 1) * hop + 1 if overlap else r * hop + 1      # FFTBackend.cpp:242,251: read after the overlap memmove
        H.ro_host_manual_push(m, rows[r].ctypes.data_as(C.POINTER(C.c_float)), 1.0, 5, 3.0 if detect[r] else 1.5,
                              es.value, eu.value, mark % raw_cap)
    H.ro_host_manual_end(m)
    evs = (BolidEvent * 4)()
    assert H.ro_host_manual_events(m, evs, 4) == 1
    e = evs[0]
    buf = C.create_string_buffer(8192)
    assert H.ro_host_manual_bolid_files(m, 0, buf, 8192) == 1
    blid = buf.value.decode().split()[0]
    assert H.ro_host_manual_bolid_files(m, 1, buf, 8192) == 1
    raws = buf.value.decode().split()[0]
    assert (e.start, e.length) == (31 - adv, 2 * adv + 6)

    def behind_the_header(path):
        hdr, data, _ = read_fits(path)
        raw = open(path, "rb").read()
        unit = -(-data.size * 4 // BLOCK) * BLOCK
        return hdr, raw[len(raw) - unit:]
    # the image: the event's full rows as one CAPTURED entry of slot 2, whose recorder keeps [lbin, rbin)
    entry = np.zeros(1, ro.capi.SNAPSHOT_DTYPE)
    entry["event"]["start_row"], entry["event"]["length"] = e.start, e.length
    entry["first_row"], entry["rows"], entry["slot"], entry["status"] = e.start, e.length, 2, CAPTURED
    sm = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
    sm["resolved"] = 1
    arena = rows[e.start:e.start + e.length].reshape(-1)
    hdr, want = behind_the_header(blid)
    unit_dir, units, out = ro.snapshot_units_host(entry, sm, arena, bins, [None, None, (lbin, rbin - lbin)], len(want) + BLOCK)
    assert unit_dir["status"].tolist() == [WRITTEN] and int(out["units_bytes"]) == len(want)
    assert (int(hdr["NAXIS1"]), int(hdr["NAXIS2"])) == (int(unit_dir[0]["naxis1"]), int(unit_dir[0]["naxis2"])) == (rbin - lbin, e.length)
    assert units.tobytes() == want and int(unit_dir[0]["bytes"]) % BLOCK != 0          # (there is padding to compare)
    # the raw run: the host twin's arena of the same event, then its unit
    raw_dir, raw_arena, raw_sm = ro.raw_host(bins, overlap, rate, entry, sm, [(iq, 0, ro.RO_IQ_F64)],
                                             np.zeros(0, ro.capi.SNAPSHOT_DTYPE), np.zeros(1, np.int64), 2 * (e.rawLength + 8))
    assert raw_dir["status"].tolist() == [CAPTURED] and int(raw_dir[0]["samples"]) == e.rawLength
    hdr, want = behind_the_header(raws)
    rs = np.zeros(1, ro.capi.RAW_SUMMARY_DTYPE)
    rs[0] = raw_sm
    unit_dir, units, out = ro.raw_units_host(raw_dir, rs, raw_arena, len(want))
    assert unit_dir["status"].tolist() == [WRITTEN] and int(out["units_bytes"]) == int(out["needed_bytes"]) == len(want)
    assert (int(hdr["NAXIS1"]), int(hdr["NAXIS2"])) == (int(unit_dir[0]["naxis1"]), int(unit_dir[0]["naxis2"])) == (2, e.rawLength)
    assert units.tobytes() == want and int(unit_dir[0]["bytes"]) % BLOCK != 0
    H.ro_host_manual_destroy(m)


# ---- the kernels' metadata ---------------------------------------------------------------------------------------------------
def test_units_kernels_build_pin(tmp_path):
    """three kernels (the plan for images, the plan for raw runs, the one copy); none spills or uses scratch memory; LDS only
    in the plan kernels: the few words their four waves exchange; no atomics; read from the compiler's resource remarks"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_units.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_units.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = re.findall(r"Function Name: (\S+)[\s\S]*?VGPRs: (\d+)[\s\S]*?ScratchSize \[bytes/lane\]: (\d+)[\s\S]*?"
                         r"SGPRs Spill: (\d+)[\s\S]*?VGPRs Spill: (\d+)[\s\S]*?LDS Size \[bytes/block\]: (\d+)", r.stderr)
    seen = {}
    for name, vgprs, scratch, sspill, vspill, lds in remarks:
        short = re.search(r"units_(plan|copy)_kernel(ILi\d)?", name).group(0)
        print("%s: %s VGPRs, LDS %s, scratch %s, spills %s + %s" % (short, vgprs, lds, scratch, sspill, vspill))
        assert (int(scratch), int(sspill), int(vspill)) == (0, 0, 0), short
        seen[short] = (int(lds), int(vgprs))
    assert sorted(seen) == ["units_copy_kernel", "units_plan_kernelILi0", "units_plan_kernelILi1"], remarks
    # LDS: two int64 and four counts per wave
    assert seen["units_plan_kernelILi0"][0] == seen["units_plan_kernelILi1"][0] == 128 and seen["units_copy_kernel"][0] == 0
    assert all(v <= 128 for _, v in seen.values())
    isa = open(out).read()
    # the blocks are scanned with the DPP ladder, four 16-bit limbs, in both plan kernels
    assert len(re.findall(r"row_bcast:31", isa)) >= 8
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_", isa)
