"""CPU-side checks of the periodic snapshots (ro_periodic_plan, ro_periodic_units_host, ro_snapshot_rows; the kernel is
csrc/ro_periodic.hip): the new symbols are exported, declared and bound and the structs have their ABI sizes and offsets in
the header and in the binding; the plan's closed form against the emulator's ROW-BY-ROW replay of update() / startWriting() /
stop() (tools/periodic/emu_periodic.py) for S in {1, 2, 7, 351} and every H in 0 ... 3 S + 5, in one call and in chunked
calls, with and without `final`; ro_snapshot_rows against the host mirror; the host twin against the emulator on the decision
table and on 200 seeded random cases, with guard bytes behind every output; every refusal names its argument and writes
nothing; the host mirror's snap files behind their headers against the plan's entries and the twin's units; the kernel's
emitted metadata.  Every comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from periodiclib import (BLOCK, EMU, GUARD, LOST, NO_ROOM, ROOT, TABLE, WRITTEN, Case, blocks_of, case_from_emu, guarded, host_call,
                         host_vs_emu, plan_call, unit_refusals)
from test_host_cpu import H, manual, read_fits  # noqa: F401  (H is the harness fixture)

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_snapshot_rows", "ro_periodic_plan", "ro_stft_periodic_units_resident", "ro_periodic_units_host")
GPU_SEED = 83                                            # tests/test_gpu_periodic.py's sixteen random cases


def test_exports_and_abi(ro, tmp_path):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("ro_periodic_t", "ro_periodic_entry_t", "ro_periodic_summary_t"):
        assert re.search(r"\}\s*%s;" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    assert C.sizeof(ro.capi.Config) == 96
    assert (ro.capi.PERIODIC_DTYPE.itemsize, ro.capi.PERIODIC_ENTRY_DTYPE.itemsize, ro.capi.PERIODIC_SUMMARY_DTYPE.itemsize) == (12, 56, 64)
    assert ro.PERIODIC_ENTRY_DTYPE is ro.capi.PERIODIC_ENTRY_DTYPE and ro.PERIODIC_SUMMARY_DTYPE is ro.capi.PERIODIC_SUMMARY_DTYPE
    assert callable(ro.periodic_plan) and callable(ro.periodic_units_host) and callable(ro.snapshot_rows)
    assert callable(ro.Stft.periodic_units_resident)
    assert (ro.RO_PERIODIC_WRITTEN, ro.RO_PERIODIC_LOST, ro.RO_PERIODIC_NO_ROOM, ro.RO_MAX_PERIODIC) == (0, 1, 2, 8)
    # the header's own sizes and offsets, through a tiny compiled probe
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    entry = ("index", "first_row", "due_row", "offset", "bytes", "rows", "naxis1", "recorder", "status")
    summary = ("entries", "written", "lost", "no_room", "unlisted", "units_bytes", "needed_bytes", "reserved")
    fields = (["sizeof(ro_periodic_t)", "sizeof(ro_periodic_entry_t)", "sizeof(ro_periodic_summary_t)", "sizeof(ro_stft_config_t)",
               "offsetof(ro_periodic_t, snapshot_rows)", "offsetof(ro_periodic_t, window)"] +
              ["offsetof(ro_periodic_entry_t, %s)" % f for f in entry] + ["offsetof(ro_periodic_summary_t, %s)" % f for f in summary] +
              ["(size_t)RO_MAX_PERIODIC", "(size_t)RO_PERIODIC_WRITTEN", "(size_t)RO_PERIODIC_LOST", "(size_t)RO_PERIODIC_NO_ROOM",
               "(size_t)RO_FITS_BLOCK", "(size_t)RO_ABI_VERSION"])
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ro_stft.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu\\n", %s);\n' % f for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [12, 56, 64, 96, 0, 4, 0, 8, 16, 24, 32, 40, 44, 48, 52, 0, 8, 16, 24, 32, 40, 48, 56,
                                     8, 0, 1, 2, 2880, 5]
    d = ro.capi.PERIODIC_ENTRY_DTYPE
    assert [d.fields[n][1] for n in entry] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert list(ro.capi.PERIODIC_SUMMARY_DTYPE.names) == list(summary)
    assert list(ro.capi.PERIODIC_DTYPE.names) == ["snapshot_rows", "first_col", "cols"]


# ---- the cadence -------------------------------------------------------------------------------------------------------------
def listed(ro, S, nxt, head, final):
    """the (first_row, rows, due_row) one plan lists; nxt moves on"""
    before = int(nxt[0])
    d, sm = ro.periodic_plan([(S, 0, 1)], nxt, head, final, 1 << 40, 1, 1 << 40, 4096)
    assert int(sm["unlisted"]) == 0 and int(sm["lost"]) == 0 and int(sm["no_room"]) == 0
    assert d["index"].tolist() == list(range(before, before + len(d))) and int(nxt[0]) == before + len(d)
    return [(int(e["first_row"]), int(e["rows"]), int(e["due_row"])) for e in d]


def cadence(ro, S, heads, final):
    """everything the plan yields over calls at `heads`, `final` with the last one"""
    nxt = np.zeros(1, np.int64)
    got = []
    for i, head in enumerate(heads):
        got += listed(ro, S, nxt, head, final and i == len(heads) - 1)
    return got


@pytest.mark.parametrize("S", [1, 2, 7, 351])
def test_closed_form_against_the_replay(ro, S):
    """every H in 0 ... 3 S + 5, with and without `final`: one call; calls in steps of 1 (one walk, looked at after every
    step; the final one asked of a copy of its state); calls in steps of S + 1; calls with every head row repeated -- each
    yields what the replay queues, each snapshot once.  In steps of 1 a snapshot is listed at H = due_row + 1, not before"""
    heads = range(3 * S + 6)
    want = {(head, final): EMU.replay(S, head, final) for head in heads for final in (False, True)}
    assert len(want[3 * S + 5, False]) == (3 * S + 3) // S and len(want[3 * S + 5, True]) == (3 * S + 3) // S + 1
    nxt, got = np.zeros(1, np.int64), []
    for head in heads:
        for final in (False, True):
            assert cadence(ro, S, [head], final) == want[head, final], (S, head, final)
            assert cadence(ro, S, list(range(0, head, S + 1)) + [head], final) == want[head, final], (S, head, final)
            repeated = [h for h in range(0, head, max(S // 2, 1)) for _ in (0, 1)] + [head, head]
            assert cadence(ro, S, repeated, final) == want[head, final], (S, head, final)
        new = listed(ro, S, nxt, head, False)
        assert all(due == head - 1 for _, _, due in new) and len(new) <= 1
        got += new
        assert got == want[head, False], (S, head)
        assert got + listed(ro, S, nxt.copy(), head, True) == want[head, True], (S, head)


def test_row_indices_beyond_2_to_the_31_and_33(ro):
    """next_index x S around 2^31 + 5 and 2^33 + 5 in a 23-slot ring: the closed form in int64"""
    S = 7
    for base in ((1 << 31) + 5, (1 << 33) + 5):
        k = -(-base // S)
        H = (k + 2) * S + 2
        d, sm = ro.periodic_plan([(S, 1, 3)], np.array([k], np.int64), H, True, 23, 5, 8 * BLOCK, 8)
        assert [(int(e["index"]), int(e["first_row"]), int(e["rows"]), int(e["due_row"]), int(e["status"])) for e in d] == \
            [(k, k * S, S, (k + 1) * S + 1, WRITTEN), (k + 1, (k + 1) * S, S, (k + 2) * S + 1, WRITTEN), (k + 2, (k + 2) * S, 2, H - 1, WRITTEN)]
        d, sm = ro.periodic_plan([(S, 1, 3)], np.array([k - 2], np.int64), H, False, 23, 5, 8 * BLOCK, 8)
        assert d["status"].tolist() == [LOST, WRITTEN, WRITTEN, WRITTEN] and k * S > base - S


REFERENCE_SHAPES = [  # (sample_rate, bins, overlap, snapshot_length) of the reference's recorders, and the scale of the mirror's rig
    (96000, 65536, 49152, 60, 64),          # Bolidozor.json
    (96000, 524288, 262144, 400, 256),      # Ionozor.json, the first backend
    (96000, 32768, 16384, 300, 64),         # Ionozor.json, the second backend
    (48000, 32768, 24576, 60, 32),          # radio-observer.json
]


@pytest.mark.parametrize("shape", REFERENCE_SHAPES, ids=lambda s: "%d-%d-%d-%d" % s[:4])
def test_snapshot_rows_is_the_mirrors(ro, H, tmp_path, shape):  # noqa: F811
    """ro_snapshot_rows at the reference configurations' shapes equals the mirror's snapshotRows_ (requestBufferSize() / 8).
    The mirror's rig holds a ring of 8 snapshotRows_ full rows, a gigabyte and more at these sizes, so it is built with the
    sample rate, the bins and the overlap all divided by the same power of two: the fft rate, rate / (bins - overlap) in
    float, is the same float, and snapshotRows_ depends on nothing else"""
    rate, bins, overlap, length, scale = shape
    assert rate % scale == 0 and ro.fft_sample_rate(rate, bins, overlap) == ro.fft_sample_rate(rate // scale, bins // scale, overlap // scale)
    m, info = manual(H, tmp_path, bins=bins // scale, overlap=overlap // scale, rate=rate // scale, snap_len=length)
    assert ro.snapshot_rows(rate, bins, overlap, length) == info[1]
    assert info[1] == int(np.ceil(np.float32(length) * np.float32(ro.fft_sample_rate(rate, bins, overlap))))
    H.ro_host_manual_destroy(m)
    assert ro.snapshot_rows(rate, bins, overlap, 0) == 1 and ro.snapshot_rows(rate, bins, overlap, -3) == 1


# ---- the rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_host_twin_against_the_emulator(ro, case_fn):
    case_fn(ro, host_vs_emu(ro))


def test_random_cases_host_twin_against_the_emulator(ro):
    rng = np.random.default_rng(2027)
    call = host_vs_emu(ro)
    seen = np.zeros(4, np.int64)
    finals = set()
    for _ in range(200):
        args = EMU.random_case(rng)
        s = call(case_from_emu(args)).summary
        seen += [int(s[k]) for k in ("written", "lost", "no_room", "unlisted")]
        finals.add(args["final"])
    assert seen.all() and finals == {True, False}, seen      # every outcome turned up


def test_the_gpu_tests_seed_writes_units():
    """the sixteen random cases of tests/test_gpu_periodic.py: the emulator says that units are written among them"""
    rng = np.random.default_rng(GPU_SEED)
    written = 0
    for _ in range(16):
        a = EMU.random_case(rng)
        written += int(EMU.plan(a["recorders"], list(a["next_index"]), a["head_row"], a["final"], a["ring"].shape[0],
                                a["units_bytes"], a["capacity"])[1]["written"])
    assert written > 0


def test_the_emulator_of_the_kernel_runs_green(capsys):
    assert EMU.main(60) == 0
    assert capsys.readouterr().out.startswith("ok: 60 cases")


def test_the_wrappers_return_what_the_calls_write(ro):
    case = Case([(4, 1, 6), (3, 0, 2)], 11, 12, 10, 5 * BLOCK, final=True)
    want = host_call(ro, case)
    nxt = np.zeros(2, np.int64)
    d, sm = ro.periodic_plan(case.recorders, nxt, 11, True, 12, 10, 5 * BLOCK, 64)
    assert d.tobytes() == want.dir.tobytes() and sm.tobytes() == want.summary.tobytes() and nxt.tolist() == want.next_index.tolist()
    assert [(int(e["recorder"]), int(e["index"]), int(e["rows"])) for e in d] == [(0, 0, 4), (0, 1, 4), (0, 2, 3), (1, 0, 3), (1, 1, 3),
                                                                              (1, 2, 3), (1, 3, 2)]
    assert d["status"].tolist() == [WRITTEN] * 5 + [NO_ROOM] * 2 and int(sm["needed_bytes"]) == 7 * BLOCK and nxt.tolist() == [3, 2]
    units = ro.periodic_units_host(case.ring, case.recorders, d, 5 * BLOCK)
    assert units.tobytes() == want.units.tobytes() and len(units) == 5 * BLOCK
    with pytest.raises(ro.StftError) as e:
        ro.periodic_plan([(0, 0, 1)], np.zeros(1, np.int64), 5, False, 8, 4, BLOCK, 4)
    assert e.value.code == -1 and "snapshot_rows" in str(e.value)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_plan(ro):
    lib = ro.library()
    recs = ro.periodic_recorders([(4, 1, 6), (3, 0, 2)])
    nxt = np.zeros(2, np.int64)
    d, sm = guarded(8 * 56, 56), guarded(64, 64)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(**kw):
        a = dict(recorders=p(recs), count=2, next_index=p(nxt), head_row=11, final=0, ring_rows=12, cols=10, units_bytes=5 * BLOCK,
                 dir=p(d), capacity=8, summary=p(sm))
        a.update(kw)
        if "recs" in a:
            other = recs.copy()
            for i, r in a.pop("recs").items():
                other[i] = r
            a["recorders"] = p(other)
            a["keep"] = other
        if "nxt" in a:
            a["keep"] = np.array(a.pop("nxt"), np.int64)
            a["next_index"] = p(a["keep"])
        return lib.ro_periodic_plan(a["recorders"], a["count"], a["next_index"], a["head_row"], a["final"], a["ring_rows"], a["cols"],
                                    a["units_bytes"], a["dir"], a["capacity"], a["summary"])
    for kw, word in [(dict(recorders=None), "null recorders"), (dict(next_index=None), "null next_index"),
                     (dict(summary=None), "null summary"), (dict(dir=None), "null dir"), (dict(count=0), "count"),
                     (dict(count=9), "count"), (dict(recs={1: (0, 0, 2)}), "recorders[1]: snapshot_rows"),
                     (dict(recs={0: (4, -1, 6)}), "recorders[0]: window"), (dict(recs={0: (4, 1, 0)}), "recorders[0]: window"),
                     (dict(recs={1: (3, 9, 2)}), "recorders[1]: window"), (dict(head_row=-1), "head_row"),
                     (dict(units_bytes=-1), "units_bytes"), (dict(capacity=-1), "capacity"), (dict(nxt=[0, -1]), "next_index[1]"),
                     (dict(nxt=[1 << 61, 0]), "next_index[0]"), (dict(ring_rows=0), "ring_rows"), (dict(cols=0), "cols")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_periodic_plan:"), (kw, text)
        assert np.all(d == GUARD) and np.all(sm == GUARD) and not nxt.any(), "a refused call wrote something"
    assert call(dir=None, capacity=0) == 0 and call(units_bytes=0) == 0 and call() == 0
    assert sm[:64].view(ro.capi.PERIODIC_SUMMARY_DTYPE)["written"][0] == 5 and nxt.tolist() == [2, 3]


def test_refusals_of_the_host_twin(ro):
    lib = ro.library()
    case = Case([(4, 1, 6), (3, 0, 2)], 11, 12, 10, 5 * BLOCK)
    directory, _, _ = plan_call(ro, case)
    assert directory["status"].tolist() == [WRITTEN] * 5
    ring = np.zeros(12 * 10 + 5 * BLOCK // 4, np.float32)      # (the ring, and room behind it for units that touch it)
    ring[:120] = case.ring.reshape(-1)
    before = ring.copy()
    units = guarded(5 * BLOCK, 64)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(**kw):
        a = dict(ring_rows_ptr=ring.ctypes.data, recorders=True, count=2, dir=True, entries=5, units=p(units), units_bytes=5 * BLOCK)
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
            a["units"] = C.c_void_p(ring.ctypes.data + 4 * 120 - 1)                   # its first byte is the ring's last
        elif a["units"] == "ring end":
            a["units"] = C.c_void_p(ring.ctypes.data - 5 * BLOCK + 1)                 # its last byte is the ring's first
        return lib.ro_periodic_units_host(None if "ring" in kw and kw["ring"] is None else C.byref(desc),
                                          p(recs) if a["recorders"] else None, a["count"], p(d) if a["dir"] else None, a["entries"],
                                          a["units"], a["units_bytes"])
    for kw, word in unit_refusals(""):
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_periodic_units_host:"), (kw, text)
        assert np.all(units == GUARD) and ring.tobytes() == before.tobytes(), "a refused call wrote something"
    # what is allowed: no directory without entries, no units without room (and nothing written); units that touch the ring
    assert call(dir=None, entries=0) == 0 and call(units=None, units_bytes=0, entries=0) == 0 and np.all(units == GUARD)
    assert call(units=C.c_void_p(ring.ctypes.data + 4 * 120)) == 0 and ring[:120].tobytes() == before[:120].tobytes()
    assert call() == 0 and np.all(units[5 * BLOCK:] == GUARD) and not np.all(units[:5 * BLOCK] == GUARD)


def test_refusal_of_the_resident_call_without_a_handle(ro):
    lib = ro.library()
    one = C.c_void_p(16)
    ring = ro.capi.RowRing(16, 4, 4, 4, 0)
    assert lib.ro_stft_periodic_units_resident(None, C.byref(ring), one, 1, one, 1, one, 2880, None) == -1
    assert b"ro_stft_periodic_units_resident: null handle" in lib.ro_last_error()


# ---- the mirror: the reference's snap files through the host mirror, against the plan and the host twin ------------------------
def test_the_host_mirrors_snap_files_are_the_plans_entries_and_the_twins_units(ro, H, oracle, tmp_path):  # noqa: F811
    """SnapshotRecorder driven as test_host_cpu.py::test_snapshot_cadence_and_fits_files drives it, over 60 rows with S = 24
    (60 mod 24 != 0), then stop(): as many snap files as the plan has entries, NAXIS1 / NAXIS2 of each header the entry's, and
    the bytes behind each header the twin's unit, padding included"""
    bins, overlap, rate, total = 4096, 2048, 48000, 60
    m, info = manual(H, tmp_path)
    S, lbin, rbin = info[1], info[2], info[3]
    assert S == ro.snapshot_rows(rate, bins, overlap, 1) == 24 and total % S != 0
    rows = np.random.default_rng(5).random((total, bins)).astype(np.float32)
    hop = bins - overlap
    for r in range(total):
        es, eu = C.c_int64(), C.c_int64()
        oracle.lib().ro_oracle_wftime_add_samples(1700000000, 0, r * hop, rate, C.byref(es), C.byref(eu))
        H.ro_host_manual_push(m, rows[r].ctypes.data_as(C.POINTER(C.c_float)), 1.0, 0, 0.5, es.value, eu.value, r)
    H.ro_host_manual_end(m)
    buf = C.create_string_buffer(8192)
    nfiles = H.ro_host_manual_files(m, buf, 8192)
    files = buf.value.decode().split()
    # the same stream through a ring of 64 slots, one plan with `final` at the end
    ring_rows = 64
    ring = np.zeros((ring_rows, bins), np.float32)
    ring[np.arange(total) % ring_rows] = rows
    recorders = [(S, lbin, rbin - lbin)]
    nxt = np.zeros(1, np.int64)
    directory, sm = ro.periodic_plan(recorders, nxt, total, True, ring_rows, bins, 1 << 20, 16)
    assert nfiles == len(files) == len(directory) == 3 and directory["status"].tolist() == [WRITTEN] * 3
    units = ro.periodic_units_host(ring, recorders, directory, 1 << 20)
    assert len(units) == int(sm["units_bytes"]) == int(sm["needed_bytes"])
    padded = 0
    for path, e in zip(files, directory):
        hdr, data, _ = read_fits(path)
        raw = open(path, "rb").read()
        unit = blocks_of(int(e["naxis1"]), int(e["rows"])) * BLOCK
        assert (int(hdr["NAXIS1"]), int(hdr["NAXIS2"])) == (int(e["naxis1"]), int(e["rows"])) == data.shape[::-1]
        assert raw[len(raw) - unit:] == units[int(e["offset"]):int(e["offset"]) + unit].tobytes(), path
        padded += int(e["bytes"]) % BLOCK != 0
        s, l = C.c_int(), C.c_int()
        assert H.ro_host_manual_snapshot(m, int(e["index"]), C.byref(s), C.byref(l)) == 0
        assert (s.value, l.value) == (int(e["first_row"]), int(e["rows"]))
    assert padded > 0 and directory["rows"].tolist() == [24, 24, 12] and directory["due_row"].tolist() == [25, 49, 59]
    H.ro_host_manual_destroy(m)


# ---- the kernel's metadata ---------------------------------------------------------------------------------------------------
def test_periodic_kernel_build_pin(tmp_path):
    """one kernel; it neither spills nor uses scratch memory or LDS, has no barrier and no atomics, and its loads and stores
    are 4 bytes wide; read from the compiler's resource remarks and the ISA"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_periodic.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_periodic.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    remarks = re.findall(r"Function Name: (\S+)[\s\S]*?VGPRs: (\d+)[\s\S]*?ScratchSize \[bytes/lane\]: (\d+)[\s\S]*?"
                         r"SGPRs Spill: (\d+)[\s\S]*?VGPRs Spill: (\d+)[\s\S]*?LDS Size \[bytes/block\]: (\d+)", r.stderr)
    assert len(remarks) == 1 and "periodic_copy_kernel" in remarks[0][0], remarks
    name, vgprs, scratch, sspill, vspill, lds = remarks[0]
    print("periodic_copy_kernel: %s VGPRs, LDS %s, scratch %s, spills %s + %s" % (vgprs, lds, scratch, sspill, vspill))
    assert (int(scratch), int(sspill), int(vspill), int(lds)) == (0, 0, 0, 0) and int(vgprs) <= 128
    isa = open(out).read()
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_|s_barrier", isa)
    assert len(re.findall(r"global_load_dword\s", isa)) >= 12 and not re.search(r"global_(load|store)_dwordx", isa)
