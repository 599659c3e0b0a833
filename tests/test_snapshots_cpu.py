"""CPU-side checks of the event snapshots (csrc/ro_snapshots.hip, ro_snapshots_host): the three entry points exist, are
declared and bound, and the three structs have their ABI sizes in the header and in the binding; every refusal names its
argument; ro_snapshots_host against the numpy restatement of the rules (tools/snapshots/emu_snapshots.py) on the decision
table and on 200 seeded random cases, with guard entries behind every output; the kernels' emitted metadata.  Every
comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from snapshotslib import (CAPTURED, GUARD, ROOT, TABLE, Case, case_from_emu, header_constant, host_call, host_vs_emu,
                          load_emu, outputs_for, ring_desc)

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_stft_ring_put_resident", "ro_stft_snapshots_resident", "ro_snapshots_host")


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def test_exports_and_abi(ro, tmp_path):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("ro_row_ring_t", "ro_snapshot_t", "ro_snap_summary_t"):
        assert re.search(r"\}\s*%s;" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    assert C.sizeof(ro.capi.Config) == 96
    assert C.sizeof(ro.capi.RowRing) == 32 and ro.capi.ROW_RING is ro.capi.RowRing
    assert ro.capi.SNAPSHOT_DTYPE.itemsize == 72 and ro.capi.SNAP_SUMMARY_DTYPE.itemsize == 64
    assert ro.SNAPSHOT_DTYPE is ro.capi.SNAPSHOT_DTYPE and callable(ro.snapshots_host)
    assert (ro.RO_SNAP_CAPTURED, ro.RO_SNAP_EMPTY, ro.RO_SNAP_LOST) == (0, 1, 2)
    for method in ("ring_put_resident", "snapshots_resident"):
        assert callable(getattr(ro.Stft, method)), method
    assert header_constant("RO_SNAP_TILE") == 256
    # the header's own sizes and offsets, through a tiny compiled probe
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ro_stft.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(ro_row_ring_t), sizeof(ro_snapshot_t),\n'
                   '         sizeof(ro_snap_summary_t), offsetof(ro_snapshot_t, first_row), offsetof(ro_snapshot_t, offset),\n'
                   '         offsetof(ro_snapshot_t, rows), offsetof(ro_snapshot_t, status), offsetof(ro_row_ring_t, cols),\n'
                   '         sizeof(ro_stft_config_t), RO_ABI_VERSION);\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 72, 64, 40, 48, 56, 64, 24, 96, 5]
    d = ro.capi.SNAPSHOT_DTYPE
    assert [d.fields[n][1] for n in ("first_row", "offset", "rows", "slot", "status", "reserved")] == [40, 48, 56, 60, 64, 68]
    assert ro.capi.RowRing.cols.offset == 24 and ro.capi.RowRing.ring_rows.offset == 16


def host_args(ro, case, outs, ring):
    p = lambda a: C.c_void_p(a.ctypes.data)
    return dict(events=p(case.events), capacity=case.capacity, summary=p(case.summary), mask=case.mask,
                rows=(C.c_int32 * 8)(*([5] * 8)), ring=ring_desc(ro, case, ring.ctypes.data), head=case.head_row,
                pending=p(outs[2]), count=p(outs[3]), pcap=case.pcap, dir=p(outs[0]), arena=p(outs[1]),
                arena_floats=case.arena_floats, out=p(outs[4]))


def refusals(ro):
    """(changed arguments, word the text must hold)"""
    R = ro.capi.RowRing
    return [(dict(ring=None), "ring"), (dict(ring=R(None, 8, 16, 5, 0)), "d_rows"), (dict(ring=R(1, 8, 0, 5, 0)), "ring_rows"),
            (dict(ring=R(1, 8, 16, 0, 0)), "cols"), (dict(ring=R(1, 4, 16, 5, 0)), "stride"), (dict(ring=R(1, 8, 16, 5, 1)), "reserved"),
            (dict(pending=None), "pending"), (dict(count=None), "pending_count"), (dict(dir=None), "dir"),
            (dict(out=None), "snap_summary"), (dict(events=None), "events"), (dict(summary=None), "summary"),
            (dict(arena=None), "arena"), (dict(capacity=-1), "capacity"), (dict(pcap=-1), "pending_capacity"),
            (dict(arena_floats=-1), "arena_floats"), (dict(head=-1), "head_row"), (dict(mask=0), "slot_mask"),
            (dict(mask=1 << 8), "slot_mask"), (dict(mask=0x1ff), "slot_mask"), (dict(rows=None), "snapshot_rows"),
            (dict(rows=(C.c_int32 * 8)(5, 0, 5, 5, 5, 5, 5, 5), mask=3), "snapshot_rows[1]"),
            (dict(rows=(C.c_int32 * 8)(-1, 5, 5, 5, 5, 5, 5, 5)), "snapshot_rows[0]"),
            (dict(capacity=(1 << 24) + 1), "candidates"), (dict(capacity=1 << 23, pcap=1 << 23, mask=3), "candidates")]


def test_refusals_of_the_host_twin(ro):
    lib = ro.library()
    case = Case(ro, {0: [(30, 4)]}, 5, 16, 5, 40, 100)
    outs, ring = outputs_for(case), case.ring.copy()
    before = [o.copy() for o in outs]

    def call(**kw):
        a = host_args(ro, case, outs, ring)
        a.update(kw)
        return lib.ro_snapshots_host(a["events"], a["capacity"], a["summary"], a["mask"], a["rows"],
                                     C.byref(a["ring"]) if a["ring"] is not None else None, a["head"], a["pending"],
                                     a["count"], a["pcap"], a["dir"], a["arena"], a["arena_floats"], a["out"])
    for kw, word in refusals(ro):
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_snapshots_host:"), (kw, text)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), "a refused call wrote something"
    # what is allowed: no events without an array, no arena without floats, no pending list without room; 2^24 candidates
    assert call(events=None, summary=None, capacity=0) == 0
    assert call(arena=None, arena_floats=0) == 0 and call(pending=None, pcap=0) == 0
    assert call() == 0 and outs[4][:64].view(ro.capi.SNAP_SUMMARY_DTYPE)["captured"][0] == 1
    with pytest.raises(ro.StftError) as e:
        ro.snapshots_host(case.events, case.summary, 0, 5, case.ring, 40, case.pending, case.pending_count, 10)
    assert e.value.code == -1 and "slot_mask" in str(e.value)


def test_refusals_of_the_resident_calls_without_a_handle_and_before_any_launch(ro):
    """the resident calls check everything on the host: a null handle is named, and the other refusals come from the
    checks the host twin shares with them"""
    lib = ro.library()
    ring = ro.capi.RowRing(1, 8, 16, 5, 0)
    rows = (C.c_int32 * 8)(*([5] * 8))
    one = C.c_void_p(1)
    assert lib.ro_stft_ring_put_resident(None, one, 8, 0, 4, C.byref(ring), None) == -1
    assert b"ro_stft_ring_put_resident: null handle" in lib.ro_last_error()
    assert lib.ro_stft_snapshots_resident(None, one, 4, one, 1, rows, C.byref(ring), 40, one, one, 4, one, one, 100, one,
                                          None) == -1
    assert b"ro_stft_snapshots_resident: null handle" in lib.ro_last_error()


def test_the_wrapper_returns_what_the_raw_call_writes(ro):
    case = Case(ro, {0: [(30, 4), (39, 4)], 2: [(28, 2)]}, 5, 16, 5, 40, 100)
    want = host_call(ro, case)
    pending, count = case.pending.copy(), case.pending_count.copy()
    d, arena, sm = ro.snapshots_host(case.events, case.summary, case.mask, 5, case.ring, 40, pending, count, 100, cols=case.cols)
    assert d.tobytes() == want.dir.tobytes() and arena.tobytes() == want.arena.tobytes() and sm.tobytes() == want.summary.tobytes()
    assert pending.tobytes() == want.pending.tobytes() and np.array_equal(count, want.pending_count)
    assert d["status"].tolist() == [CAPTURED, CAPTURED] and d["slot"].tolist() == [0, 2] and count.tolist() == [1, 0, 0]


@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_host_twin_against_the_emulator(ro, emu, case_fn):
    case_fn(ro, host_vs_emu(ro, emu))


def test_random_cases_host_twin_against_the_emulator(ro, emu):
    rng = np.random.default_rng(2024)
    call = host_vs_emu(ro, emu)
    seen = np.zeros(6, np.int64)
    for _ in range(200):
        case = case_from_emu(ro, emu.random_case(rng))
        r = call(case)
        s = r.summary
        seen += [int(s[k]) for k in ("captured", "empty", "lost", "pending", "pending_dropped", "unlisted")]
    assert seen.all(), seen                                  # every outcome turned up
    # the cases vary what the issue asks them to vary
    rng = np.random.default_rng(2024)
    shapes = [emu.random_case(rng) for _ in range(200)]
    assert {bin(a["slot_mask"]).count("1") < a["slot_mask"].bit_length() for a in shapes} == {True, False}     # holes
    assert min(a["ring"].shape[0] for a in shapes) == 1 and max(a["ring"].shape[0] for a in shapes) == 64
    assert min(a["cols"] for a in shapes) == 1 and max(a["cols"] for a in shapes) == 70
    assert {a["pending"].shape[1] for a in shapes} == set(range(9)) and any(a["events"] is None for a in shapes)
    assert max(a["events"].shape[1] for a in shapes if a["events"] is not None) == 40


def test_the_emulator_of_the_kernels_runs_green(emu, capsys):
    assert emu.main(60) == 0
    assert capsys.readouterr().out.startswith("ok: 60 cases")


def test_snapshot_kernels_build_pin(tmp_path):
    """three kernels; none spills or uses scratch; LDS only in the plan kernel: the few words its four waves exchange"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_snapshots.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_snapshots.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.group_segment_fixed_size:\s*(\d+)[\s\S]*?\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)"
                         r"[\s\S]*?\.vgpr_count:\s*(\d+)[\s\S]*?\.vgpr_spill_count:\s*(\d+)", isa)
    seen = {}
    for lds, name, scratch, vgprs, spills in entries:
        short = re.search(r"(ring_put|snap_plan|snap_copy)_kernel", name).group(0)
        print("%s: %s VGPRs, LDS %s, scratch %s, spills %s" % (short, vgprs, lds, scratch, spills))
        assert (int(scratch), int(spills)) == (0, 0), short
        seen[short] = (int(lds), int(vgprs))
    assert sorted(seen) == ["ring_put_kernel", "snap_copy_kernel", "snap_plan_kernel"], entries
    # LDS: two int64 and four counts per wave; the copies hold eight and four floats per lane
    assert seen["snap_plan_kernel"][0] == 128 and seen["ring_put_kernel"][0] == 0 and seen["snap_copy_kernel"][0] == 0
    assert seen["ring_put_kernel"][1] <= 32 and seen["snap_copy_kernel"][1] <= 32 and seen["snap_plan_kernel"][1] <= 128
    # the packed rows are scanned with the DPP ladder: two runs of it
    assert len(re.findall(r"row_bcast:31", isa)) >= 2
    # no atomics anywhere: equal inputs give equal bytes
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_", isa)
