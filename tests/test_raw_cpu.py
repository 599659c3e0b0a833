"""CPU-side checks of the raw I/Q capture (csrc/ro_raw.hip, ro_raw_host): the two entry points exist, are declared and bound,
and the three structs have their ABI sizes in the header and in the binding; the raw length against the oracle's
fftSamplesToRaw and the first sample against the closed form; the host mirror's raws.fits image against ro_raw_host on the
same event and samples, with and without overlap; every refusal names its argument; ro_raw_host against the numpy
restatement of the rules (tools/raw/emu_raw.py) on the decision table and on 200 seeded random cases, with guard entries
behind every output; the conversions of the three formats; the kernels' emitted metadata.  Every comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hostlib import BolidEvent
from rawlib import (CAPTURED, EMPTY, EMU, F32, F64, I16, LOST, ROOT, TABLE, Case, L_of, apply_refusal, case_from_emu, f_of,
                    header_constant, host_call, host_vs_emu, outputs_for, refusals, snaps_of, span_structs, statuses)
from test_host_cpu import H, manual, read_fits  # noqa: F401  (H is the harness fixture)

BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_stft_raw_resident", "ro_raw_host")


def test_exports_and_abi(ro, tmp_path):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("ro_iq_span_t", "ro_raw_capture_t", "ro_raw_summary_t"):
        assert re.search(r"\}\s*%s;" % name, header), name
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    assert C.sizeof(ro.capi.Config) == 96
    assert C.sizeof(ro.capi.IqSpan) == 32 and ro.capi.RO_MAX_IQ_SPANS == 4
    assert ro.capi.RAW_CAPTURE_DTYPE.itemsize == 72 and ro.capi.RAW_SUMMARY_DTYPE.itemsize == 64
    assert ro.RAW_CAPTURE_DTYPE is ro.capi.RAW_CAPTURE_DTYPE and ro.IqSpan is ro.capi.IqSpan and callable(ro.raw_host)
    assert callable(ro.Stft.raw_resident)
    assert header_constant("RO_RAW_BLOCK") % 64 == 0 and header_constant("RO_RAW_TILE") == 256
    # the header's own sizes and offsets, through a tiny compiled probe
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ro_stft.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(ro_iq_span_t),\n'
                   '         sizeof(ro_raw_capture_t), sizeof(ro_raw_summary_t), offsetof(ro_iq_span_t, first_sample),\n'
                   '         offsetof(ro_iq_span_t, samples), offsetof(ro_iq_span_t, format), offsetof(ro_iq_span_t, reserved),\n'
                   '         offsetof(ro_raw_capture_t, first_sample), offsetof(ro_raw_capture_t, samples),\n'
                   '         offsetof(ro_raw_capture_t, offset), offsetof(ro_raw_capture_t, slot), offsetof(ro_raw_capture_t, status),\n'
                   '         sizeof(ro_stft_config_t), RO_MAX_IQ_SPANS, RO_ABI_VERSION);\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 72, 64, 8, 16, 24, 28, 40, 48, 56, 64, 68, 96, 4, 5]
    d = ro.capi.RAW_CAPTURE_DTYPE
    assert [d.fields[n][1] for n in ("first_sample", "samples", "offset", "slot", "status")] == [40, 48, 56, 64, 68]
    assert list(ro.capi.RAW_SUMMARY_DTYPE.names) == ["resolved", "captured", "empty", "lost", "pending", "pending_dropped",
                                                     "arena_floats", "reserved"]
    Sp = ro.capi.IqSpan
    assert (Sp.first_sample.offset, Sp.samples.offset, Sp.format.offset, Sp.reserved.offset) == (8, 16, 24, 28)


# ---- the length and the first sample ------------------------------------------------------------------------------------
def resolves_at(ro, shape, case, f, head):
    """the status a snapshot resolves with when the spans end at `head` -- base f + 1, so that no sample is read: a run with
    L > 0 is LOST there -- or None while it is still pending"""
    buf = np.zeros((4, 2), np.float32)
    outs = outputs_for(case)
    span = (ro.capi.IqSpan * 1)(ro.capi.IqSpan(buf.ctypes.data, f + 1, head - f - 1, F32, 0))
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert ro.library().ro_raw_host(*shape, p(case.directory), 1, p(case.snap_summary), span, 1, p(outs[2]), p(outs[3]), 1,
                                    p(outs[0]), None, 0, p(outs[4])) == 0, ro.library().ro_last_error()
    sm = outs[4][:64].view(ro.capi.RAW_SUMMARY_DTYPE)[0]
    entry = outs[0][:72].view(ro.capi.RAW_CAPTURE_DTYPE)[0]
    assert int(sm["resolved"]) + int(sm["pending"]) == 1
    if not int(sm["resolved"]):
        return None
    assert int(entry["first_sample"]) == f and int(entry["samples"]) == 0
    return int(entry["status"])


@pytest.mark.parametrize("shape", [(32768, 24576, 48000), (4096, 2048, 48000), (256, 1, 48000), (1024, 0, 96000)])
def test_raw_length_is_the_recorders_fft_samples_to_raw(ro, oracle, shape):
    bins, overlap, rate = shape
    fft_rate = oracle.lib().ro_oracle_fft_sample_rate(rate, bins, overlap)
    assert int(fft_rate) == EMU.int_rate(*shape) >= 1
    for length in range(0, 401):
        want = oracle.lib().ro_oracle_recorder_fft_samples_to_raw(length, fft_rate, rate)
        assert L_of(shape, length) == want, length           # the emulator's restatement
        if length in (0, 1, 2) or want <= 64:
            # directly: a captured run of `want` samples
            case = Case(ro, shape, [(3, length)], [(0, f_of(shape, 3) + want + 5, I16)], 2 * want + 2, pcap=1)
            r = host_call(ro, case)
            assert statuses(r) == ([CAPTURED] if want else [EMPTY]) and int(r.dir[0]["samples"]) == want, (length, r.dir)
        if want >= 3:
            # L itself, without a sample being read: the run resolves exactly when f + L <= head_sample
            case = Case(ro, shape, [(3, length)], [(0, 1, F32)], 0, pcap=1)
            f = f_of(shape, 3)
            assert resolves_at(ro, shape, case, f, f + want) == LOST and resolves_at(ro, shape, case, f, f + want - 1) is None, length
    assert L_of((32768, 24576, 48000), 5) == 48000 and L_of((32768, 24576, 48000), 400) > 400 * 8192   # 5.86 / 5


def test_a_shape_whose_integer_fft_rate_is_zero_is_refused(ro):
    case = Case(ro, (64, 48, 1000), [(3, 4)], [(0, 500, F32)], 100)
    outs = outputs_for(case)
    before = [o.copy() for o in outs]
    p = lambda a: C.c_void_p(a.ctypes.data)
    for shape in ((32768, 0, 16000), (1024, 0, 1023), (256, 1, 200)):
        assert int(np.float32(shape[2]) / np.float32(shape[0] - shape[1])) == 0
        rc = ro.library().ro_raw_host(*shape, p(case.directory), 1, p(case.snap_summary),
                                      span_structs(ro, case, [case.spans[0][0].ctypes.data]), 1, p(outs[2]), p(outs[3]), case.pcap,
                                      p(outs[0]), p(outs[1]), 100, p(outs[4]))
        assert rc == -2 and "fft sample rate" in ro.library().ro_last_error().decode(), shape
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before))
    with pytest.raises(ro.StftError) as e:
        ro.raw_host(1024, 0, 1023, case.directory, case.snap_summary, [(case.spans[0][0], 0, F32)], case.pending,
                    case.pending_count, 100)
    assert e.value.code == -2


@pytest.mark.parametrize("shape", [(64, 0, 1000), (64, 48, 1000), (4096, 2048, 48000), (4096, 0, 48000)])
def test_first_sample_is_the_raw_mark_of_the_row_in_front(ro, shape):
    """f = (start - z) hop + 1 for start >= 1, z = (overlap == 0), and 0 at and below row 0"""
    hop, z = shape[0] - shape[1], int(shape[1] == 0)
    starts = [-3, 0, 1, 2, 57]
    want = [0, 0, (1 - z) * hop + 1, (2 - z) * hop + 1, (57 - z) * hop + 1]
    # (a base behind every f: the runs resolve as LOST, with their first samples, and no sample is read)
    case = Case(ro, shape, [(s, 4) for s in starts], [(want[-1] + 1, L_of(shape, 4) + 5, I16)], 0, pcap=0)
    r = host_call(ro, case)
    assert statuses(r) == [LOST] * 5 and r.dir["first_sample"].tolist() == want


# ---- the mirror: the reference's writeRaw() through the host mirror, against the host twin ------------------------------------
@pytest.mark.parametrize("overlap", [2048, 0])
def test_the_host_mirrors_raw_image_is_the_host_twins_run(ro, H, oracle, tmp_path, overlap):  # noqa: F811
    """driven exactly as test_host_cpu.py::test_bolid_event_writes_band_snapshot_and_raw_iq drives it: the raws.fits image
    of the event; the same event as a CAPTURED directory entry and the same samples as one F64 span give the same L, the
    same first sample and the same floats"""
    bins, rate = 4096, 48000
    hop = bins - overlap
    m, info = manual(H, tmp_path, bins=bins, overlap=overlap, snap_len=4, lo=9000.0, hi=12000.0, adv=0.1, jit=0.3)
    raw_cap = H.ro_host_manual_raw_capacity(m)
    assert raw_cap > 0
    H.ro_host_manual_set_clock(m, 1700000000 + 2 * 3600 + 17, 123456)
    fft_rate = oracle.lib().ro_oracle_fft_sample_rate(rate, bins, overlap)
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
    assert H.ro_host_manual_bolid_files(m, 1, buf, 8192) == 1
    hdr, data, _ = read_fits(buf.value.decode().split()[0])
    assert (e.start, e.length) == (31 - adv, 2 * adv + 6) and int(hdr["NAXIS1"]) == 2
    # the same event through the host twin
    entry = np.zeros(1, ro.capi.SNAPSHOT_DTYPE)
    entry["event"]["start_row"], entry["event"]["length"] = e.start, e.length
    entry["first_row"], entry["rows"], entry["status"] = e.start, e.length, CAPTURED
    sm = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
    sm["resolved"] = 1
    d, arena, out = ro.raw_host(bins, overlap, rate, entry, sm, [(iq, 0, F64)], np.zeros(0, ro.capi.SNAPSHOT_DTYPE),
                                np.zeros(1, np.int64), 2 * (e.rawLength + 8))
    assert d["status"].tolist() == [CAPTURED]
    L, f = int(d[0]["samples"]), int(d[0]["first_sample"])
    assert L == e.rawLength == int(hdr["NAXIS2"]) and L > e.length * hop
    assert f == (e.start - (overlap == 0)) * hop + 1 and f + L <= raw_cap      # (the mirror's ring has not wrapped)
    assert arena.tobytes() == data.astype("<f4").tobytes() == iq[f:f + L].astype(np.float32).tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_twin(ro):
    lib = ro.library()
    case = Case(ro, (64, 48, 1000), [(20, 4)], [(300, 200, F32)], 200)
    outs, samples = outputs_for(case), case.spans[0][0].copy()
    before = [o.copy() for o in outs]
    base = span_structs(ro, case, [samples.ctypes.data])
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(**kw):
        a = dict(dir=p(case.directory), dcap=1, snap_summary=p(case.snap_summary), spans=base, span_count=1, pending=p(outs[2]),
                 count=p(outs[3]), pcap=case.pcap, raw_dir=p(outs[0]), arena=p(outs[1]), arena_floats=200, out=p(outs[4]),
                 shape=case.shape)
        a.update(apply_refusal(ro, base, kw))
        return lib.ro_raw_host(*a["shape"], a["dir"], a["dcap"], a["snap_summary"], a["spans"], a["span_count"], a["pending"],
                               a["count"], a["pcap"], a["raw_dir"], a["arena"], a["arena_floats"], a["out"])
    for kw, word in refusals(ro, "") + [(dict(shape=(1, 0, 1000)), "bins")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_raw_host:"), (kw, text)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), "a refused call wrote something"
    # what is allowed: no directory without entries, no arena without floats, no pending list without room; spans that touch
    assert call(dir=None, dcap=0) == 0 and call(arena=None, arena_floats=0) == 0 and call(pending=None, pcap=0) == 0
    assert call(spans=[dict(samples=100), dict(first_sample=400, samples=100)]) == 0
    assert call() == 0 and outs[4][:64].view(ro.capi.RAW_SUMMARY_DTYPE)["captured"][0] == 1
    with pytest.raises(ro.StftError) as e:
        ro.raw_host(64, 48, 1000, case.directory, case.snap_summary, [], case.pending, case.pending_count, 10)
    assert e.value.code == -1 and "span_count" in str(e.value)


def test_refusal_of_the_resident_call_without_a_handle(ro):
    lib = ro.library()
    one = C.c_void_p(8)
    spans = (ro.capi.IqSpan * 1)(ro.capi.IqSpan(8, 0, 10, F32, 0))
    assert lib.ro_stft_raw_resident(None, one, 4, one, spans, 1, one, one, 4, one, one, 100, one, None) == -1
    assert b"ro_stft_raw_resident: null handle" in lib.ro_last_error()


def test_the_wrapper_returns_what_the_raw_call_writes(ro):
    case = Case(ro, (64, 48, 1000), [(20, 4), (40, 4), (21, 4, EMPTY), (10, 3)], [(300, 200, I16), (450, 100, F64)], 400)
    want = host_call(ro, case)
    pending, count = case.pending.copy(), case.pending_count.copy()
    d, arena, sm = ro.raw_host(*case.shape, case.directory, case.snap_summary, case.spans, pending, count, 400)
    assert d.tobytes() == want.dir.tobytes() and arena.tobytes() == want.arena.tobytes() and sm.tobytes() == want.summary.tobytes()
    assert pending.tobytes() == want.pending.tobytes() and np.array_equal(count, want.pending_count)
    assert d["status"].tolist() == [CAPTURED, LOST] and count.tolist() == [1]


# ---- the rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_host_twin_against_the_emulator(ro, case_fn):
    case_fn(ro, host_vs_emu(ro))


def test_random_cases_host_twin_against_the_emulator(ro):
    rng = np.random.default_rng(2025)
    call = host_vs_emu(ro)
    seen = np.zeros(5, np.int64)
    shapes = []
    for _ in range(200):
        args = EMU.random_case(rng)
        shapes.append(args)
        s = call(case_from_emu(ro, args)).summary
        seen += [int(s[k]) for k in ("captured", "empty", "lost", "pending", "pending_dropped")]
    assert seen.all(), seen                                  # every outcome turned up
    assert {len(a["spans"]) for a in shapes} == {1, 2, 3, 4} and {a["overlap"] == 0 for a in shapes} == {True, False}
    assert {fmt for a in shapes for _, _, fmt in a["spans"]} == {F32, I16, F64}
    assert any(a["resolved"] > len(a["directory"]) for a in shapes) and any(a["resolved"] < 0 for a in shapes)
    assert any(a["pending_count"][0] > len(a["pending"]) for a in shapes) and any(a["pending_count"][0] < 0 for a in shapes)


def test_the_emulator_of_the_kernels_runs_green(capsys):
    assert EMU.main(60) == 0
    assert capsys.readouterr().out.startswith("ok: 60 cases")


# ---- values ------------------------------------------------------------------------------------------------------------------
def one_span_run(ro, array, fmt):
    """every sample of `array` as one captured run"""
    shape = (2, 1, 1)                                         # hop 1, R = 1, sample rate 1: L = len, f = start + 1
    n = len(array)
    entry = snaps_of(ro, [(1, n)])
    sm = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
    sm["resolved"] = 1
    d, arena, _ = ro.raw_host(*shape, entry, sm, [(array, 2, fmt)], np.zeros(0, ro.capi.SNAPSHOT_DTYPE), np.zeros(1, np.int64), 2 * n)
    assert d["status"].tolist() == [CAPTURED] and int(d[0]["first_sample"]) == 2 and int(d[0]["samples"]) == n
    return arena


def test_values_of_the_three_formats(ro):
    # F32: a bit copy -- NaN payloads, -0.0, denormals survive
    bits = np.array([[0x7fc12345, 0xffa00001], [0x80000000, 0x00000001], [0x7f800000, 0x3f800000]], np.uint32)
    assert one_span_run(ro, bits.view(np.float32), F32).tobytes() == bits.tobytes()
    # I16: (float) of each int16, the extremes included
    i16 = np.array([[-32768, 32767], [0, -1], [1, 12345]], np.int16)
    assert one_span_run(ro, i16, I16).tobytes() == i16.astype(np.float32).tobytes()
    # F64: round to nearest even; ties, overflow, -0.0, a NaN
    f64 = np.array([[1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24], [1e300, -1e300], [-0.0, np.nan], [0.1, -1 / 3]], np.float64)
    got = one_span_run(ro, f64, F64).reshape(-1)
    with np.errstate(over="ignore"):
        want = f64.astype(np.float32).reshape(-1)
    assert want[0] == 1.0 and want[1] == np.float32(1 + 2.0 ** -22) and np.isinf(want[2]) and np.signbit(want[4])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


# ---- the kernels' metadata ---------------------------------------------------------------------------------------------------
def test_raw_kernels_build_pin(tmp_path):
    """two kernels; neither spills or uses scratch; LDS only in the plan kernel: the few words its four waves exchange; no
    atomics"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_raw.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_raw.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.group_segment_fixed_size:\s*(\d+)[\s\S]*?\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)"
                         r"[\s\S]*?\.vgpr_count:\s*(\d+)[\s\S]*?\.vgpr_spill_count:\s*(\d+)", isa)
    seen = {}
    for lds, name, scratch, vgprs, spills in entries:
        short = re.search(r"raw_(plan|copy)_kernel", name).group(0)
        print("%s: %s VGPRs, LDS %s, scratch %s, spills %s" % (short, vgprs, lds, scratch, spills))
        assert (int(scratch), int(spills)) == (0, 0), short
        seen[short] = (int(lds), int(vgprs))
    assert sorted(seen) == ["raw_copy_kernel", "raw_plan_kernel"], entries
    # LDS: four int64 and four counts per wave
    assert seen["raw_plan_kernel"][0] == 192 and seen["raw_copy_kernel"][0] == 0
    assert seen["raw_plan_kernel"][1] <= 128 and seen["raw_copy_kernel"][1] <= 128
    # the pairs and the blocks are scanned with the DPP ladder: four 16-bit limbs each
    assert len(re.findall(r"row_bcast:31", isa)) >= 8
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_", isa)
