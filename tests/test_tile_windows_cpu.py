"""CPU-side checks of the tile windows (up to 8 column windows cut from each FULL row, csrc/ro_cut_windows.hip): the new
entry points exist, are bound and refuse without a handle; the two pure-host helpers, ro_tile_windows_supported and
ro_merge_windows (against a restatement written here); the new kernel's emitted metadata.  Several recorders with their
own column range are a configuration the reference runs: src/WaterfallBackend.cpp:174-205, :368-374."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
NEW = ("ro_tile_windows_supported", "ro_merge_windows", "ro_stft_cut_windows_resident", "ro_stft_run_resident_windows",
       "ro_stft_set_tile_windows", "ro_stft_tile_windows")


def as_pairs(windows):
    return [(w.first_col, w.cols) for w in windows]


def test_exports_and_abi(ro):
    lib = ro.library()
    header = open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ro.capi.exported_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"#define\s+RO_MAX_TILE_WINDOWS\s+8\b", header) and ro.capi.RO_MAX_TILE_WINDOWS == 8
    assert lib.ro_abi_version() == 5                        # additive: the ABI number and the config struct stay
    # sizeof(ro_stft_config_t) as the library itself states it when it refuses another: 96 bytes, as before
    cfg = ro.capi.Config()
    cfg.struct_size = 1
    h = C.c_void_p()
    assert lib.ro_stft_create(C.byref(cfg), C.byref(h)) == -1
    m = re.search(rb"neither (\d+) \(ABI 2\)", lib.ro_last_error())
    assert m and int(m.group(1)) == C.sizeof(ro.capi.Config) == 96
    for name in ("tile_windows_supported", "merge_windows"):
        assert callable(getattr(ro, name)) and callable(getattr(ro.capi, name))
    for method in ("cut_windows_resident", "run_resident_windows", "set_tile_windows"):
        assert callable(getattr(ro.Stft, method)), method
    assert isinstance(ro.Stft.tile_windows, property)


def test_tile_windows_supported(ro):
    ok = ro.tile_windows_supported
    assert ok(32768, [(0, 32768)])                                      # the whole row as one window
    assert ok(16384, [(1000 + 128 * i, 128) for i in range(8)])         # eight touching windows
    assert ok(16384, [ro.BandWindow(0, 1), ro.BandWindow(16383, 1)])    # one column at either edge
    assert ok(258, [(0, 1), (100, 57), (257, 1)]) and ok(32728, [(5, 11), (32000, 728)])     # chirp-z lengths
    assert ok(32768, [(22528, 2048)]) and ok(32768, [(0, 1025)]) and ok(16384, [(0, 512), (600, 513)])   # above 1024 in all
    assert not ok(16384, [(1000 * i, 100) for i in range(9)])           # nine windows
    assert not ok(16384, [])
    assert not ok(16384, [(5000, 100), (100, 100)])                     # descending
    assert not ok(16384, [(100, 200), (299, 50)])                       # overlapping by one column
    assert not ok(16384, [(100, 100), (300, 0)])                        # an empty window
    assert not ok(16384, [(100, 100), (16285, 100)])                    # ends at bins + 1
    assert ok(16384, [(100, 100), (16284, 100)])
    assert not ok(16384, [(-1, 100)])
    assert not ok(1001, [(0, 10)])                                      # no kernel for these bins
    assert not ok(0, [(0, 1)])
    assert ro.library().ro_tile_windows_supported(16384, None, 1) == 0


def merge_numpy(ranges, limit=8):
    """ro_merge_windows restated: merge what overlaps or touches; while more than `limit` remain, merge the pair with the
    smallest gap, the lower pair on a tie; a range's offset is the image column of its first column"""
    iv = np.array(sorted((lo, lo + n) for lo, n in ranges), dtype=np.int64)
    out = []
    for lo, hi in iv:
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    while len(out) > limit:
        gaps = np.array([out[i + 1][0] - out[i][1] for i in range(len(out) - 1)])
        i = int(np.argmin(gaps))                            # (the first of equal minima: the lower pair)
        out[i][1] = out[i + 1][1]
        del out[i + 1]
    lo = np.array([w[0] for w in out])
    widths = np.array([w[1] - w[0] for w in out])
    starts = np.concatenate(([0], np.cumsum(widths)[:-1]))
    offsets = []
    for first, _ in ranges:
        w = int(np.searchsorted(lo, first, side="right")) - 1
        offsets.append(int(starts[w] + first - lo[w]))
    return [(int(a), int(n)) for a, n in zip(lo, widths)], offsets


def check_merge(ro, ranges, bins):
    windows, offsets = ro.merge_windows(ranges, bins)
    want_w, want_o = merge_numpy(ranges)
    assert as_pairs(windows) == want_w and offsets == want_o
    assert ro.tile_windows_supported(bins, windows)
    # every range sits whole inside the image at its offset: the columns the image holds there are the range's
    cols = np.concatenate([np.arange(lo, lo + n) for lo, n in want_w])
    for (lo, n), off in zip(ranges, offsets):
        assert np.array_equal(cols[off:off + n], np.arange(lo, lo + n))
    return as_pairs(windows), offsets


def test_merge_windows_unsorted_and_nested(ro):
    # radio-observer.json's noise band, detect band and snapshot columns, as three recorders' ranges in no order
    w, off = check_merge(ro, [(23278, 615), (22528, 409), (23415, 410)], 32768)
    assert w == [(22528, 409), (23278, 615)] and off == [409, 0, 409 + 137]
    # nested, touching, duplicated, and a one-column range at either edge of the row
    w, off = check_merge(ro, [(500, 1000), (700, 10), (1500, 20), (500, 1000), (16383, 1), (0, 1), (1521, 5)], 16384)
    assert w == [(0, 1), (500, 1020), (1521, 5), (16383, 1)] and off == [1, 201, 1001, 1, 1026, 0, 1021]
    # one range that is the whole row; a chirp-z length
    assert check_merge(ro, [(0, 32768)], 32768) == ([(0, 32768)], [0])
    check_merge(ro, [(200, 58), (0, 17)], 258)
    # 32 ranges, all overlapping their neighbours: one window
    w, off = check_merge(ro, [(100 * i, 150) for i in reversed(range(32))], 16384)
    assert w == [(0, 3250)] and off == [100 * i for i in reversed(range(32))]


def test_merge_windows_merges_the_smallest_gap(ro):
    # twelve disjoint ranges; gaps 400, 90, 300, 90, 500, 700, 120, 1000, 95, 2000, 90: the smallest (90) three times
    lows = [100, 600, 790, 1190, 1380, 1980, 2780, 3000, 4100, 4295, 6395, 6585]
    ranges = [(lo, 100) for lo in lows]
    assert len(merge_numpy(ranges, limit=99)[0]) == 12
    w, off = check_merge(ro, ranges, 16384)
    assert len(w) == 8
    # four merges: the three 90-column gaps from the bottom up, then the 95
    assert w[1] == (600, 290) and w[2] == (1190, 290) and w[6] == (4100, 295) and w[7] == (6395, 290)
    # the offsets of ranges that went into a wider window: behind the gap's columns, which the image now holds
    assert off[1:3] == [100, 100 + 190] and off[3:5] == [390, 390 + 190]
    # ... and with ONE merge to make, the lower of two equal gaps goes and the upper stays
    nine = [(lo, 100) for lo in (100, 600, 790, 1190, 1380, 1980, 2780, 3000, 4100)]
    w, off = check_merge(ro, nine[::-1], 16384)
    assert w[1] == (600, 290) and w[2] == (1190, 100) and w[3] == (1380, 100)


def test_merge_windows_refusals(ro):
    lib = ro.library()
    for bad in ([(16380, 5)], [(100, 10), (-1, 5)], [(100, 0)], [(100, -3)], [], [(10 * i, 5) for i in range(33)],
                [(0, 32769)]):
        with pytest.raises(ro.StftError) as e:
            ro.merge_windows(bad, 16384)
        assert e.value.code == -1, bad
    with pytest.raises(ro.StftError) as e:
        ro.merge_windows([(100, 10), (16380, 5)], 16384)
    assert "range 1" in str(e.value) and "leaves the row" in str(e.value)
    one = (ro.BandWindow * 1)(ro.BandWindow(0, 4))
    out, n = (ro.BandWindow * 8)(), C.c_int()
    assert lib.ro_merge_windows(None, 1, 16384, out, C.byref(n), None) == -1
    assert lib.ro_merge_windows(one, 1, 16384, None, C.byref(n), None) == -1
    assert lib.ro_merge_windows(one, 1, 16384, out, None, None) == -1
    assert lib.ro_merge_windows(one, 1, 16384, out, C.byref(n), None) == 0 and n.value == 1      # offsets are optional
    assert ro.merge_windows([(10 * i, 5) for i in range(32)], 16384)[0]


def test_new_calls_without_a_handle(ro):
    """A null handle is RO_ERR_INVALID for each of the four handle entry points, like the calls they extend."""
    lib = ro.library()
    w = (ro.BandWindow * 1)(ro.BandWindow(0, 4))
    assert lib.ro_stft_cut_windows_resident(None, None, 0, 0, w, 1, None, 0, None) == -1
    assert b"null" in lib.ro_last_error()
    assert lib.ro_stft_run_resident_windows(None, None, 0, 0, 0, 0, None, 0, w, 1, None, 0, None, None, None) == -1
    assert b"null" in lib.ro_last_error()
    assert lib.ro_stft_set_tile_windows(None, w, 1) == -1
    assert lib.ro_stft_set_tile_windows(None, None, 0) == -1
    assert lib.ro_stft_tile_windows(None, None) == -1
    assert b"null" in lib.ro_last_error()


def test_cut_windows_kernel_build_pin(tmp_path):
    """a plain streaming copy: no scratch, no LDS; one kernel"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_cut_windows.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_cut_windows.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.group_segment_fixed_size:\s*(\d+)[\s\S]*?\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)"
                         r"[\s\S]*?\.vgpr_count:\s*(\d+)[\s\S]*?\.vgpr_spill_count:\s*(\d+)", isa)
    assert len(entries) == 1 and "cut_windows_kernel" in entries[0][1], entries
    lds, name, scratch, vgprs, spills = entries[0]
    print("cut_windows_kernel: %s VGPRs, LDS %s, scratch %s, spills %s" % (vgprs, lds, scratch, spills))
    assert (int(lds), int(scratch), int(spills)) == (0, 0, 0)
    assert int(vgprs) == 20
    assert "ds_" not in isa and "atomic" not in isa and "scratch_" not in isa
