"""CPU-side checks of the band-only transform over several column windows (ro_stft_band_windows_resident): the window-list
gather's index maps against numpy's FFT (tools/band/emu_band_windows.py) and the two pure-host entry points,
ro_bands_windows and ro_stft_band_windows_supported."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's


def test_the_window_gather_reproduces_numpys_fft():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "band", "emu_band_windows.py")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "all band window maps ok"
    kinds, colliding = set(), 0
    for line in lines[:-1]:
        m = re.match(r"(f32|f64)\s+bins\s+(\d+)\s+M\s+(\d+)\s+A\s+(\d+)\s+slabs\s+(\d+)\s+(\d+) windows,\s+(\d+) columns,"
                     r"\s+(\d+) share a residue \(([^)]*)\): max err / row max ([0-9.e+-]+)", line)
        assert m, line
        bins, mm, a, slabs, count, cols, shared = (int(m.group(i)) for i in range(2, 9))
        assert mm * a * slabs == bins and mm >= cols and 1 <= count <= 8
        assert float(m.group(10)) < 1e-12, line
        kinds.add((m.group(1), mm))
        if "colliding" in m.group(9):
            assert shared > 0 and cols <= mm, line
            colliding += 1
        if m.group(1) == "f64":                             # recorded, not gated: the figure is there
            assert re.search(r"gather worst LDS cycles per 16-lane group \d+ \(one band of \d+ columns: \d+\)", line), line
    assert colliding >= 2                                   # one per precision at the least
    assert kinds == {(p, mm) for p in ("f32", "f64") for mm in (256, 512, 1024)}


def as_pairs(windows):
    return [(w.first_col, w.cols) for w in windows]


def reads(b):
    """the two intervals [lo, hi) a band set reads: its noise band, its detect band with the average's margin"""
    return [(b.low_noise, b.low_noise + b.noise_width),
            (b.low_detect - b.avg_bins // 2, b.low_detect + b.detect_width - 1 - b.avg_bins // 2 + b.avg_bins)]


def windows_numpy(intervals, limit=8):
    """ro_bands_windows restated: merge what overlaps or touches; while more than `limit` remain, merge the pair with the
    smallest gap, the lower pair on a tie"""
    out = []
    for lo, hi in sorted(intervals):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    while len(out) > limit:
        gaps = [out[i + 1][0] - out[i][1] for i in range(len(out) - 1)]
        i = gaps.index(min(gaps))
        out[i][1] = out[i + 1][1]
        del out[i + 1]
    return [(lo, hi - lo) for lo, hi in out]


def radio_observer(ro, oracle):
    """radio-observer.json: the bolid recorder's bands and the snapshot's columns at 32768 bins, 48 kHz"""
    bins, fs, overlap = 32768, 48000, 24576
    ob = oracle.bolid_bands(bins, fs, overlap, 10300, 10900, 9000, 9600, 2, 5, 40)
    b = ro.Bands(low_noise=ob.low_noise, noise_width=ob.noise_width, low_detect=ob.low_detect,
                 detect_width=ob.detect_width, avg_bins=ob.avg_bins)
    t0, t1 = ro.frequency_to_bin(bins, fs, 10100.0), ro.frequency_to_bin(bins, fs, 11000.0)
    return bins, b, (t0, t1 - t0)


def test_bands_windows_radio_observer(ro, oracle):
    bins, b, tile = radio_observer(ro, oracle)
    w = ro.bands_windows(b, bins, *tile)
    assert as_pairs(w) == windows_numpy(reads(b) + [(tile[0], sum(tile))])
    assert len(w) == 2
    assert sum(x.cols for x in w) <= 1024
    assert ro.band_windows_supported(bins, w)
    assert ro.band_windows_supported(bins, as_pairs(w), ro.RO_PRECISION_F32)
    # the noise band is a window of its own; the detect band and the tile share the other
    assert as_pairs(w)[0] == (b.low_noise, b.noise_width)
    lo, hi = reads(b)[1]
    assert w[1].first_col <= min(lo, tile[0]) and max(hi, sum(tile)) <= w[1].first_col + w[1].cols
    # one range over the same inputs is too wide for the band kernels
    first, cols = ro.bands_hull(b, bins, *tile)
    assert cols > 1024 and not ro.band_supported(bins, cols)
    # without the tile: the two intervals of the set, as they are
    assert as_pairs(ro.bands_windows([b], bins)) == windows_numpy(reads(b))


def test_bands_windows_touching_sets_merge(ro):
    a = ro.Bands(low_noise=1000, noise_width=100, low_detect=3000, detect_width=50, avg_bins=9)
    # b's noise band starts where a's ends; its detect interval [3046 - 5, 3046 + 20 - 1 - 5 + 11) = [3041, 3071) overlaps
    # a's [2996, 3054)
    b = ro.Bands(low_noise=1100, noise_width=60, low_detect=3046, detect_width=20, avg_bins=11)
    assert reads(a)[0][1] == reads(b)[0][0]
    w = as_pairs(ro.bands_windows([a, b], 16384))
    assert w == windows_numpy(reads(a) + reads(b)) == [(1000, 160), (2996, 75)]
    # a tile that touches the second window from above joins it
    assert as_pairs(ro.bands_windows([a, b], 16384, 3071, 29)) == [(1000, 160), (2996, 104)]
    # ... and one column further up it is a window of its own
    assert as_pairs(ro.bands_windows([a, b], 16384, 3072, 29)) == [(1000, 160), (2996, 75), (3072, 29)]


def test_bands_windows_merges_the_smallest_gap(ro):
    # four sets and a tile: nine disjoint intervals; gaps 400, 90, 300, 90, 500, 700, 120, 1000 -- the smallest (90) twice
    lows = [100, 600, 790, 1190, 1380, 1980, 2780, 3000, 4100]
    sets = [ro.Bands(low_noise=lows[2 * i], noise_width=100, low_detect=lows[2 * i + 1] + 4, detect_width=92, avg_bins=9)
            for i in range(4)]
    tile = (lows[8], 100)
    intervals = [iv for s in sets for iv in reads(s)] + [(tile[0], sum(tile))]
    assert sorted(intervals) == [(lo, lo + 100) for lo in lows]
    assert len(windows_numpy(intervals, limit=99)) == 9
    w = as_pairs(ro.bands_windows(sets, 16384, *tile))
    assert len(w) == 8 and w == windows_numpy(intervals)
    assert w[1] == (600, 290) and w[2] == (1190, 100)       # the LOWER of the two 90-column gaps went
    # eight sets, sixteen disjoint intervals: eight come back
    many = [ro.Bands(low_noise=200 * i + 1000 * (i // 3), noise_width=50, low_detect=200 * i + 1000 * (i // 3) + 104,
                     detect_width=42, avg_bins=9) for i in range(8)]
    w = as_pairs(ro.bands_windows(many, 16384))
    assert len(w) == 8 and w == windows_numpy([iv for s in many for iv in reads(s)])


def test_bands_windows_refusals(ro):
    lib = ro.library()
    ok = ro.Bands(low_noise=500, noise_width=100, low_detect=1000, detect_width=50, avg_bins=27)
    bad = ro.Bands(low_noise=500, noise_width=100, low_detect=0, detect_width=50, avg_bins=27)      # the margin leaves the row
    with pytest.raises(ro.StftError) as e:
        ro.bands_windows([ok, bad], 16384)
    assert e.value.code == -1 and "leaves the row" in str(e.value)
    with pytest.raises(ro.StftError) as e:
        ro.bands_windows(ok, 16384, 16384 - 10, 11)
    assert e.value.code == -1 and "leaves the row" in str(e.value)
    with pytest.raises(ro.StftError):
        ro.bands_windows([ok] * 9, 16384)
    with pytest.raises(ro.StftError):
        ro.bands_windows([], 16384)
    with pytest.raises(ro.StftError):
        ro.bands_windows(ro.Bands(low_noise=500, noise_width=0, low_detect=1000, detect_width=50, avg_bins=27), 16384)
    assert lib.ro_bands_windows(None, 1, 16384, 0, 0, None, None) == -1


def test_band_windows_supported(ro):
    eight = [(1000 * i, 128) for i in range(8)]
    assert ro.band_windows_supported(16384, eight)
    assert ro.band_windows_supported(16384, [ro.BandWindow(*w) for w in eight])
    assert ro.band_windows_supported(16384, [(0, 512), (512, 512)])                     # touching; 1024 in all
    assert ro.band_windows_supported(16384, [(0, 100), (16284, 100)])                   # the row's two edges
    assert not ro.band_windows_supported(16384, [(1000 * i, 100) for i in range(9)])    # nine windows
    assert not ro.band_windows_supported(16384, [])
    assert not ro.band_windows_supported(16384, [(0, 512), (600, 513)])                 # 1025 in all
    assert not ro.band_windows_supported(16384, [(100, 200), (299, 50)])                # overlapping
    assert not ro.band_windows_supported(16384, [(5000, 100), (100, 100)])              # not ascending
    assert not ro.band_windows_supported(16384, [(100, 100), (300, 0)])                 # an empty window
    assert not ro.band_windows_supported(16384, [(100, 100), (16300, 100)])             # past the last column
    assert not ro.band_windows_supported(16384, [(-1, 100)])
    assert not ro.band_windows_supported(8192, eight)                                   # below the float32 kernels' sizes
    assert ro.band_windows_supported(131072, eight, ro.RO_PRECISION_F64)
    assert not ro.band_windows_supported(65536, eight, ro.RO_PRECISION_F64)             # FP64 starts at 131072 bins
    assert ro.band_windows_supported(65536, eight, ro.RO_PRECISION_F32)
    assert not ro.band_windows_supported(131072, eight, 7)
    assert ro.library().ro_stft_band_windows_supported(16384, None, 1, ro.RO_PRECISION_F32) == 0


def test_abi_version_and_exports(ro):
    lib = ro.library()
    assert lib.ro_abi_version() == 5
    for name in ("ro_stft_band_windows_supported", "ro_bands_windows", "ro_stft_band_windows_resident"):
        assert getattr(lib, name) is not None
        assert name in open(os.path.join(ROOT, "include", "ro_stft.h")).read()
    for name in ("BandWindow", "band_windows_supported", "bands_windows"):
        assert hasattr(ro, name), name
    assert hasattr(ro.Stft, "band_windows_resident")
    assert ro.capi.RO_MAX_BAND_WINDOWS == 8
    assert C.sizeof(ro.BandWindow) == 8


@pytest.mark.parametrize("source,slab,finish,count,lds_limit", [
    ("ro_band_windows.hip", "bandw_slab_kernel", "bandw_finish_kernel", 6, 64 << 10),
    ("ro_band_windows_f64.hip", "band64w_slab_kernel", "band64w_finish_kernel", 9, 80 << 10),
])
def test_window_kernels_use_no_scratch(tmp_path, source, slab, finish, count, lds_limit):
    """the window-list kernels keep what tests/test_band_cpu.py and tests/test_band_f64_cpu.py pin for the consecutive
    call's: three transform lengths x the sample formats and one finishing kernel, no scratch, two workgroups per CU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / (source + ".s"))
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", source), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)", isa)
    assert len([n for n, _ in entries if slab in n]) == count
    assert len([n for n, _ in entries if finish in n]) == 1
    bad = [(n, int(x)) for n, x in entries if int(x) != 0]
    assert not bad, bad
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", isa)]
    assert max(lds) == 65536 <= lds_limit
