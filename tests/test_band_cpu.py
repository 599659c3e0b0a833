"""CPU-side checks of the band-only transform (ro_stft_band_resident, csrc/ro_band.hip): the derivation and the kernel's
index maps against numpy's FFT (tools/band/emu_band.py), the two pure-host entry points, and the emitted ISA."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's


def test_the_index_maps_reproduce_numpys_fft():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "band", "emu_band.py")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "all band maps ok"
    seen = {}
    for line in lines[:-1]:
        m = re.match(r"bins\s+(\d+)\s+cols\s+(\d+)\s+M\s+(\d+)\s+A\s+(\d+)\s+slabs\s+(\d+): max err / row max (\S+)$", line)
        assert m, line
        bins, cols, mm, a, slabs = (int(m.group(i)) for i in range(1, 6))
        assert mm * a * slabs == bins and mm >= cols and float(m.group(6)) < 1e-12
        seen[(bins, cols)] = mm
    for shape in ((16384, 256), (16384, 1024), (65536, 600), (524288, 218)):
        assert shape in seen, shape
    assert set(seen.values()) == {256, 512, 1024}          # every transform length the library has


def test_band_supported(ro):
    for bins, cols in ((16384, 1), (16384, 1024), (1048576, 1024), (65536, 600)):
        assert ro.band_supported(bins, cols), (bins, cols)
    for bins, cols in ((8192, 256), (16384, 1025), (16384, 0), (32728, 256), (2097152, 256)):
        assert not ro.band_supported(bins, cols), (bins, cols)


def hull_numpy(b, tile=None):
    lo = [b.low_noise, b.low_detect - b.avg_bins // 2] + ([tile[0]] if tile else [])
    hi = [b.low_noise + b.noise_width, b.low_detect + b.detect_width - 1 - b.avg_bins // 2 + b.avg_bins] + ([sum(tile)] if tile else [])
    return min(lo), max(hi) - min(lo)


@pytest.mark.parametrize("bins,rate,overlap,freqs", [
    (32768, 48000, 24576, (10300, 10900, 9000, 9600, 2, 5, 40)),          # radio-observer.json:62-87
    (65536, 96000, 49152, (26450, 26550, 26000, 26300, 5, 2, 40)),        # Bolidozor.json:84-93
])
def test_bands_hull(ro, oracle, bins, rate, overlap, freqs):
    ob = oracle.bolid_bands(bins, rate, overlap, *freqs)
    b = ro.Bands(low_noise=ob.low_noise, noise_width=ob.noise_width, low_detect=ob.low_detect,
                 detect_width=ob.detect_width, avg_bins=ob.avg_bins)
    first, cols = ro.bands_hull(b, bins)
    assert (first, cols) == hull_numpy(b)
    # every column the scan can touch is inside: the noise band, the detect band, the average's window at either end
    assert first <= b.low_noise and b.low_noise + b.noise_width <= first + cols
    for peak in (0, b.detect_width - 1):
        start = b.low_detect + peak - b.avg_bins // 2
        assert first <= start and start + b.avg_bins <= first + cols
    # with a tile: the snapshot's columns too, on either side of the bands
    for tile in ((first - 100, 50), (first + cols + 7, 33), (first + 5, 10)):
        assert ro.bands_hull(b, bins, *tile) == hull_numpy(b, tile)
    with pytest.raises(ro.StftError) as e:
        ro.bands_hull(b, bins, bins - 10, 11)
    assert e.value.code == -1


def test_bands_hull_refuses_a_window_that_leaves_the_row(ro):
    b = ro.Bands(low_noise=500, noise_width=100, low_detect=0, detect_width=50, avg_bins=27)
    with pytest.raises(ro.StftError) as e:
        ro.bands_hull(b, 16384)
    assert e.value.code == -1 and "leaves the row" in str(e.value)
    b.low_detect = 13                                       # avg_bins // 2: the window just fits
    assert ro.bands_hull(b, 16384) == (0, 600)
    b.low_detect, b.low_noise = 16384 - 50, 16000           # ... and runs past the last column at the other end
    with pytest.raises(ro.StftError):
        ro.bands_hull(b, 16384)
    assert ro.library().ro_bands_hull(None, 16384, 0, 0, None, None) == -1


def test_band_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_band.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_band.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)", isa)
    # three transform lengths x two sample formats, and the finishing kernel
    assert len([n for n, _ in entries if "band_slab_kernel" in n]) == 6
    assert len([n for n, _ in entries if "band_finish_kernel" in n]) == 1
    bad = [(n, int(s)) for n, s in entries if int(s) != 0]
    assert not bad, bad
    # two workgroups of the 64 KiB kernels share a CU's 160 KiB
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", isa)]
    assert max(lds) == 65536
