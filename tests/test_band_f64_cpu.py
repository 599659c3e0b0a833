"""CPU-side checks of the FP64 band-only transform (ro_stft_band_resident on RO_PRECISION_F64 handles of 131072 bins and
above, csrc/ro_band_f64.hip): the kernel's index maps and LDS swizzle against numpy's FFT (tools/band/emu_band_f64.py),
the pure-host entry point that knows the precision, and the emitted code's resources."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-slp-vectorize"]       # radio-observer_amd/build.py's
SHAPES = ((131072, 256), (131072, 300), (131072, 1024), (524288, 218), (1048576, 1024))


def test_the_f64_index_maps_reproduce_numpys_fft():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "band", "emu_band_f64.py")], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "all f64 band maps ok"
    seen = {}
    for line in lines[:-1]:
        m = re.match(r"bins\s+(\d+)\s+cols\s+(\d+)\s+M\s+(\d+)\s+A\s+(\d+)\s+slabs\s+(\d+): max err / row max (\S+), "
                     r"worst LDS conflict per level (\d+)\b", line)
        assert m, line
        bins, cols, mm, a, slabs = (int(m.group(i)) for i in range(1, 6))
        assert mm * a * slabs == bins and mm >= cols and mm * a == 4096
        assert float(m.group(6)) < 1e-12
        assert 1 <= int(m.group(7)) <= 4                    # 4 = the unpadded image at A = 4; the swizzle is there to beat it
        seen[(bins, cols)] = mm
    assert set(seen) == set(SHAPES)
    assert set(seen.values()) == {256, 512, 1024}


def test_band_supported_with_precision(ro):
    lib = ro.library()
    # test_band_cpu.py's table: float32 answers are ro_stft_band_supported's
    for bins, cols in ((16384, 1), (16384, 1024), (1048576, 1024), (65536, 600),
                       (8192, 256), (16384, 1025), (16384, 0), (32728, 256), (2097152, 256)):
        want = bool(lib.ro_stft_band_supported(bins, cols))
        assert ro.band_supported(bins, cols) == want
        assert ro.band_supported(bins, cols, ro.RO_PRECISION_F32) == want
        assert ro.band_supported(bins, cols, precision=2) is False
    for bins, cols in ((131072, 1), (131072, 1024), (524288, 218), (1048576, 1024)):
        assert ro.band_supported(bins, cols, ro.RO_PRECISION_F64), (bins, cols)
    for bins, cols in ((65536, 600), (16384, 256), (131072, 1025), (131072, 0), (2097152, 256), (262142, 256)):
        assert not ro.band_supported(bins, cols, ro.RO_PRECISION_F64), (bins, cols)
    assert not ro.band_supported(131072, 256, 2) and not ro.band_supported(131072, 256, -1)
    assert lib.ro_abi_version() == 5                        # additive, like the band-set entries


def test_f64_band_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = str(tmp_path / "ro_band_f64.s")
    r = subprocess.run([hipcc, *BUILD_FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_band_f64.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    entries = re.findall(r"\.name:\s*(\S+)[\s\S]*?\.private_segment_fixed_size:\s*(\d+)", isa)
    # three transform lengths x three sample formats, and the finishing kernel
    assert len([n for n, _ in entries if "band64_slab_kernel" in n]) == 9
    assert len([n for n, _ in entries if "band64_finish_kernel" in n]) == 1
    bad = [(n, int(s)) for n, s in entries if int(s) != 0]
    assert not bad, bad
    # two workgroups share a CU's 160 KiB
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", isa)]
    assert len(lds) == 10 and max(lds) <= 81920
