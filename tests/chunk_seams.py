"""The row-chunk seams of the chunked launch paths: the seam arithmetic restated and the case table the CPU and the GPU
test walk (test infrastructure; tests/test_chunk_seams_cpu.py keeps the table tied to the library's constants,
tests/test_gpu_chunk_seams.py runs every case across its seams).

Several transform paths cannot take any number of rows in one grid: the host cuts a call into chunks and advances
first_row, the output pointer and sometimes a scratch block from chunk to chunk.  A SEAM is the last row of a chunk
that is not the call's last: row `seam` comes from one launch and row `seam + 1` from the next.  Each function below
restates one path's rows per chunk from the code it names; the three RO_*_SCRATCH_MB defaults are read from
csrc/ro_host.h's own #ifndef / #define lines, so a case that no longer crosses its seam after somebody changes one
shows up in the CPU test, not as a GPU test that quietly runs as one chunk again.

Every case is a legal call of the ABI: the sample count is exactly what ro_row_count turns into `rows` rows."""
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_HEADER = os.path.join(ROOT, "radio-observer_amd", "csrc", "ro_host.h")

F32, F64 = 0, 1                       # RO_PRECISION_F32, RO_PRECISION_F64 (include/ro_stft.h)
IQ_F32, IQ_I16 = 0, 1                 # RO_IQ_F32, RO_IQ_I16
GRID_ROWS = 65535                     # gridDim.y of a HIP launch; the literal 65535 of every formula below
MIB = 1 << 20


# ---- the library's constants ------------------------------------------------------------------------------------------
def header_defaults(path=None):
    """{name: value} of every `#ifndef NAME` / `#define NAME <integer>` pair of csrc/ro_host.h"""
    text = open(path or HOST_HEADER).read()
    return {name: int(value) for name, value in
            re.findall(r"^#ifndef\s+(RO_\w+)\s*\n#define\s+\1\s+(\d+)\s*$", text, flags=re.M)}


def scratch_mib(name, path=None):
    found = header_defaults(path)
    assert name in found, "%s has no #ifndef / #define default in %s" % (name, path or HOST_HEADER)
    return found[name]


# ---- rows per chunk, path by path -------------------------------------------------------------------------------------
def f64_scratch_rows(bins, path=None):
    """launch_transform_f64 (ro_stft_capi.cpp): scratch_rows_d = max(1, (RO_F64_SCRATCH_MB << 20) / (bins * 16))"""
    return max(1, (scratch_mib("RO_F64_SCRATCH_MB", path) * MIB) // (bins * 16))


def spectra_rows(bins, path=None):
    """ensure_big_scratch (ro_stft_capi.cpp): spec_rows = min(65535, max(1, (RO_SPEC_SCRATCH_MB << 20) / (bins * 8)))"""
    return min(GRID_ROWS, max(1, (scratch_mib("RO_SPEC_SCRATCH_MB", path) * MIB) // (bins * 8)))


def four_rows(bins, path=None):
    """launch_transform, the four-step branch (ro_stft_capi.cpp): limit = max(1, (RO_FOUR_SCRATCH_MB << 20) / (bins * 8));
    the block grows to min(limit, rows) of the call that needs more, so a call of more than `limit` rows runs in chunks
    of `limit`"""
    return max(1, (scratch_mib("RO_FOUR_SCRATCH_MB", path) * MIB) // (bins * 8))


def czt_length(bins):
    """czt_length (ro_czt.cpp): the smallest power of two M >= 512 with M >= 2 bins - 1"""
    m = 512
    while m < 2 * bins - 1:
        m <<= 1
    return m


def czt_rows(bins):
    """launch_transform_czt (ro_czt.cpp): czt_rows = min(65535, max(1, 2^30 / (M * 8))) -- the 1 GiB is a literal there"""
    return min(GRID_ROWS, max(1, (1 << 30) // (czt_length(bins) * 8)))


def band_plan(bins, cols, precision):
    """(m, a, slabs).  float32, band_plan (ro_band.hip): m the smallest of 256 / 512 / 1024 >= cols, a = 8 at m = 1024 and
    16 otherwise, slabs = bins / (m a).  FP64, band64_plan (ro_band_f64.hip): the same m, a = 4096 / m, slabs = bins / 4096."""
    m = 256 if cols <= 256 else 512 if cols <= 512 else 1024
    if precision == F64:
        return m, 4096 // m, bins // 4096
    a = 8 if m == 1024 else 16
    return m, a, bins // (m * a)


def band_rows(bins, cols, precision, rows):
    """run_band (ro_stft_capi.cpp): chunk = min(rows, 65535, max(1, 256 MiB / (slabs * cols * sizeof T))), T = float2 or
    double2 -- the 256 MiB is a literal there; `cols` is the windows' total"""
    slabs = band_plan(bins, cols, precision)[2]
    row_bytes = slabs * cols * (16 if precision == F64 else 8)
    return min(rows, GRID_ROWS, max(1, (256 * MIB) // row_bytes))


# ---- the case table ---------------------------------------------------------------------------------------------------
# path: "rows" (ro_stft_run_resident), "spectra" (ro_stft_spectra_resident), "band" (ro_stft_band_resident),
#       "windows" (ro_stft_band_windows_resident)
# family: which formula above cuts the call; windows: the band's windows ((first_col, cols), ...), one for "band"
# min_seams: the seams the case was written to cross; pad: the long call writes at stride width + 3
# records: the long call also asks for scan records (and the tile / the extra set where the entry point has them)
# rows: enough for a full first chunk and a short last one (two seams where that is cheap); the seams themselves are
# computed, never typed in -- tests/test_gpu_chunk_seams.py's docstring has the device memory of the two large cases
Case = namedtuple("Case", "name path family bins hop rows fmt precision windows min_seams pad records")


def _case(name, path, family, bins, hop, rows, fmt=IQ_F32, precision=F32, windows=(), min_seams=1, pad=False,
          records=False):
    return Case(name, path, family, bins, hop, rows, fmt, precision, tuple(windows), min_seams, pad, records)


ACROSS_HALF = ((523776, 1024),)                         # 1024 columns across N/2 of 1048576 bins
TWO_WIDE = ((100000, 600), (523776 + 300, 424))         # two windows, 1024 columns in all, the second across N/2

CASES = (
    _case("f64 scratch 131072", "rows", "f64", 131072, 512, 131, precision=F64, min_seams=2, pad=True, records=True),
    _case("f64 scratch 1048576", "rows", "f64", 1048576, 4096, 17, precision=F64, min_seams=2),
    _case("spectra 65536", "spectra", "spectra", 65536, 8, 4098, pad=True),
    _case("chirp-z 524286", "rows", "czt", 524286, 2, 130),
    _case("chirp-z 258", "rows", "czt", 258, 1, 65537, pad=True, records=True),
    _case("four-step 1048576", "rows", "four", 1048576, 4096, 130, pad=True),
    _case("four-step 524288", "rows", "four", 524288, 2048, 258, fmt=IQ_I16),
    _case("band 1048576 x 1024", "band", "band", 1048576, 64, 257, windows=ACROSS_HALF, pad=True),
    _case("band 16384 x 5", "band", "band", 16384, 1, 65537, windows=((9000, 5),), records=True),
    _case("windows 16384 x (3 + 2)", "windows", "band", 16384, 1, 65537, windows=((100, 3), (9000, 2)), pad=True,
          records=True),
    _case("windows 1048576 x 1024", "windows", "band", 1048576, 64, 257, windows=TWO_WIDE),
    _case("f64 band 131072 x 5", "band", "band", 131072, 1, 65537, precision=F64, windows=((70000, 5),), pad=True),
    _case("f64 windows 131072 x (3 + 2)", "windows", "band", 131072, 1, 65537, precision=F64,
          windows=((40000, 3), (90000, 2))),
    _case("f64 windows 1048576 x 1024", "windows", "band", 1048576, 4096, 65, precision=F64, windows=TWO_WIDE, pad=True),
)

# the scan bands of the cases with records=True, in row columns (low_noise, noise_width, low_detect, detect_width,
# avg_bins); the band cases' lie inside their windows with the average's margin
BANDS = {
    "f64 scratch 131072": (101034, 410, 101649, 136, 54),          # Bolidozor.json:84-93 at 131072 bins
    "chirp-z 258": (10, 60, 150, 40, 3),
    "band 16384 x 5": (9000, 5, 9001, 3, 3),
    "windows 16384 x (3 + 2)": (100, 3, 101, 1, 3),
}
TILES = {"f64 scratch 131072": (101034, 615), "chirp-z 258": (100, 45)}      # (first_col, cols) of the rows cases' tile
EXTRA = {"windows 16384 x (3 + 2)": ((9000, 2, 9000, 2, 1),)}                # one extra set, in the second window


def by_name(name):
    return next(c for c in CASES if c.name == name)


def names(path=None):
    return [c.name for c in CASES if path is None or c.path == path]


def overlap(c):
    return c.bins - c.hop


def samples(c):
    """what ro_row_count turns into exactly c.rows rows"""
    return c.bins + (c.rows - 1) * c.hop


def cols(c):
    return sum(n for _, n in c.windows)


def width(c):
    """floats (spectra: complex pairs) of one output row"""
    return cols(c) if c.windows else c.bins


def chunk_rows(c, path=None):
    if c.family == "f64":
        return f64_scratch_rows(c.bins, path)
    if c.family == "spectra":
        return spectra_rows(c.bins, path)
    if c.family == "four":
        return four_rows(c.bins, path)
    if c.family == "czt":
        return czt_rows(c.bins)
    if c.family == "band":
        return band_rows(c.bins, cols(c), c.precision, c.rows)
    raise ValueError(c.family)


def seams(c, path=None):
    """the last row of every chunk of the long call but the last"""
    n = chunk_rows(c, path)
    return list(range(n - 1, c.rows - 1, n))


def shards(c, path=None):
    """three uneven shards (first_row, rows), in the order small, large, small.  No cut lies on a seam (between rows
    seam and seam + 1): the cuts are in front of row 3 and in front of the last seam's row, so the last shard computes
    rows seam and seam + 1 in ONE launch where the long call computes them in two, and the large shard is cut by the
    library at other rows than the long call is (its chunks start at row 3)"""
    cut = seams(c, path)[-1]
    return ((0, 3), (3, cut - 3), (cut, c.rows - cut))


def oracle_rows(c, path=None):
    """the rows that go to the oracle: either side of every seam, and the call's last"""
    want = set()
    for s in seams(c, path):
        want.update((s, s + 1))
    want.add(c.rows - 1)
    return sorted(want)
