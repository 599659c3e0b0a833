"""The band scan at the row's edges: two references and the case tables the CPU and the GPU test walk (test
infrastructure; tests/test_scan_edges_cpu.py pins the references to each other, tests/test_gpu_scan_edges.py judges
the kernels with them).

A band set is the tuple (low_noise, noise_width, low_detect, detect_width, avg_bins) of tests/test_gpu_scan_sets.py.

No NaN and no -0.0 inside a band anywhere in these tables: neither the oracle's comparator nor numpy's sort defines an
order the other shares for them, and a row of magnitudes cannot hold -0.0."""
import numpy as np

from util import add_tone, noise_iq

FLT_MAX = np.float32(np.finfo(np.float32).max)
SCAN_DTYPE = np.dtype([("noise", np.float32), ("peak", np.int32), ("average", np.float32)])
FS = 48000


# ---- the two references ----------------------------------------------------------------------------------------------
def scan_reference(rows, bands, bins, wrap=False):
    """BolidRecorder::noise / peak / average (src/BolidRecorder.cpp:121-132, :313-347) in numpy: float64 and integer
    arithmetic, one narrowing per result.  average(): columns outside [0, bins) contribute 0 and the sum is divided by
    avg_bins all the same.  `wrap` is for the fixtures' own sanity check only: it reads those columns from the other
    end of the row instead, which is what a missing guard on an LDS image would do."""
    low_noise, noise_width, low_detect, detect_width, avg_bins = bands
    rows = np.asarray(rows, dtype=np.float32)
    assert rows.ndim == 2 and rows.shape[1] == bins
    out = np.zeros(rows.shape[0], SCAN_DTYPE)
    for r in range(rows.shape[0]):
        row = rows[r]
        quartile = np.sort(row[low_noise:low_noise + noise_width])[noise_width // 4]
        with np.errstate(over="ignore"):
            out["noise"][r] = np.float32(np.float64(quartile) * 2)
        band = row[low_detect:low_detect + detect_width]
        peak = detect_width - 1 - int(np.argmax(band[::-1]))          # the LAST index of the maximum
        start = low_detect + peak - avg_bins // 2
        acc = np.float64(0.0)
        for c in range(start, start + avg_bins):
            if wrap:
                acc += np.float64(row[c % bins])
            elif 0 <= c < bins:
                acc += np.float64(row[c])
        out["peak"][r] = peak
        with np.errstate(over="ignore"):
            out["average"][r] = np.float32(acc / np.float64(avg_bins))
    return out


def oracle_padded(oracle, rows, bands):
    """the project's oracle on rows padded with avg_bins zeros on both sides, the bands moved by the padding: it answers
    the clipped window without reading out of bounds"""
    low_noise, noise_width, low_detect, detect_width, avg_bins = bands
    rows = np.asarray(rows, dtype=np.float32)
    padded = np.zeros((rows.shape[0], rows.shape[1] + 2 * avg_bins), np.float32)
    padded[:, avg_bins:avg_bins + rows.shape[1]] = rows
    n, p, a = oracle.scan_rows(padded, low_noise + avg_bins, noise_width, low_detect + avg_bins, detect_width, avg_bins)
    out = np.zeros(rows.shape[0], SCAN_DTYPE)
    out["noise"], out["peak"], out["average"] = n, p, a
    return out


def oracle_plain(oracle, rows, bands):
    n, p, a = oracle.scan_rows(np.asarray(rows, dtype=np.float32), *bands)
    out = np.zeros(len(n), SCAN_DTYPE)
    out["noise"], out["peak"], out["average"] = n, p, a
    return out


def window_inside(bands, bins):
    """the averaging window stays in the row whatever the peak"""
    return bands[2] >= bands[4] // 2 and bands[2] + bands[3] - 1 - bands[4] // 2 + bands[4] <= bins


def window_leaves(rows, bands, bins):
    """per row: whether average()'s window leaves [0, bins) for the peak this row has"""
    start = bands[2] + scan_reference(rows, bands, bins)["peak"].astype(np.int64) - bands[4] // 2
    return (start < 0) | (start + bands[4] > bins)


def same_bits(got, want):
    return all(np.array_equal(np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32))
               for f in ("noise", "peak", "average"))


def describe(got, want):
    """the records that differ, for an assertion's message"""
    bad = [r for r in range(len(want)) if not same_bits(got[r:r + 1], want[r:r + 1])]
    return "; ".join("row %d got %s want %s" % (r, got[r], want[r]) for r in bad[:4])


# ---- A: the window leaves the row, rows in HBM ---------------------------------------------------------------------
A_SMALL_BINS = 256
A_SMALL_AVG = (1, 2, 3, 27, 64, 65, 129, 255)
A_SMALL_MAXIMA = (0, 1, 127, 254, 255)
A_LARGE_BINS = 16384
A_LARGE_WIDTHS = (16384, 1024, 1025, 4096, 4097, 8192, 8193)
A_LARGE_AVG = 101
A_STRIDE_EXTRA = 37

_rows_cache = {}


def a_small_rows():
    """6 rows of 256: the maximum forced to column 0, 1, 127, 254, 255; the last row has equal maxima at 0 and 255"""
    if "a_small" not in _rows_cache:
        rows = (np.abs(np.random.default_rng(0xA1).standard_normal((6, A_SMALL_BINS))) + 0.25).astype(np.float32)
        for r, c in enumerate(A_SMALL_MAXIMA):
            rows[r, c] = 50.0
        rows[5, 0] = rows[5, 255] = 50.0
        rows.setflags(write=False)
        _rows_cache["a_small"] = rows
    return _rows_cache["a_small"]


def a_large_rows():
    """3 rows of 16384: the maximum at column 0, at column 16383, at both"""
    if "a_large" not in _rows_cache:
        rows = (np.abs(np.random.default_rng(0xA2).standard_normal((3, A_LARGE_BINS))) + 0.25).astype(np.float32)
        rows[0, 0] = rows[1, A_LARGE_BINS - 1] = rows[2, 0] = rows[2, A_LARGE_BINS - 1] = 50.0
        rows.setflags(write=False)
        _rows_cache["a_large"] = rows
    return _rows_cache["a_large"]


def hbm_window_cases():
    """[(name, rows, bands)]"""
    cases = []
    for avg in A_SMALL_AVG:
        cases.append(("256 whole row avg %d" % avg, a_small_rows(), (3, 100, 0, 256, avg)))
    for low in (0, 255):
        for avg in (2, 27):
            cases.append(("256 detect [%d,+1) avg %d" % (low, avg), a_small_rows(), (low, 1, low, 1, avg)))
    for w in A_LARGE_WIDTHS:
        for low in sorted({0, A_LARGE_BINS - w}):
            cases.append(("16384 bands [%d,+%d) avg %d" % (low, w, A_LARGE_AVG), a_large_rows(), (low, w, low, w, A_LARGE_AVG)))
    return cases


# ---- B: values at float32's edges --------------------------------------------------------------------------------
B_BINS = 16384
B_WIDTHS = (5, 64, 409, 1024, 1025, 4097)
B_LOW = 5003
B_AVG = 9
B_ROWS = 4
B_FIXTURES = ("denormal", "mixed", "low_byte", "bit8", "flt_max", "inf")
B_ORACLE_SORTS = ("denormal", "mixed", "low_byte", "bit8", "flt_max")      # inf - inf is NaN in the oracle's comparator


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def float_edge_band(name, width, rng):
    """one band of `width` values of fixture `name`"""
    if name == "denormal":                       # distinct positive denormals only
        return _bits(rng.choice(0x7fffff, size=width, replace=False) + 1)
    if name == "mixed":                          # denormals and normal numbers, both signs
        u = (rng.choice(0x7fffff, size=width, replace=False) + 1).astype(np.uint32)
        normal = rng.random(width) < 0.5
        u[normal] += np.uint32(0x3f000000)       # [0.5, 1): distinct mantissas stay distinct
        u[rng.random(width) < 0.5] |= np.uint32(0x80000000)
        return _bits(u)
    if name == "low_byte":                       # 1 + k 2^-23, k a permutation of 0 ... 255, repeated
        k = np.resize(rng.permutation(256), width).astype(np.uint32)
        return _bits(np.uint32(0x3f800000) + k)
    if name == "bit8":                           # 1 + k 2^-23, k < 512, bit 8 set in some and clear in others
        k = np.resize(rng.permutation(512), width).astype(np.uint32)
        k[0] &= np.uint32(0xff)
        k[1 % width] |= np.uint32(0x100)
        return _bits(np.uint32(0x3f800000) + k)
    raise ValueError(name)


def float_edge_rows(name, width):
    """[B_ROWS, B_BINS] rows whose band [B_LOW, +width) is fixture `name`; ordinary positive values around it"""
    key = (name, width)
    if key not in _rows_cache:
        rng = np.random.default_rng([B_FIXTURES.index(name), width])
        rows = (np.abs(rng.standard_normal((B_ROWS, B_BINS))) + 0.25).astype(np.float32)
        for r in range(B_ROWS):
            if name == "flt_max":
                if r < 2:      # a few FLT_MAX among values above FLT_MAX / 2: the quartile doubles to +inf
                    band = rng.uniform(1.8e38, 3.3e38, width).astype(np.float32)
                    band[rng.choice(width, size=min(3, width), replace=False)] = FLT_MAX
                else:          # the quartile itself is FLT_MAX: at most width / 4 smaller values
                    band = np.full(width, FLT_MAX, np.float32)
                    small = min(width // 4, 3)
                    band[rng.choice(width, size=small, replace=False)] = rng.uniform(1.0, 2.0, small).astype(np.float32)
            elif name == "inf":
                band = (np.abs(rng.standard_normal(width)) + 0.25).astype(np.float32)
                count = 1 if r < 2 else min(3, width - 2)              # one +inf; several: ties at infinity go to the last
                band[rng.choice(width, size=count, replace=False)] = np.inf
            else:
                band = float_edge_band(name, width, rng)
            rows[r, B_LOW:B_LOW + width] = band
        rows.setflags(write=False)
        _rows_cache[key] = rows
    return _rows_cache[key]


def float_edge_cases():
    """[(name, fixture, rows, bands)]: noise band = detect band = the fixture's band; the window stays in the row"""
    return [("%s width %d" % (fx, w), fx, float_edge_rows(fx, w), (B_LOW, w, B_LOW, w, B_AVG))
            for fx in B_FIXTURES for w in B_WIDTHS]


# ---- C: the fused epilogue's own forms, through the transform -------------------------------------------------------
C_ROWS = 8
C_SHAPES = ((32768, 24576), (4096, 2048))        # the fused epilogue; the control, whose primary route is scan_kernel
C_NOISE_WIDTHS = (1, 2, 3, 4, 5, 511, 512, 513, 1024, 1025, 32768)
C_DETECT_WIDTHS = (1, 63, 64, 65, 511, 512, 513, 1025, 32768)
C_AVG = (1, 2, 27, 63, 64, 65, 129)
TONE_AMP = 20.0


def column_freq(bins, col):
    """column c of the fft-shifted row is frequency (c - N/2) fs / N: column 0 is -fs/2, column N/2 is DC"""
    return (col - bins // 2) * FS / bins


def json_like(bins):
    """radio-observer.json's bands (22528 / 409 / 23415 / 410 / 27 at 32768 bins), their columns scaled to the row"""
    return (22528 * bins // 32768, 409, 23415 * bins // 32768, 410, 27)


def interior_tone(bins):
    return json_like(bins)[2] + 205


def tone_signal(bins, overlap, tones):
    """noise_iq plus an on-bin tone of amplitude 20 at every column of `tones`, C_ROWS rows long"""
    key = ("sig", bins, overlap, tuple(tones))
    if key not in _rows_cache:
        iq = noise_iq(np.random.default_rng([0xC0, bins]), bins + (C_ROWS - 1) * (bins - overlap))
        for c in tones:
            add_tone(iq, column_freq(bins, c), TONE_AMP, fs=FS)
        iq.setflags(write=False)
        _rows_cache[key] = iq
    return _rows_cache[key]


def epilogue_cases(bins):
    """[(name, bands, tones)]: `tones` are the columns that carry a tone; the one inside the detect band is its maximum.
    With both edge tones the maximum is within one column of either: columns 0 and N - 1 are neighbours on the
    frequency circle, the two main lobes of the window overlap and beat from row to row (tone_slack)."""
    N = bins
    jn, jnw, jd, jdw, javg = json_like(N)
    T = interior_tone(N)
    cases = []
    for w in C_NOISE_WIDTHS:
        w = min(w, N)
        cases.append(("noise width %d" % w, (min(jn, N - w), w, T - 2, 5, 3), (T,)))
    for w in C_DETECT_WIDTHS:
        w = min(w, N)
        cases.append(("detect width %d" % w, (jn, jnw, min(max(T - w // 2, 0), N - w), w, javg), (T,)))
    for avg in C_AVG:
        cases.append(("avg_bins %d" % avg, (jn, jnw, jd, jdw, avg), (T,)))
    cases += [
        ("noise band across N/2", (N // 2 - 200, 409, jd, jdw, javg), (T,)),
        ("noise band from column 0", (0, 409, jd, jdw, javg), (T,)),
        ("noise band to column N", (N - 409, 409, jd, jdw, javg), (T,)),
        ("detect band [N/2 - 1, +2), DC tone", (jn, jnw, N // 2 - 1, 2, javg), (N // 2,)),
        ("detect band from column 0, window clipped left", (jn, jnw, 0, 410, 27), (0,)),
        ("detect band to column N, window clipped right", (jn, jnw, N - 410, 410, 27), (N - 1,)),
        ("whole row, both edge tones", (jn, jnw, 0, N, 27), (0, N - 1)),
        ("whole row, both edge tones, avg 129", (0, N, 0, N, 129), (0, N - 1)),
    ]
    return cases


def tone_slack(tones):
    return 1 if len(tones) > 1 else 0


def peaks_on_tones(rows, bands, tones):
    """the fixture's own check: every row's last maximum of the detect band sits on a tone meant for that band"""
    peak = bands[2] + scan_reference(rows, bands, rows.shape[1])["peak"].astype(np.int64)
    inside = [c for c in tones if bands[2] <= c < bands[2] + bands[3]]
    return bool(inside) and all(min(abs(int(p) - c) for c in inside) <= tone_slack(tones) for p in peak)


# ---- D: the epilogue's tile cut ---------------------------------------------------------------------------------
D_BINS, D_OVERLAP = 32768, 24576
D_TILES = ((16384 - 100, 200), (16383, 1), (16384, 1), (0, 1), (32767, 1), (0, 63), (5, 64), (7, 65), (100, 127),
           (100, 128), (100, 129), (32768 - 615, 615), (0, 32768))
D_TONES = (0, 16384, interior_tone(32768), 32767)


# ---- E: silence ----------------------------------------------------------------------------------------------------
# (bins, overlap, rows): every float32 family, the last one chirp-z
E_SHAPES = ((256, 128, 5), (4096, 2048, 5), (16384, 12288, 3), (32768, 24576, 8), (65536, 49152, 2), (262144, 0, 2),
            (1000, 0, 3))
E_BAND = (16384, 12288, 3, 9000, 600)            # ro_stft_band_resident: bins, overlap, rows, first_col, cols
E_BAND_BANDS = (9010, 100, 9200, 200, 5)         # ... and bands that lie in those columns with the average's margin


def silence_bands(bins):
    """(bands, tile) for a row of `bins` zeros: every size has room for them"""
    return (bins // 8, bins // 16, bins // 2 + 3, bins // 10, 5), (bins // 2 - 20, 45)
