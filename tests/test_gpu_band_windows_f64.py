"""GPU checks of the band-only transform over several column windows on RO_PRECISION_F64 handles of 131072 bins
(ro_stft_band_windows_resident, csrc/ro_band_f64.hip) against the oracle's rows and against the consecutive call.

The bar is the FP64 mode's own, per bin: |image - the oracle row's columns| <= ONE_ULP x oracle on every bin of every
window -- one float32 ulp, with a 40 dB carrier outside every window in every signal.  With one window the bits are the
consecutive call's.  The scan records are integer / exact work on top of the image: bit-identical to the oracle's scan of
the GPU's own image, the bands moved to image coordinates."""
import numpy as np
import pytest

from util import add_chirp, add_tone, noise_iq

pytestmark = pytest.mark.gpu

ONE_ULP = 2e-7
FS = 48000
BINS, OVERLAP = 131072, 98304        # the smallest size the kernels exist at: 32 slabs
ROWS = 5


def column_freq(bins, col, fs=FS):
    """frequency whose bin is (fractional) column `col` of the fft-shifted row"""
    return (col - bins / 2) * fs / bins


def columns(windows):
    return np.concatenate([np.arange(f, f + n) for f, n in windows])


def offsets(windows):
    return np.concatenate([[0], np.cumsum([n for _, n in windows])]).tolist()


def carrier_column(bins, windows):
    """the middle of the widest run of columns no window covers"""
    edges = [0] + [x for f, n in windows for x in (f, f + n)] + [bins]
    width, lo = max((edges[i + 1] - edges[i], edges[i]) for i in range(0, len(edges), 2))
    assert width > 10000
    return lo + width // 2


def make_signal(seed, samples, bins, windows):
    """sigma = 1 noise + a tone of amplitude 300 outside every window + a tone of amplitude 3 at a non-integer bin inside
    each"""
    iq = noise_iq(np.random.default_rng(seed), samples)
    add_tone(iq, column_freq(bins, carrier_column(bins, windows) + 0.21), 300.0, fs=FS)
    for i, (f, n) in enumerate(windows):
        add_tone(iq, column_freq(bins, f + n // 2 + 0.37), 3.0, fs=FS, phase=0.5 + i)
    return iq


_cache = {}


def case(oracle, seed, rows, windows):
    """(iq, the oracle's full rows [0, rows)) of a seeded signal, computed once per module and left alone"""
    key = (seed, rows, tuple(windows))
    if key not in _cache:
        iq = make_signal(seed, (rows - 1) * (BINS - OVERLAP) + BINS, BINS, windows)
        want = oracle.stft(iq, BINS, OVERLAP, max_rows=rows)
        iq.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (iq, want)
    return _cache[key]


def upload(torch, iq):
    return torch.from_numpy(np.array(iq)).cuda()          # (a copy: the cached signals are read-only)


def run_windows(ro, torch, iq, rows, windows, fmt=None, d_records=None, d_extra=None, **kw):
    d_iq = upload(torch, iq)
    d_band = torch.zeros((rows, sum(n for _, n in windows)), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=BINS, overlap=OVERLAP, precision=ro.RO_PRECISION_F64, **kw) as st:
        st.band_windows_resident(d_iq, ro.RO_IQ_F32 if fmt is None else fmt, iq.shape[0], 0, rows, windows, d_band,
                                 d_records=d_records, d_extra=d_extra)
        torch.cuda.synchronize()
    return d_band.cpu().numpy()


def bin_error(got, full_rows, windows):
    """max over the windows' bins of |image - oracle| / oracle"""
    want = np.asarray(full_rows, dtype=np.float64)[:, columns(windows)]
    assert (want > 0).all()
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / want).max())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


CASES = {
    "M = 256, A = 16": ((40000, 100), (90000, 120)),
    "M = 512, A = 8": ((5000, 150), (70000, 203)),
    "M = 1024, A = 4, row edges, across N/2": ((0, 409), (65300, 515), (BINS - 100, 100)),
    "colliding residues": ((40000, 100), (40000 + 5 * 256, 100)),
    "eight windows": tuple((900 + 15000 * i, 21 + 13 * i) for i in range(8)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_parity(ro, oracle, torch_cuda, name):
    windows = CASES[name]
    assert ro.band_windows_supported(BINS, windows, ro.RO_PRECISION_F64)
    if "colliding" in name:
        k = (columns(windows) + BINS // 2) % BINS
        assert k.size <= 256 and np.unique(k % 256).size < k.size
    iq, want = case(oracle, 500 + len(name), ROWS, windows)
    got = run_windows(ro, torch_cuda, iq, ROWS, windows)
    err = bin_error(got, want, windows)
    print("%s: max per-bin err %.3e" % (name, err))
    assert err <= ONE_ULP, err
    off = offsets(windows)
    for i in range(len(windows)):                           # every window's tone is there
        part = got[:, off[i]:off[i + 1]]
        assert part.max() > 10 * np.median(part), i


@pytest.mark.parametrize("first_col,cols", [(65000, 1024), (40000, 256), (777, 513)])
def test_one_window_is_the_consecutive_call(ro, oracle, torch_cuda, first_col, cols):
    torch = torch_cuda
    iq, _ = case(oracle, 43, ROWS, ((first_col, cols),))
    got = run_windows(ro, torch, iq, ROWS, [(first_col, cols)])
    d_iq = upload(torch, iq)
    d_band = torch.zeros((ROWS, cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=BINS, overlap=OVERLAP, precision=ro.RO_PRECISION_F64) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, ROWS, first_col, cols, d_band)
        torch.cuda.synchronize()
    assert got.any() and same_bits(got, d_band.cpu().numpy())


def test_doubles_pass_un_narrowed(ro, oracle, torch_cuda):
    """true doubles: sigma = 1 noise that no float32 holds, the amplitude-300 carrier outside the windows built in double"""
    windows, rows = CASES["M = 512, A = 8"], ROWS
    samples = (rows - 1) * (BINS - OVERLAP) + BINS
    iq = np.random.default_rng(22).standard_normal((samples, 2))
    ph = 2.0 * np.pi * column_freq(BINS, carrier_column(BINS, windows) + 0.21) * np.arange(samples, dtype=np.float64) / FS
    iq[:, 0] += 300.0 * np.cos(ph)
    iq[:, 1] += 300.0 * np.sin(ph)
    want = oracle.stft(iq, BINS, OVERLAP, max_rows=rows)
    # the test can tell doubles from narrowed doubles: the oracle itself moves by far more than the bar
    narrowed = oracle.stft(iq.astype(np.float32), BINS, OVERLAP, max_rows=rows)
    moved = bin_error(narrowed[:, columns(windows)], want, windows)
    print("oracle on the narrowed samples against the oracle on the doubles: %.3e" % moved)
    assert moved > 10 * ONE_ULP, moved
    got = run_windows(ro, torch_cuda, iq, rows, windows, fmt=ro.RO_IQ_F64)
    err = bin_error(got, want, windows)
    print("doubles: max per-bin err %.3e" % err)
    assert err <= ONE_ULP, err


def image_bands(b, windows):
    """band set b in image coordinates: its noise band and its detect band (margin included) each inside one window"""
    off = offsets(windows)

    def shift(lo, hi):
        hits = [i for i, (f, n) in enumerate(windows) if f <= lo and hi <= f + n]
        assert len(hits) == 1
        return off[hits[0]] - windows[hits[0]][0]

    low_noise = b.low_noise + shift(b.low_noise, b.low_noise + b.noise_width)
    low_detect = b.low_detect + shift(b.low_detect - b.avg_bins // 2,
                                      b.low_detect + b.detect_width - 1 - b.avg_bins // 2 + b.avg_bins)
    return low_noise, b.noise_width, low_detect, b.detect_width, b.avg_bins


def check_records(ro, oracle, got, image, b, windows):
    got = np.ascontiguousarray(got).view(ro.capi.SCAN_DTYPE).reshape(-1)
    n, p, a = oracle.scan_rows(image, *image_bands(b, windows))
    assert np.array_equal(got["peak"], p)
    assert same_bits(got["noise"], n)
    assert same_bits(got["average"], a)
    return p


def test_records_over_two_windows(ro, oracle, torch_cuda):
    """the primary's noise band in the first window and its detect band in the second; the extra set the other way round"""
    torch = torch_cuda
    windows, rows = CASES["M = 512, A = 8"], ROWS
    primary = ro.Bands(low_noise=5020, noise_width=120, low_detect=70040, detect_width=140, avg_bins=27)
    extra = ro.Bands(low_noise=70010, noise_width=190, low_detect=5010, detect_width=130, avg_bins=9)
    iq, _ = case(oracle, 500 + len("M = 512, A = 8"), rows, windows)
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    d_extra = torch.zeros((rows, 1, 3), dtype=torch.float32, device="cuda")
    image = run_windows(ro, torch, iq, rows, windows, d_records=d_recs, d_extra=d_extra, bands=primary, extra_bands=[extra])
    peaks = check_records(ro, oracle, d_recs.cpu().numpy(), image, primary, windows)
    assert set(peaks.tolist()) <= {70101 - 70040, 70102 - 70040}        # the second window's tone, at column 70101.37
    peaks = check_records(ro, oracle, d_extra.cpu().numpy()[:, 0], image, extra, windows)
    assert set(peaks.tolist()) <= {5075 - 5010, 5076 - 5010}            # the first window's, at column 5075.37


def test_scan_peaks_are_the_oracles_own(ro, oracle, torch_cuda):
    """Bolidozor.json's bands at 131072 bins as two windows (the noise band; the detect band with its margin) and a chirp
    through the detect band: the records are the oracle's scan of the image, and the peak is the oracle's own on EVERY
    row -- on the oracle's rows the two largest detect-band values of each row differ by at least 2 % of the larger,
    which one float32 ulp cannot bridge"""
    torch = torch_cuda
    rows, fs = 9, 96000
    hop = BINS - OVERLAP
    ob = oracle.bolid_bands(BINS, fs, OVERLAP, 26450, 26550, 26000, 26300, 5, 2, 40)       # Bolidozor.json:84-93
    bands = ro.Bands(low_noise=ob.low_noise, noise_width=ob.noise_width, low_detect=ob.low_detect,
                     detect_width=ob.detect_width, avg_bins=ob.avg_bins)
    windows = [(w.first_col, w.cols) for w in ro.bands_windows(bands, BINS)]
    assert len(windows) == 2 and windows[0] == (ob.low_noise, ob.noise_width)
    assert sum(n for _, n in windows) < ro.bands_hull(bands, BINS)[1]
    iq = noise_iq(np.random.default_rng(41), (rows - 1) * hop + BINS)
    add_chirp(iq, 0, 10.0, 26540.0, -15.0, 3.0, fs=fs)      # through the detect band (26450 ... 26550 Hz)
    want = oracle.stft(iq, BINS, OVERLAP, max_rows=rows)
    wn, wp, wa = oracle.scan_rows(want, bands.low_noise, bands.noise_width, bands.low_detect, bands.detect_width,
                                  bands.avg_bins)
    det = np.sort(want[:, bands.low_detect:bands.low_detect + bands.detect_width].astype(np.float64), axis=1)
    assert ((det[:, -1] - det[:, -2]) >= 0.02 * det[:, -1]).all()
    assert len(set(wp.tolist())) == rows                    # the chirp moves through the band
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    image = run_windows(ro, torch, iq, rows, windows, d_records=d_recs, bands=bands, sample_rate=fs)
    peaks = check_records(ro, oracle, d_recs.cpu().numpy(), image, bands, windows)
    assert np.array_equal(peaks, wp)                        # all rows, none left out
    assert bin_error(image, want, windows) <= ONE_ULP
