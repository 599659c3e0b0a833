"""GPU checks of the band-only transform over several column windows (ro_stft_band_windows_resident, float32 handles)
against the oracle's double rows and against the consecutive call.

A column of the band image depends on its bin, on the short transforms' length M and on the slab size A only -- not on
which other columns are asked for -- so wherever two calls share M, the columns they share are equal bit for bit; no
tolerance is involved.  Against the oracle the bar is the float32 bar of the full rows: max |image - oracle row's columns|
over a row <= 1e-5 x the maximum of the FULL oracle row; every signal puts a 40 dB carrier outside every window and a weak
tone inside each.  The scan records are integer / exact work on top of the image: bit-identical to the oracle's scan of the
GPU's own image, the bands moved to image coordinates."""
import numpy as np
import pytest

from util import add_chirp, add_tone, noise_iq

pytestmark = pytest.mark.gpu

BAR = 1e-5
FS = 48000
BINS, OVERLAP = 16384, 12288          # two slabs at M = 1024, four at M = 256, two at M = 512
ROWS = 7


def column_freq(bins, col):
    """frequency whose bin is (fractional) column `col` of the fft-shifted row"""
    return (col - bins / 2) * FS / bins


def columns(windows):
    """row column of every image column"""
    return np.concatenate([np.arange(f, f + n) for f, n in windows])


def offsets(windows):
    return np.concatenate([[0], np.cumsum([n for _, n in windows])]).tolist()


def carrier_column(bins, windows):
    """the middle of the widest run of columns no window covers"""
    edges = [0] + [x for f, n in windows for x in (f, f + n)] + [bins]
    gaps = [(edges[i + 1] - edges[i], edges[i]) for i in range(0, len(edges), 2)]
    width, lo = max(gaps)
    assert width > 400, "no room for the carrier"
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


def case(oracle, seed, bins, overlap, rows, windows):
    """(iq, the oracle's full rows [0, rows)) of a seeded signal, computed once per module and left alone"""
    key = (seed, bins, overlap, rows, tuple(windows))
    if key not in _cache:
        iq = make_signal(seed, (rows - 1) * (bins - overlap) + bins, bins, windows)
        want = oracle.stft(iq, bins, overlap, max_rows=rows)
        iq.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (iq, want)
    return _cache[key]


def upload(torch, iq):
    return torch.from_numpy(np.array(iq)).cuda()          # (a copy: the cached signals are read-only)


def run_windows(ro, torch, iq, bins, overlap, rows, windows, fmt=None, **kw):
    d_iq = upload(torch, iq)
    total = sum(n for _, n in windows)
    d_band = torch.zeros((rows, total), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, **kw) as st:
        st.band_windows_resident(d_iq, ro.RO_IQ_F32 if fmt is None else fmt, iq.shape[0], 0, rows, windows, d_band)
        torch.cuda.synchronize()
    return d_band.cpu().numpy()


def run_band(ro, torch, iq, bins, overlap, rows, first_col, cols, **kw):
    d_iq = upload(torch, iq)
    d_band = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, **kw) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, d_band)
        torch.cuda.synchronize()
    return d_band.cpu().numpy()


def image_error(got, full_rows, windows):
    """max over rows of max |image - the oracle's columns| / max of the FULL oracle row"""
    want = np.asarray(full_rows, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want[:, columns(windows)]).max(axis=1)
    return float((err / want.max(axis=1)).max())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def tones_present(got, windows):
    off = offsets(windows)
    for i, (_, n) in enumerate(windows):
        part = got[:, off[i]:off[i + 1]]
        assert n < 8 or part.max() > 10 * np.median(part), "window %d holds no tone" % i


TWO = ((3000, 300), (9000, 400))
CASES = {
    "two windows, M = 1024": TWO,
    "colliding residues, M = 256": ((1000, 100), (1000 + 5 * 256, 100)),
    "row edges, M = 512": ((0, 150), (BINS - 170, 170)),
    "across N/2 next to another": ((8100, 200), (9000, 100)),
    "eight windows": tuple((700 + 1900 * i, 100 + 7 * i) for i in range(8)),
    "touching windows, 1024 in all": ((5000, 512), (5512, 512)),
    "one column each": ((4000, 1), (4002, 1), (12000, 1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_parity(ro, oracle, torch_cuda, name):
    windows = CASES[name]
    assert ro.band_windows_supported(BINS, windows)
    if "colliding" in name:
        k = (columns(windows) + BINS // 2) % BINS
        assert k.size <= 256 and np.unique(k % 256).size < k.size
    iq, want = case(oracle, 300 + len(name), BINS, OVERLAP, ROWS, windows)
    got = run_windows(ro, torch_cuda, iq, BINS, OVERLAP, ROWS, windows)
    err = image_error(got, want, windows)
    print("%s: max err / full row max %.3e" % (name, err))
    assert err <= BAR, err
    tones_present(got, windows)


@pytest.mark.parametrize("first_col,cols", [(3000, 300), (8000, 1024), (16127, 257)])
def test_one_window_is_the_consecutive_call(ro, oracle, torch_cuda, first_col, cols):
    iq, _ = case(oracle, 41, BINS, OVERLAP, ROWS, ((first_col, cols),))
    got = run_windows(ro, torch_cuda, iq, BINS, OVERLAP, ROWS, [ro.BandWindow(first_col, cols)])
    assert got.any() and same_bits(got, run_band(ro, torch_cuda, iq, BINS, OVERLAP, ROWS, first_col, cols))


def test_each_window_has_the_bits_of_a_band_that_contains_it(ro, oracle, torch_cuda):
    """700 columns in two windows and 600 consecutive columns both run on M = 1024"""
    iq, _ = case(oracle, 300 + len("two windows, M = 1024"), BINS, OVERLAP, ROWS, TWO)
    got = run_windows(ro, torch_cuda, iq, BINS, OVERLAP, ROWS, TWO)
    off = offsets(TWO)
    for i, (first, n) in enumerate(TWO):
        band_first = first - 100 - 50 * i
        band = run_band(ro, torch_cuda, iq, BINS, OVERLAP, ROWS, band_first, 600)
        assert same_bits(got[:, off[i]:off[i + 1]], band[:, first - band_first:first - band_first + n]), i


@pytest.mark.parametrize("rows", [1, ROWS])
def test_layout(ro, oracle, torch_cuda, rows):
    torch = torch_cuda
    total = sum(n for _, n in TWO)
    stride = total + 13
    iq, want = case(oracle, 300 + len("two windows, M = 1024"), BINS, OVERLAP, ROWS, TWO)
    d_iq = upload(torch, iq)
    sentinel = -777.25
    a = torch.full((rows + 1, stride), sentinel, dtype=torch.float32, device="cuda")       # + a guard row
    b = torch.full((rows + 1, stride), sentinel, dtype=torch.float32, device="cuda")
    with ro.Stft(bins=BINS, overlap=OVERLAP) as st:
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, TWO, a, band_stride=stride)
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, TWO, b, band_stride=stride)
        torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert (a[:rows, total:] == sentinel).all(), "floats beyond the total were written"
    assert (a[rows] == sentinel).all(), "the row after the last one was written"
    assert image_error(a[:rows, :total], want[:rows], TWO) <= BAR
    assert same_bits(a, b), "two launches differ"
    assert same_bits(a[:rows, :total], run_windows(ro, torch, iq, BINS, OVERLAP, rows, TWO))


@pytest.mark.parametrize("option", ["i16", "gain"])
def test_formats_and_options(ro, oracle, torch_cuda, option):
    windows, rows = CASES["colliding residues, M = 256"], 5
    iq = make_signal(21, (rows - 1) * (BINS - OVERLAP) + BINS, BINS, windows)
    kw, fmt, gain, send = {}, ro.RO_IQ_F32, 0.0, iq
    if option == "i16":
        send = np.clip(np.rint(iq * 64.0), -32768, 32767).astype(np.int16)       # un-normalised, like WAVStream
        iq = send.astype(np.float32)
        fmt = ro.RO_IQ_I16
    else:
        gain = 0.25
        kw["iq_gain"] = gain
    want = oracle.stft(iq, BINS, OVERLAP, gain=gain, max_rows=rows)
    got = run_windows(ro, torch_cuda, send, BINS, OVERLAP, rows, windows, fmt=fmt, **kw)
    err = image_error(got, want, windows)
    print("%s: max err / full row max %.3e" % (option, err))
    assert err <= BAR, err


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
    got = got.view(ro.capi.SCAN_DTYPE).reshape(-1)
    n, p, a = oracle.scan_rows(image, *image_bands(b, windows))
    assert np.array_equal(got["peak"], p)
    assert same_bits(got["noise"], n)
    assert same_bits(got["average"], a)
    return p


def test_records_over_two_windows(ro, oracle, torch_cuda):
    """the primary's noise band in the first window and its detect band in the second; one extra set the other way round,
    one with both in the second window"""
    torch = torch_cuda
    windows, rows = TWO, ROWS
    primary = ro.Bands(low_noise=3040, noise_width=200, low_detect=9150, detect_width=120, avg_bins=9)
    extras = [ro.Bands(low_noise=9010, noise_width=100, low_detect=3004, detect_width=290, avg_bins=9),
              ro.Bands(low_noise=9300, noise_width=100, low_detect=9020, detect_width=60, avg_bins=27)]
    iq, _ = case(oracle, 300 + len("two windows, M = 1024"), BINS, OVERLAP, rows, windows)
    d_iq = upload(torch, iq)
    total = sum(n for _, n in windows)
    d_band = torch.zeros((rows, total), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    d_extra = torch.zeros((rows, len(extras), 3), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=BINS, overlap=OVERLAP, bands=primary, extra_bands=extras) as st:
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, windows, d_band, d_records=d_recs,
                                 d_extra=d_extra)
        torch.cuda.synchronize()
    image = d_band.cpu().numpy()
    peaks = check_records(ro, oracle, d_recs.cpu().numpy(), image, primary, windows)
    assert set(peaks.tolist()) <= {9200 - 9150, 9201 - 9150}      # the second window's tone, at column 9200.37
    ext = d_extra.cpu().numpy()
    for s, b in enumerate(extras):
        check_records(ro, oracle, np.ascontiguousarray(ext[:, s]), image, b, windows)
    # the first extra set's detect band holds the first window's tone (column 3150.37): that is its peak on every row
    first = np.ascontiguousarray(ext[:, 0]).view(ro.capi.SCAN_DTYPE).reshape(-1)
    assert set(first["peak"].tolist()) <= {3150 - 3004, 3151 - 3004}


def test_records_equal_the_consecutive_calls_where_the_hull_fits(ro, oracle, torch_cuda):
    """windows [2000,+300) and [2500,+300) (600 columns) and their hull [2000,+800) both run on M = 1024"""
    torch = torch_cuda
    windows, rows = ((2000, 300), (2500, 300)), ROWS
    bands = ro.Bands(low_noise=2010, noise_width=280, low_detect=2520, detect_width=260, avg_bins=27)
    first_col, cols = ro.bands_hull(bands, BINS)
    assert first_col >= 2000 and first_col + cols <= 2800 and len(ro.bands_windows(bands, BINS)) == 2
    iq, _ = case(oracle, 77, BINS, OVERLAP, rows, windows)
    d_iq = upload(torch, iq)
    d_win = torch.zeros((rows, 600), dtype=torch.float32, device="cuda")
    d_hull = torch.zeros((rows, 800), dtype=torch.float32, device="cuda")
    r_win = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    r_hull = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=BINS, overlap=OVERLAP, bands=bands) as st:
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, windows, d_win, d_records=r_win)
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, 2000, 800, d_hull, d_records=r_hull)
        torch.cuda.synchronize()
    win, hull = d_win.cpu().numpy(), d_hull.cpu().numpy()
    assert same_bits(win[:, :300], hull[:, :300]) and same_bits(win[:, 300:], hull[:, 500:])
    a = r_win.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1)
    b = r_hull.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1)
    assert np.array_equal(a["peak"], b["peak"]) and same_bits(a["noise"], b["noise"]) and same_bits(a["average"], b["average"])
    check_records(ro, oracle, r_win.cpu().numpy(), win, bands, windows)


def test_radio_observer_json(ro, oracle, torch_cuda):
    """32768 / 24576 with the windows of radio-observer.json: the noise band, and the detect band with the snapshot's
    columns -- 1365 columns as one range, which the consecutive call refuses"""
    torch = torch_cuda
    bins, overlap, rows = 32768, 24576, 9
    hop = bins - overlap
    ob = oracle.bolid_bands(bins, FS, overlap, 10300, 10900, 9000, 9600, 2, 5, 40)
    bands = ro.Bands(low_noise=ob.low_noise, noise_width=ob.noise_width, low_detect=ob.low_detect,
                     detect_width=ob.detect_width, avg_bins=ob.avg_bins)
    t0, t1 = ro.frequency_to_bin(bins, FS, 10100.0), ro.frequency_to_bin(bins, FS, 11000.0)
    tile = (t0, t1 - t0)
    windows = [(w.first_col, w.cols) for w in ro.bands_windows(bands, bins, *tile)]
    assert len(windows) == 2 and ro.band_windows_supported(bins, windows)
    assert not ro.band_supported(bins, ro.bands_hull(bands, bins, *tile)[1])
    total = sum(n for _, n in windows)
    iq = noise_iq(np.random.default_rng(41), (rows - 1) * hop + bins)
    add_tone(iq, column_freq(bins, carrier_column(bins, windows) + 0.21), 300.0, fs=FS)
    # a chirp through the detect band (10300 ... 10900 Hz): 10850 Hz falling 15 Hz/s over the 2 s of the stream
    add_chirp(iq, 0, 10.0, 10850.0, -15.0, 3.0, fs=FS)
    d_iq = upload(torch, iq)
    d_band = torch.zeros((rows, total), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, bands=bands) as st:
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, windows, d_band, d_records=d_recs)
        with pytest.raises(ro.StftError) as e:
            first_col, cols = ro.bands_hull(bands, bins, *tile)
            st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, d_band)
        assert e.value.code == -2
        torch.cuda.synchronize()
    image = d_band.cpu().numpy()
    want = oracle.stft(iq, bins, overlap, max_rows=rows)
    err = image_error(image, want, windows)
    # the tile's columns, cut from the second window
    at = offsets(windows)[1] + tile[0] - windows[1][0]
    tile_err = image_error(image[:, at:at + tile[1]], want, [tile])
    print("radio-observer.json windows %s: max err / full row max %.3e (tile %.3e)" % (windows, err, tile_err))
    assert tile_err <= BAR and err <= BAR
    peaks = check_records(ro, oracle, d_recs.cpu().numpy(), image, bands, windows)
    assert len(set(peaks.tolist())) > 3                     # the chirp moves through the band


def test_refusals(ro, torch_cuda):
    torch = torch_cuda
    bins, overlap = BINS, OVERLAP
    samples = 4 * (bins - overlap) + bins                   # five rows
    d_iq = torch.zeros((samples, 2), dtype=torch.float32, device="cuda")
    sentinel = 5.5
    d_band = torch.full((5, 1100), sentinel, dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((5, 3), dtype=torch.float32, device="cuda")
    d_extra = torch.zeros((5, 2, 3), dtype=torch.float32, device="cuda")
    good = [(2000, 110), (2190, 80)]

    def refused(st, code, word, first_row, rows, windows, fmt=None, **kw):
        with pytest.raises(ro.StftError) as e:
            st.band_windows_resident(d_iq, ro.RO_IQ_F32 if fmt is None else fmt, samples, first_row, rows, windows, d_band,
                                     **kw)
        assert e.value.code == code, str(e.value)
        text = (ro.library().ro_last_error() or b"").decode()
        assert word in text, text

    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        refused(st, -2, "RO_PRECISION_F64", 0, 5, good)
    with ro.Stft(bins=32728, overlap=0) as st:
        refused(st, -2, "power-of-two", 0, 1, good)
    # noise [2000,+100), detect with the margin [2196,2254)
    bands = ro.Bands(low_noise=2000, noise_width=100, low_detect=2200, detect_width=50, avg_bins=9)
    with ro.Stft(bins=bins, overlap=overlap, bands=bands) as st:
        refused(st, -1, "1 ... 8 windows", 0, 5, [])
        refused(st, -1, "1 ... 8 windows", 0, 5, [(100 * i, 10) for i in range(9)])
        refused(st, -1, "at least one column", 0, 5, [(100, 10), (200, 0)])
        refused(st, -1, "outside the row", 0, 5, [(100, 10), (bins - 9, 10)])
        refused(st, -1, "outside the row", 0, 5, [(-1, 10)])
        refused(st, -1, "must not overlap", 0, 5, [(100, 100), (199, 10)])
        refused(st, -1, "ascending", 0, 5, [(5000, 100), (100, 10)])
        refused(st, -2, "1025", 0, 5, [(100, 512), (700, 513)])
        refused(st, -1, "band_stride", 0, 5, good, band_stride=189)
        refused(st, -1, "samples", 1, 5, good)
        refused(st, -1, "negative", 0, -1, good)
        refused(st, -2, "RO_IQ_F32 or RO_IQ_I16", 0, 5, good, fmt=ro.RO_IQ_F64)
        refused(st, -1, "set 0 need its noise band, columns [2000,2100)", 0, 5, [(2001, 110), (2190, 80)], d_records=d_recs)
        refused(st, -1, "set 0 need its detect band and the average's margin, columns [2196,2254)", 0, 5,
                [(2000, 110), (2190, 63)], d_records=d_recs)
        # (the two together hold the detect band, but no one window does)
        refused(st, -1, "set 0 need its detect band", 0, 5, [(2000, 100), (2190, 30), (2220, 80)], d_records=d_recs)
        refused(st, -5, "no extra band sets", 0, 5, good, d_extra=d_extra)
        st.set_extra_bands([ro.Bands(low_noise=2200, noise_width=60, low_detect=2010, detect_width=80, avg_bins=9),
                            ro.Bands(low_noise=4000, noise_width=60, low_detect=2010, detect_width=80, avg_bins=9)])
        refused(st, -1, "set 2 need its noise band, columns [4000,4060)", 0, 5, good, d_records=d_recs, d_extra=d_extra)
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, samples, 0, 0, good, d_band)            # rows = 0: RO_OK, nothing touched
        st.band_windows_resident(None, ro.RO_IQ_F32, 0, 7, 0, good, None)
        torch.cuda.synchronize()
        assert (d_band == sentinel).all().item()
        assert ro.library().ro_stft_band_windows_resident(st._h, None, ro.RO_IQ_F32, 0, 0, 0, None, 1, None, 0, None, None,
                                                          None) == -1
        # ... and the windows that do hold the sets go through, records and all
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, samples, 0, 5, good + [(3990, 80)], d_band, band_stride=1100,
                                 d_records=d_recs, d_extra=d_extra)
        torch.cuda.synchronize()
        # (the samples are zeros: every magnitude is exactly 0)
        assert (d_band[:, :270] == 0.0).all().item() and (d_band[:, 270:] == sentinel).all().item()
    with ro.Stft(bins=bins, overlap=overlap) as st:                                        # no bands configured
        refused(st, -1, "enable_scan", 0, 5, good, d_records=d_recs)
