"""GPU parity of the band-only transform (ro_stft_band_resident, csrc/ro_band.hip) against the oracle's double rows.

The bar is the float32 bar of the full rows applied to a band: max |band - oracle_row[first_col : first_col + cols]| over a
row <= 1e-5 x the maximum of the FULL oracle row (rounding noise scales with the whole row's energy, and every signal
here puts a 40 dB carrier outside the band to make that count).  The scan records are integer / exact work on top of
the band image: bit-identical to the oracle's scan of that image."""
import numpy as np
import pytest

from util import add_chirp, add_tone, noise_iq

pytestmark = pytest.mark.gpu

BAR = 1e-5
FS = 48000


def column_freq(bins, col):
    """frequency whose bin is (fractional) column `col` of the fft-shifted row"""
    return (col - bins / 2) * FS / bins


def make_signal(seed, samples, bins, first_col, cols):
    """sigma = 1 noise + a tone of amplitude 300 some 5000 columns OUTSIDE the band + a tone of amplitude 3 at a non-integer
    bin inside it"""
    iq = noise_iq(np.random.default_rng(seed), samples)
    outside = first_col + cols + 5000 if first_col + cols + 5000 < bins else first_col - 5000
    assert 0 <= outside < bins
    add_tone(iq, column_freq(bins, outside + 0.21), 300.0, fs=FS)
    add_tone(iq, column_freq(bins, first_col + cols // 2 + 0.37), 3.0, fs=FS, phase=0.5)
    return iq


def band_error(got, full_rows, first_col, cols):
    """max over rows of max |band - oracle band| / max of the FULL oracle row"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(full_rows, dtype=np.float64)
    err = np.abs(got - want[:, first_col:first_col + cols]).max(axis=1)
    return float((err / want.max(axis=1)).max())


def run_band(ro, torch, iq, bins, overlap, first_row, rows, first_col, cols, fmt=None, stride=None, **kw):
    fmt = ro.RO_IQ_F32 if fmt is None else fmt
    d_iq = torch.from_numpy(iq).cuda()
    d_band = torch.zeros((rows, stride or cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, **kw) as st:
        st.band_resident(d_iq, fmt, iq.shape[0], first_row, rows, first_col, cols, d_band, band_stride=stride)
        torch.cuda.synchronize()
    return d_band.cpu().numpy()


_cache = {}


def case(oracle, seed, bins, overlap, first_row, rows, first_col, cols):
    """(iq, the oracle's full rows [first_row, +rows)) of a seeded signal, computed once per module"""
    key = (seed, bins, overlap, first_row, rows, first_col, cols)
    if key not in _cache:
        hop = bins - overlap
        iq = make_signal(seed, (first_row + rows - 1) * hop + bins, bins, first_col, cols)
        _cache[key] = (iq, oracle.stft(iq, bins, overlap, first_row=first_row, max_rows=rows))
    return _cache[key]


def check_parity(ro, oracle, torch, seed, bins, overlap, first_row, rows, first_col, cols):
    iq, want = case(oracle, seed, bins, overlap, first_row, rows, first_col, cols)
    got = run_band(ro, torch, iq, bins, overlap, first_row, rows, first_col, cols)
    err = band_error(got, want, first_col, cols)
    print("bins %d band [%d,+%d): max err / full row max %.3e" % (bins, first_col, cols, err))
    assert err <= BAR, err
    # the in-band tone is there (the comparison is not of two empty bands)
    assert got.max() > 10 * np.median(got) or cols < 8


@pytest.mark.parametrize("first_col,cols", [(8000, 1024), (8092, 256), (0, 300), (16127, 257), (5001, 1), (777, 513)])
def test_parity_smallest_shape(ro, oracle, torch_cuda, first_col, cols):
    """16384 bins: two slabs at M = 1024, four at 256, two at 512; a band across column N/2 (bin N - 1 next to bin 0),
    one from column 0, one to column N, one column, the first width past 512"""
    check_parity(ro, oracle, torch_cuda, 100 + cols, 16384, 12288, 2, 9, first_col, cols)


def ionozor_band(ro):
    return ro.frequency_to_bin(524288, 96000, 10580.0), 218


@pytest.mark.parametrize("bins,overlap,rows,first_col,cols", [
    (65536, 49152, 7, 50000, 600),                        # Bolidozor.json:45-46, eight slabs
    (524288, 262144, 3, None, 218),                       # Ionozor.json:27-28 (doppler), 128 slabs
    (1048576, 0, 2, 523776, 1024),                        # the largest size, across N/2, 128 slabs of M = 1024
])
def test_parity_other_shapes(ro, oracle, torch_cuda, bins, overlap, rows, first_col, cols):
    if first_col is None:
        first_col = ionozor_band(ro)[0]
    check_parity(ro, oracle, torch_cuda, 7, bins, overlap, 0, rows, first_col, cols)


def test_parity_odd_hop(ro, oracle, torch_cuda):
    """hop 1001: row starts that are 8-byte aligned and no more"""
    check_parity(ro, oracle, torch_cuda, 11, 16384, 16384 - 1001, 0, 5, 7000, 700)


@pytest.mark.parametrize("option", ["i16", "gain", "hann", "custom"])
def test_formats_and_options(ro, oracle, torch_cuda, option):
    bins, overlap, rows, first_col, cols = 16384, 12288, 5, 9100, 300
    iq = make_signal(21, 4 * (bins - overlap) + bins, bins, first_col, cols)
    kw, fmt, w, gain, send = {}, ro.RO_IQ_F32, None, 0.0, iq
    if option == "i16":
        send = np.clip(np.rint(iq * 64.0), -32768, 32767).astype(np.int16)       # un-normalised, like WAVStream
        iq = send.astype(np.float32)
        fmt = ro.RO_IQ_I16
    elif option == "gain":
        gain = 0.25
        kw["iq_gain"] = gain
    elif option == "hann":
        w = oracle.window(bins, "hann")
        kw["window"] = ro.RO_WINDOW_HANN
    else:
        w = np.random.default_rng(5).uniform(0.5, 1.0, bins).astype(np.float32)
        kw["window_table"] = w
    want = oracle.stft(iq, bins, overlap, w=w, gain=gain, max_rows=rows)
    got = run_band(ro, torch_cuda, send, bins, overlap, 0, rows, first_col, cols, fmt=fmt, **kw)
    err = band_error(got, want, first_col, cols)
    print("%s: max err / full row max %.3e" % (option, err))
    assert err <= BAR, err


@pytest.mark.parametrize("rows", [1, 37])
def test_stride_and_bounds(ro, oracle, torch_cuda, rows):
    torch = torch_cuda
    bins, overlap, first_col, cols = 16384, 12288, 3000, 300
    stride = cols + 13
    iq, want = case(oracle, 31, bins, overlap, 0, 37, first_col, cols)
    d_iq = torch.from_numpy(iq).cuda()
    sentinel = -777.25
    d_band = torch.full((rows + 1, stride), sentinel, dtype=torch.float32, device="cuda")       # + a guard row
    with ro.Stft(bins=bins, overlap=overlap) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, d_band, band_stride=stride)
        torch.cuda.synchronize()
    out = d_band.cpu().numpy()
    assert (out[:rows, cols:] == sentinel).all(), "floats beyond cols were written"
    assert (out[rows] == sentinel).all(), "the row after the last one was written"
    assert band_error(out[:rows, :cols], want[:rows], first_col, cols) <= BAR
    assert np.array_equal(out[:rows, :cols], run_band(ro, torch, iq, bins, overlap, 0, rows, first_col, cols))


def test_two_launches_give_the_same_bits(ro, oracle, torch_cuda):
    """524288 bins: 128 slabs per row summed by the finishing kernel -- in slab order, not in arrival order"""
    torch = torch_cuda
    bins, overlap, rows = 524288, 262144, 3
    first_col, cols = ionozor_band(ro)
    iq, _ = case(oracle, 7, bins, overlap, 0, rows, first_col, cols)
    d_iq = torch.from_numpy(iq).cuda()
    a = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    b = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, a)
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, b)
        torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bolidozor_bands(ro, oracle):
    b = oracle.bolid_bands(65536, 96000, 49152, 26450, 26550, 26000, 26300, 5, 2, 40)       # Bolidozor.json:84-93
    return ro.Bands(low_noise=b.low_noise, noise_width=b.noise_width, low_detect=b.low_detect,
                    detect_width=b.detect_width, avg_bins=b.avg_bins)


def test_scan_records(ro, oracle, torch_cuda):
    """records of band mode: bit-identical to the oracle's scan of the band image the GPU returned (bands moved by
    first_col), and the same peak as the full path wherever the row's maximum is not a near-tie"""
    torch = torch_cuda
    bins, overlap, rows, fs = 65536, 49152, 33, 96000
    hop = bins - overlap
    bands = bolidozor_bands(ro, oracle)
    first_col, cols = ro.bands_hull(bands, bins)
    assert ro.band_supported(bins, cols)
    iq = noise_iq(np.random.default_rng(41), (rows - 1) * hop + bins)
    # a chirp through the detect band (26450 ... 26550 Hz): 26545 Hz falling 15 Hz/s over the 6.1 s of the stream;
    # amplitude 3: on the oracle's own rows no row's two largest detect-band values are within 1e-4 of each other
    add_chirp(iq, 0, 10.0, 26545.0, -15.0, 3.0, fs=fs)
    d_iq = torch.from_numpy(iq).cuda()
    d_band = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    d_rows = torch.zeros((rows, bins), dtype=torch.float32, device="cuda")
    d_full = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, sample_rate=fs, bands=bands) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, d_band, d_records=d_recs)
        st.run_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, d_rows, d_records=d_full)
        torch.cuda.synchronize()
    image = d_band.cpu().numpy()
    got = d_recs.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1)
    n, p, a = oracle.scan_rows(image, bands.low_noise - first_col, bands.noise_width, bands.low_detect - first_col,
                               bands.detect_width, bands.avg_bins)
    assert np.array_equal(got["peak"], p)
    assert np.array_equal(got["noise"].view(np.uint32), n.view(np.uint32))
    assert np.array_equal(got["average"].view(np.uint32), a.view(np.uint32))
    assert len(set(p.tolist())) > 10                        # the chirp moves through the band
    # against the full path: the same peak on every row whose maximum is not a near-tie
    full = d_full.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1)
    want = oracle.stft(iq, bins, overlap, max_rows=rows)
    det = np.sort(want[:, bands.low_detect:bands.low_detect + bands.detect_width].astype(np.float64), axis=1)
    clear = (det[:, -1] - det[:, -2]) > 1e-4 * det[:, -1]
    skipped = int((~clear).sum())
    print("rows skipped as near-ties: %d of %d" % (skipped, rows))
    assert skipped <= 2
    assert np.array_equal(got["peak"][clear], full["peak"][clear])
    assert band_error(image, want, first_col, cols) <= BAR


def test_refusals(ro, torch_cuda):
    torch = torch_cuda
    bins, overlap = 16384, 12288
    samples = 4 * (bins - overlap) + bins                   # five rows
    d_iq = torch.zeros((samples, 2), dtype=torch.float32, device="cuda")
    sentinel = 5.5
    d_band = torch.full((5, 1100), sentinel, dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((5, 3), dtype=torch.float32, device="cuda")

    def refused(st, code, word, *args, **kw):
        with pytest.raises(ro.StftError) as e:
            st.band_resident(d_iq, ro.RO_IQ_F32, samples, *args, **kw)
        assert e.value.code == code, str(e.value)
        text = (ro.library().ro_last_error() or b"").decode()
        assert word in text, text

    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        refused(st, -2, "RO_PRECISION_F64", 0, 5, 100, 300, d_band)
    with ro.Stft(bins=32728, overlap=0) as st:
        refused(st, -2, "power-of-two", 0, 1, 100, 300, d_band)
    bands = ro.Bands(low_noise=2000, noise_width=100, low_detect=2200, detect_width=50, avg_bins=9)
    with ro.Stft(bins=bins, overlap=overlap, bands=bands) as st:
        refused(st, -2, "1025", 0, 5, 100, 1025, d_band)
        refused(st, -1, "records need", 0, 5, 2100, 300, d_band, d_records=d_recs)       # the noise band is outside
        refused(st, -1, "records need", 0, 5, 2000, 252, d_band, d_records=d_recs)       # the average's margin is
        refused(st, -1, "outside", 0, 5, bins - 299, 300, d_band)
        refused(st, -1, "band_stride", 0, 5, 100, 300, d_band, band_stride=299)
        refused(st, -1, "samples", 1, 5, 100, 300, d_band)
        st.band_resident(d_iq, ro.RO_IQ_F32, samples, 0, 0, 100, 300, d_band)            # rows = 0: RO_OK, nothing touched
        st.band_resident(None, ro.RO_IQ_F32, 0, 7, 0, 100, 300, None)
        torch.cuda.synchronize()
        assert (d_band == sentinel).all().item()
        # ... and the band that does hold the bands goes through, records and all
        st.band_resident(d_iq, ro.RO_IQ_F32, samples, 0, 5, 1996, 300, d_band, band_stride=1100, d_records=d_recs)
        torch.cuda.synchronize()
    with ro.Stft(bins=bins, overlap=overlap) as st:                                        # no bands configured
        refused(st, -1, "enable_scan", 0, 5, 2000, 300, d_band, d_records=d_recs)
