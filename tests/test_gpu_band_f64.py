"""GPU parity of the band-only transform on RO_PRECISION_F64 handles of 131072 bins and above (ro_stft_band_resident,
csrc/ro_band_f64.hip) against the oracle's rows.

The bar is the FP64 mode's own, per bin: |band - oracle_row[first_col : first_col + cols]| <= ONE_ULP x oracle on every
bin of the band -- one float32 ulp, with a 40 dB carrier 5000 columns outside the band in every signal, which a
float32 transform's rounding noise would bury the band's weak bins under.  The scan records are integer / exact work on
top of the band image: bit-identical to the oracle's scan of that image."""
import numpy as np
import pytest

from util import add_chirp, add_tone, noise_iq

pytestmark = pytest.mark.gpu

ONE_ULP = 2e-7
FS = 48000
BINS, OVERLAP = 131072, 98304        # the smallest size the kernels exist at


def column_freq(bins, col):
    """frequency whose bin is (fractional) column `col` of the fft-shifted row"""
    return (col - bins / 2) * FS / bins


def make_signal(seed, samples, bins, first_col, cols):
    """test_gpu_band.make_signal's: sigma = 1 noise + a tone of amplitude 300 some 5000 columns OUTSIDE the band + a tone
    of amplitude 3 at a non-integer bin inside it"""
    iq = noise_iq(np.random.default_rng(seed), samples)
    outside = first_col + cols + 5000 if first_col + cols + 5000 < bins else first_col - 5000
    assert 0 <= outside < bins
    add_tone(iq, column_freq(bins, outside + 0.21), 300.0, fs=FS)
    add_tone(iq, column_freq(bins, first_col + cols // 2 + 0.37), 3.0, fs=FS, phase=0.5)
    return iq


def bin_error(got, full_rows, first_col, cols):
    """max over the band's bins of |band - oracle| / oracle"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(full_rows, dtype=np.float64)[:, first_col:first_col + cols]
    assert (want > 0).all()
    return float((np.abs(got - want) / want).max())


def upload(torch, iq):
    return torch.from_numpy(np.array(iq)).cuda()          # (a copy: the cached signals are read-only)


def run_band(ro, torch, iq, bins, overlap, first_row, rows, first_col, cols, fmt=None, stride=None, **kw):
    fmt = ro.RO_IQ_F32 if fmt is None else fmt
    d_iq = upload(torch, iq)
    d_band = torch.zeros((rows, stride or cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64, **kw) as st:
        st.band_resident(d_iq, fmt, iq.shape[0], first_row, rows, first_col, cols, d_band, band_stride=stride)
        torch.cuda.synchronize()
    return d_band.cpu().numpy()


_cache = {}


def case(oracle, seed, bins, overlap, first_row, rows, first_col, cols):
    """(iq, the oracle's full rows [first_row, +rows)) of a seeded signal, computed once per module and left alone"""
    key = (seed, bins, overlap, first_row, rows, first_col, cols)
    if key not in _cache:
        hop = bins - overlap
        iq = make_signal(seed, (first_row + rows - 1) * hop + bins, bins, first_col, cols)
        want = oracle.stft(iq, bins, overlap, first_row=first_row, max_rows=rows)
        iq.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (iq, want)
    return _cache[key]


def check_parity(ro, oracle, torch, seed, bins, overlap, first_row, rows, first_col, cols, as_doubles=False):
    iq, want = case(oracle, seed, bins, overlap, first_row, rows, first_col, cols)
    send, fmt = (iq.astype(np.float64), ro.RO_IQ_F64) if as_doubles else (iq, ro.RO_IQ_F32)
    got = run_band(ro, torch, send, bins, overlap, first_row, rows, first_col, cols, fmt=fmt)
    err = bin_error(got, want, first_col, cols)
    print("bins %d band [%d,+%d)%s: max per-bin err %.3e" % (bins, first_col, cols, " doubles" if as_doubles else "", err))
    assert err <= ONE_ULP, err
    # the in-band tone is there (the comparison is not of two empty bands)
    assert got.max() > 10 * np.median(got) or cols < 8


@pytest.mark.parametrize("first_col,cols", [(65000, 1024), (0, 300), (130815, 257), (70001, 1), (40000, 256), (777, 513)])
def test_parity_smallest_shape(ro, oracle, torch_cuda, first_col, cols):
    """131072 bins, 32 slabs: M = 1024 across column N/2 (bin N - 1 next to bin 0), M = 512 from column 0, a band to
    column N, one column, M = 256, the first width past 512"""
    check_parity(ro, oracle, torch_cuda, 100 + cols, BINS, OVERLAP, 2, 5, first_col, cols)


def ionozor_band(ro):
    return ro.frequency_to_bin(524288, 96000, 10580.0), 218


@pytest.mark.parametrize("bins,overlap,rows,first_col,cols", [
    (524288, 262144, 3, None, 218),                       # Ionozor.json:27-28 (doppler), 128 slabs
    (1048576, 0, 2, 523776, 1024),                        # the largest size, across N/2, 256 slabs of M = 1024
])
def test_parity_other_sizes(ro, oracle, torch_cuda, bins, overlap, rows, first_col, cols):
    if first_col is None:
        first_col = ionozor_band(ro)[0]
    check_parity(ro, oracle, torch_cuda, 7, bins, overlap, 0, rows, first_col, cols)


@pytest.mark.parametrize("as_doubles", [False, True])
def test_parity_odd_hop(ro, oracle, torch_cuda, as_doubles):
    """hop 1001: row starts aligned to one sample (8 bytes of float32, 16 of double) and no more"""
    check_parity(ro, oracle, torch_cuda, 11, BINS, BINS - 1001, 0, 4, 60000, 700, as_doubles=as_doubles)


@pytest.mark.parametrize("option", ["i16", "gain", "hann", "custom", "f64"])
def test_formats_and_options(ro, oracle, torch_cuda, option):
    bins, overlap, rows, first_col, cols = BINS, OVERLAP, 3, 72000, 300
    samples = (rows - 1) * (bins - overlap) + bins
    iq = make_signal(21, samples, bins, first_col, cols)
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
    elif option == "custom":
        w = np.random.default_rng(5).uniform(0.5, 1.0, bins).astype(np.float32)
        kw["window_table"] = w
    else:
        # true doubles: sigma = 1 noise that no float32 holds, the amplitude-300 carrier outside the band built in double
        iq = np.random.default_rng(22).standard_normal((samples, 2))
        t = np.arange(samples, dtype=np.float64)
        ph = 2.0 * np.pi * column_freq(bins, first_col + cols + 5000.21) * t / FS
        iq[:, 0] += 300.0 * np.cos(ph)
        iq[:, 1] += 300.0 * np.sin(ph)
        send, fmt = iq, ro.RO_IQ_F64
    want = oracle.stft(iq, bins, overlap, w=w, gain=gain, max_rows=rows)
    if option == "f64":
        # the test can tell doubles from narrowed doubles: the oracle itself moves by far more than the bar
        narrowed = oracle.stft(iq.astype(np.float32), bins, overlap, max_rows=rows)
        moved = bin_error(narrowed[:, first_col:first_col + cols], want, first_col, cols)
        print("oracle on the narrowed samples against the oracle on the doubles: %.3e" % moved)
        assert moved > 10 * ONE_ULP, moved
    got = run_band(ro, torch_cuda, send, bins, overlap, 0, rows, first_col, cols, fmt=fmt, **kw)
    err = bin_error(got, want, first_col, cols)
    print("%s: max per-bin err %.3e" % (option, err))
    assert err <= ONE_ULP, err


@pytest.mark.parametrize("rows", [1, 9])
def test_stride_and_bounds(ro, oracle, torch_cuda, rows):
    torch = torch_cuda
    bins, overlap, first_col, cols = BINS, OVERLAP, 3000, 300
    stride = cols + 13
    iq, want = case(oracle, 31, bins, overlap, 0, 9, first_col, cols)
    d_iq = upload(torch, iq)
    sentinel = -777.25
    d_band = torch.full((rows + 1, stride), sentinel, dtype=torch.float32, device="cuda")       # + a guard row
    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, d_band, band_stride=stride)
        torch.cuda.synchronize()
    out = d_band.cpu().numpy()
    assert (out[:rows, cols:] == sentinel).all(), "floats beyond cols were written"
    assert (out[rows] == sentinel).all(), "the row after the last one was written"
    assert bin_error(out[:rows, :cols], want[:rows], first_col, cols) <= ONE_ULP
    dense = run_band(ro, torch, iq, bins, overlap, 0, rows, first_col, cols)
    assert np.array_equal(out[:rows, :cols].view(np.uint32), dense.view(np.uint32))


def test_chunk_boundary(ro, oracle, torch_cuda):
    """1048576 bins x 1024 columns: 256 slabs x 1024 x 16 B = 4 MiB of partial sums per row, so the 256 MiB block holds 64
    rows and a call of 65 runs as 64 + 1"""
    torch = torch_cuda
    bins, hop, first_col, cols, rows = 1048576, 4096, 523776, 1024, 65
    overlap = bins - hop
    iq = make_signal(51, (rows - 1) * hop + bins, bins, first_col, cols)
    d_iq = upload(torch, iq)
    one = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    two = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, one)
        torch.cuda.synchronize()
    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 40, first_col, cols, two[:40])
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 40, 25, first_col, cols, two[40:])
        torch.cuda.synchronize()
    one, two = one.cpu().numpy(), two.cpu().numpy()
    assert one.all() and np.array_equal(one.view(np.uint32), two.view(np.uint32))
    want = oracle.stft(iq, bins, overlap, first_row=63, max_rows=2)
    err = bin_error(one[63:65], want, first_col, cols)
    print("rows 63, 64 (either side of the chunk boundary): max per-bin err %.3e" % err)
    assert err <= ONE_ULP, err


def test_two_launches_give_the_same_bits(ro, oracle, torch_cuda):
    """524288 bins: 128 slabs per row summed by the finishing kernel -- in slab order, not in arrival order"""
    torch = torch_cuda
    bins, overlap, rows = 524288, 262144, 3
    first_col, cols = ionozor_band(ro)
    iq, _ = case(oracle, 7, bins, overlap, 0, rows, first_col, cols)
    d_iq = upload(torch, iq)
    a = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    b = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, a)
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, b)
        torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_scan_records(ro, oracle, torch_cuda):
    """records of band mode on an FP64 handle: bit-identical to the oracle's scan of the band image the GPU returned
    (bands moved by first_col), and the oracle's own peak on EVERY row: on the oracle's rows the two largest detect-band
    values of each row differ by at least 2 % of the larger, which one float32 ulp cannot bridge"""
    torch = torch_cuda
    bins, overlap, rows, fs = BINS, OVERLAP, 17, 96000
    hop = bins - overlap
    ob = oracle.bolid_bands(bins, fs, overlap, 26450, 26550, 26000, 26300, 5, 2, 40)       # Bolidozor.json:84-93
    assert (ob.low_noise, ob.noise_width, ob.low_detect, ob.detect_width, ob.avg_bins) == (101034, 410, 101649, 136, 54)
    bands = ro.Bands(low_noise=ob.low_noise, noise_width=ob.noise_width, low_detect=ob.low_detect,
                     detect_width=ob.detect_width, avg_bins=ob.avg_bins)
    first_col, cols = ro.bands_hull(bands, bins)
    assert (first_col, cols) == (101034, 777)
    assert ro.band_supported(bins, cols, ro.RO_PRECISION_F64)
    iq = noise_iq(np.random.default_rng(41), (rows - 1) * hop + bins)
    add_chirp(iq, 0, 10.0, 26540.0, -15.0, 3.0, fs=fs)      # through the detect band (26450 ... 26550 Hz)
    want = oracle.stft(iq, bins, overlap, max_rows=rows)
    wn, wp, wa = oracle.scan_rows(want, bands.low_noise, bands.noise_width, bands.low_detect, bands.detect_width,
                                  bands.avg_bins)
    assert wp.tolist()[:3] == [109, 102, 95] and wp.tolist()[-2:] == [4, 0] and len(set(wp.tolist())) == 17
    det = np.sort(want[:, bands.low_detect:bands.low_detect + bands.detect_width].astype(np.float64), axis=1)
    assert ((det[:, -1] - det[:, -2]) >= 0.02 * det[:, -1]).all()
    d_iq = upload(torch, iq)
    d_band = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, sample_rate=fs, bands=bands, precision=ro.RO_PRECISION_F64) as st:
        st.band_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, rows, first_col, cols, d_band, d_records=d_recs)
        torch.cuda.synchronize()
    image = d_band.cpu().numpy()
    got = d_recs.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(-1)
    n, p, a = oracle.scan_rows(image, bands.low_noise - first_col, bands.noise_width, bands.low_detect - first_col,
                               bands.detect_width, bands.avg_bins)
    assert np.array_equal(got["peak"], p)
    assert np.array_equal(got["noise"].view(np.uint32), n.view(np.uint32))
    assert np.array_equal(got["average"].view(np.uint32), a.view(np.uint32))
    assert np.array_equal(got["peak"], wp)                  # all 17 rows, none left out
    assert bin_error(image, want, first_col, cols) <= ONE_ULP


def test_refusals(ro, torch_cuda):
    torch = torch_cuda
    bins, overlap = BINS, OVERLAP
    samples = 4 * (bins - overlap) + bins                   # five rows
    d_iq = torch.zeros((samples, 2), dtype=torch.float32, device="cuda")
    sentinel = 5.5
    d_band = torch.full((5, 1100), sentinel, dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((5, 3), dtype=torch.float32, device="cuda")
    f64 = dict(precision=ro.RO_PRECISION_F64)

    def refused(st, code, word, *args, fmt=None, **kw):
        with pytest.raises(ro.StftError) as e:
            st.band_resident(d_iq, ro.RO_IQ_F32 if fmt is None else fmt, samples, *args, **kw)
        assert e.value.code == code, str(e.value)
        text = (ro.library().ro_last_error() or b"").decode()
        assert word in text, text

    with ro.Stft(bins=65536, overlap=49152, **f64) as st:
        refused(st, -2, "RO_PRECISION_F64", 0, 5, 100, 300, d_band)
        refused(st, -2, "131072", 0, 5, 100, 300, d_band)                               # ... and says where the band starts
    bands = ro.Bands(low_noise=2000, noise_width=100, low_detect=2200, detect_width=50, avg_bins=9)
    with ro.Stft(bins=bins, overlap=overlap, bands=bands, **f64) as st:
        refused(st, -2, "1025", 0, 5, 100, 1025, d_band)
        refused(st, -1, "outside", 0, 5, bins - 299, 300, d_band)
        refused(st, -1, "band_stride", 0, 5, 100, 300, d_band, band_stride=299)
        refused(st, -1, "samples", 1, 5, 100, 300, d_band)
        refused(st, -1, "records need", 0, 5, 2100, 300, d_band, d_records=d_recs)       # the noise band is outside
        st.band_resident(d_iq, ro.RO_IQ_F32, samples, 0, 0, 100, 300, d_band)            # rows = 0: RO_OK, nothing touched
        st.band_resident(None, ro.RO_IQ_F64, 0, 7, 0, 100, 300, None)
        torch.cuda.synchronize()
        assert (d_band == sentinel).all().item()
    with ro.Stft(bins=bins, overlap=overlap) as st:                                        # float32: no doubles, as before
        refused(st, -2, "RO_IQ_F32 or RO_IQ_I16", 0, 5, 100, 300, d_band, fmt=ro.RO_IQ_F64)
