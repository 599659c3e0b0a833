"""GPU: every chunked launch path across the internal row-chunk seams of ONE call (tests/chunk_seams.py has the seam
arithmetic and the case table; tests/test_chunk_seams_cpu.py keeps it tied to csrc/ro_host.h).

For every case:
  1. one long call into an output filled with NaN, one guard row behind the last, a padded stride on at least one
     case per path: guard and padding keep their fill bit for bit, every real row is finite (a row no chunk wrote
     stays NaN);
  2. split invariance, bit for bit, all rows: the same rows on a fresh handle as three uneven shards whose cuts are
     not the seams, issued small, large, small (scratch grows once and is reused by a smaller call) -- include/ro_stft.h:
     "Two launches on the same input give the same bits", and rows do not depend on where the launch starts;
  3. the oracle on the rows either side of every seam and on the call's last row, at the bar and with the signal recipe
     that path already has (imported from the test file it comes from, named where they are used; no new tolerance);
  4. where the case asks for them, scan records (and tile / extra set) from the long call: equal to
     scan_edges.scan_reference on the rows or band image that very call produced, the tile the column cut of the rows,
     one guard record behind the last intact.
Every call is a legal call of the ABI; nothing here is meant to be refused.

Device memory of the two large cases, measured on an MI355X: torch.cuda.max_memory_allocated plus the handle's
scratch, which torch does not see.
  "spectra 65536":   5.91 GB in torch (the long output, 4099 x 65539 x 8 B = 2.15 GB; the large shard's 4092 x 65536 x
                     8 B = 2.15 GB; the comparison's own copy of the rows it compares) + the handle's two 2 GiB spectra
                     blocks = 10.2 GB at the peak
  "chirp-z 524286":  0.76 GB in torch + the handle's three chirp-z blocks of 128 rows x 2^20 (1 + 1 + 0.5 GiB), the inner
                     handle's two 2 GiB spectra blocks and its 1 GiB four-step block = 8.8 GB at the peak
One handle is alive at a time and every tensor of a case is dropped before the next case starts."""
import time

import numpy as np
import pytest

import chunk_seams as S
import scan_edges
from util import add_tone, noise_iq, rel_to_row_max
from test_gpu_stft import TOL                                                  # float32 rows: 1e-5 of the row maximum
from test_gpu_strict import per_bin                                            # FP64 rows: per bin ...
from test_gpu_band import BAR as BAND_BAR, band_error, make_signal as band_signal
from test_gpu_band_f64 import ONE_ULP, bin_error, make_signal as band64_signal   # ... within 2e-7, one float32 ulp
from test_gpu_band_windows import (BAR as WINDOWS_BAR, image_bands, image_error, make_signal as windows_signal)
from test_gpu_band_windows_f64 import bin_error as windows_bin_error, make_signal as windows64_signal

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---- signals: one per case, made once and left alone ------------------------------------------------------------------
_signals = {}


def signal(c):
    """(what the oracle is given, what is uploaded) -- float32 [samples, 2] both, or the int16 frames and their values"""
    if c.name not in _signals:
        n, seed = S.samples(c), 0x5EA + S.CASES.index(c)
        if c.family == "f64":            # tests/test_gpu_strict.py::test_every_size_per_bin: noise + a 1000 sigma tone
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 7000.0, 1000.0)
        elif c.family == "spectra":      # tests/test_gpu_spectra.py: noise + a 5 sigma tone
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 7000.0, 5.0)
        elif c.family in ("czt", "four"):    # tests/test_gpu_stft.py: noise + a 20 sigma tone
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 10600.0, 20.0)
        elif c.path == "band":
            make = band64_signal if c.precision == S.F64 else band_signal
            iq = make(seed, n, c.bins, *c.windows[0])
        else:
            make = windows64_signal if c.precision == S.F64 else windows_signal
            iq = make(seed, n, c.bins, c.windows)
        send = iq
        if c.fmt == S.IQ_I16:            # un-normalised frames, like WAVStream (tests/test_gpu_band.py's "i16" option)
            send = np.clip(np.rint(iq * 64.0), -32768, 32767).astype(np.int16)
            iq = send.astype(np.float32)
        iq.setflags(write=False)
        send.setflags(write=False)
        _signals[c.name] = (iq, send)
    return _signals[c.name]


def handle_kwargs(ro, c):
    kw = dict(bins=c.bins, overlap=S.overlap(c), precision=c.precision)
    if c.records:
        kw["bands"] = ro.Bands(*S.BANDS[c.name])
        if c.name in S.TILES:
            kw["tile"] = S.TILES[c.name]
        if c.name in S.EXTRA:
            kw["extra_bands"] = [ro.Bands(*e) for e in S.EXTRA[c.name]]
    return kw


def launch(torch, st, c, d_iq, first, n, out, stride, tile=None, recs=None, extra=None):
    s = torch.cuda.current_stream().cuda_stream
    ns = S.samples(c)
    if c.path == "rows":
        st.run_resident(d_iq, c.fmt, ns, first, n, out, row_stride=stride, d_tile=tile, d_records=recs, stream=s)
    elif c.path == "spectra":
        st.spectra_resident(d_iq, c.fmt, ns, first, n, out, stride=stride, stream=s)
    elif c.path == "band":
        first_col, cols = c.windows[0]
        st.band_resident(d_iq, c.fmt, ns, first, n, first_col, cols, out, band_stride=stride, d_records=recs, stream=s)
    else:
        st.band_windows_resident(d_iq, c.fmt, ns, first, n, c.windows, out, band_stride=stride, d_records=recs,
                                 d_extra=extra, stream=s)


def oracle_check(ro, oracle, c, r, got, iq, window):
    """row r of the long call against the oracle, at the bar of the path's own test file; returns (figure, bar)"""
    bins, overlap = c.bins, S.overlap(c)
    if c.path == "spectra":              # tests/test_gpu_spectra.py: |X - X_oracle| <= 1e-5 max |X_oracle|
        z = iq[r * c.hop:r * c.hop + bins].astype(np.float64)
        _, want = oracle.row_with_spectrum(z[:, 0] + 1j * z[:, 1], window)
        x = got.astype(np.float64).reshape(bins, 2)
        return float(np.abs(x[:, 0] + 1j * x[:, 1] - want).max() / np.abs(want).max()), TOL
    want = oracle.stft(iq, bins, overlap, first_row=r, max_rows=1)
    assert want.shape == (1, bins)
    if c.path == "rows":
        if c.precision == S.F64:
            return float(per_bin(got[None], want).max()), ONE_ULP
        return rel_to_row_max(got[None], want), TOL
    if c.path == "band":
        first_col, cols = c.windows[0]
        if c.precision == S.F64:
            return bin_error(got[None], want, first_col, cols), ONE_ULP
        return band_error(got[None], want, first_col, cols), BAND_BAR
    if c.precision == S.F64:
        return windows_bin_error(got[None], want, c.windows), ONE_ULP
    return image_error(got[None], want, c.windows), WINDOWS_BAR


def records_of(ro, t, rows):
    return t[:rows].cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(rows, -1)


def check_case(ro, oracle, torch, c):
    t0 = time.perf_counter()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    iq, send = signal(c)
    rows, width, comp = c.rows, S.width(c), (2 if c.path == "spectra" else 1)
    seams = S.seams(c)
    # the fixture is a valid call: exactly `rows` rows of samples, at least one seam with rows on both sides
    assert send.shape == (S.samples(c), 2) and ro.row_count(send.shape[0], c.bins, S.overlap(c)) == rows
    assert len(seams) >= c.min_seams and 0 < seams[0] and seams[-1] < rows - 1
    fill = int(torch.full((1,), NAN, dtype=torch.float32).view(torch.int32).item())

    def filled(*shape):
        return torch.full(shape, NAN, dtype=torch.float32, device="cuda")

    def untouched(t):
        return bool((t.view(torch.int32) == fill).all())

    d_iq = torch.from_numpy(np.array(send)).cuda()
    stride = width + 3 if c.pad else width
    kw = handle_kwargs(ro, c)
    tile = recs = extra = window = None
    if c.records:
        recs = filled(rows + 1, 3)
        if c.name in S.TILES:
            tile = filled(rows + 1, S.TILES[c.name][1])
        if c.name in S.EXTRA:
            extra = filled(rows + 1, len(S.EXTRA[c.name]), 3)

    # ---- 1. one long call
    long = filled(rows + 1, stride * comp)
    with ro.Stft(**kw) as st:
        launch(torch, st, c, d_iq, 0, rows, long, stride, tile, recs, extra)
        torch.cuda.synchronize()
        if c.path == "spectra":
            window = st.window
    real = long[:rows, :width * comp]
    assert untouched(long[rows]), "the row behind the last one was written"
    assert untouched(long[:rows, width * comp:]), "the stride's padding was written"
    assert bool(torch.isfinite(real).all()), "a row of the long call was never written"

    # ---- 2. three uneven shards on a fresh handle: the same bits
    shards = S.shards(c)
    part = filled(max(n for _, n in shards), width * comp)
    with ro.Stft(**kw) as st:
        for first, n in shards:
            part.fill_(NAN)
            launch(torch, st, c, d_iq, first, n, part, width)
            torch.cuda.synchronize()
            assert torch.equal(part[:n].view(torch.int32), real[first:first + n].view(torch.int32)), (c.name, first, n)
    del part

    # ---- 3. the oracle either side of every seam and on the last row
    for r in S.oracle_rows(c):
        figure, bar = oracle_check(ro, oracle, c, r, real[r].cpu().numpy(), iq, window)
        print("%s: row %d (seams after %s) against the oracle %.3e, bar %.0e" % (c.name, r, seams, figure, bar))
        assert figure <= bar, (c.name, r, figure)

    # ---- 4. records, tile and the extra set of the long call
    if c.records:
        image = real.cpu().numpy()
        b = ro.Bands(*S.BANDS[c.name])
        sets = [(b, records_of(ro, recs, rows)[:, 0])]
        if extra is not None:
            got = records_of(ro, extra, rows)
            sets += [(ro.Bands(*e), np.ascontiguousarray(got[:, i])) for i, e in enumerate(S.EXTRA[c.name])]
            assert untouched(extra[rows]), "the extra records' guard was written"
        for which, (bands, got) in enumerate(sets):
            where = image_bands(bands, c.windows) if c.windows else tuple(S.BANDS[c.name])
            want = scan_edges.scan_reference(image, where, width)
            assert scan_edges.same_bits(got, want), (c.name, which, scan_edges.describe(got, want))
        assert untouched(recs[rows]), "the record behind the last one was written"
        if tile is not None:
            first_col, cols = S.TILES[c.name]
            assert torch.equal(tile[:rows].view(torch.int32), real[:, first_col:first_col + cols].view(torch.int32))
            assert untouched(tile[rows]), "the tile's guard row was written"

    torch.cuda.synchronize()
    print("%s: %d rows in chunks of %d, %.2f s, torch peak %.2f GB" % (
        c.name, rows, S.chunk_rows(c), time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 1e9))
    del long, real, d_iq, tile, recs, extra
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", S.names("rows"))
def test_full_rows_across_their_seams(ro, oracle, torch_cuda, name):
    """FP64 through HBM scratch (64 rows per chunk at 131072 bins, 8 at 1048576), chirp-z (128 rows at M = 2^20; the
    65535-row grid at M = 1024) and the four-step form (128 rows at 1048576 bins, 256 at 524288)"""
    check_case(ro, oracle, torch_cuda, S.by_name(name))


@pytest.mark.parametrize("name", S.names("spectra"))
def test_complex_spectra_across_their_seam(ro, oracle, torch_cuda, name):
    """launch_spectra_big: 4096 rows per chunk at 65536 bins"""
    check_case(ro, oracle, torch_cuda, S.by_name(name))


@pytest.mark.parametrize("name", S.names("band"))
def test_band_across_its_seams(ro, oracle, torch_cuda, name):
    """ro_stft_band_resident, float32 and FP64: the 256 MiB block of partial sums (float32; FP64's is crossed by
    tests/test_gpu_band_f64.py::test_chunk_boundary) and the 65535-row grid"""
    check_case(ro, oracle, torch_cuda, S.by_name(name))


@pytest.mark.parametrize("name", S.names("windows"))
def test_band_windows_across_their_seams(ro, oracle, torch_cuda, name):
    """ro_stft_band_windows_resident, float32 and FP64: the 256 MiB block of partial sums and the 65535-row grid"""
    check_case(ro, oracle, torch_cuda, S.by_name(name))
