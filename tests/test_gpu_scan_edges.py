"""The band scan (noise / peak / average, src/BolidRecorder.cpp:121-132, :313-347) and the tile cut where the suite did
not reach: an averaging window that leaves the row, float32's edge values inside a band, the forms of the 32768-bin
kernel's fused epilogue, its tile cut and log, and an all-zero stream through every float32 family.

The judge is tests/scan_edges.py's numpy restatement (pinned to the oracle by tests/test_scan_edges_cpu.py): columns
outside [0, bins) add 0 to average() and the sum is divided by avg_bins all the same.  Every comparison of
a record is bit-exact: `peak` as integers, `noise` and `average` through .view(np.uint32).  No band holds NaN or -0.0:
their order is not defined on either side, and magnitudes cannot be -0.0.  The log of the tile keeps the bars of
tests/test_gpu_ln_tile.py (its grey-level statistics are for images of thousands of pixels and are not repeated on tiles
of 8)."""
import numpy as np
import pytest

import scan_edges as se
from test_gpu_ln_tile import ln_close, viewer_levels
from util import noise_iq, rel_to_row_max

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def mk(ro, t):
    return ro.Bands(low_noise=t[0], noise_width=t[1], low_detect=t[2], detect_width=t[3], avg_bins=t[4])


def recs_of(ro, d, n):
    """the first n records of a device buffer and whether everything behind them is still the sentinel"""
    a = d.cpu().numpy()
    return a[:n].copy().view(ro.capi.SCAN_DTYPE).reshape(-1), bool((a[n:] == np.float32(SENTINEL)).all())


def rec_buffer(torch, n):
    return torch.full((n + 1, 3), SENTINEL, dtype=torch.float32, device="cuda")       # one guard record


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def two_routes(ro, torch, st, d_rows, nrows, stride, bands):
    """the band set as the primary through scan_kernel and as the only extra set through scan_sets_kernel"""
    b = mk(ro, bands)
    st.set_bands(b)
    st.set_extra_bands([b])
    d_a, d_b = rec_buffer(torch, nrows), rec_buffer(torch, nrows)
    st.scan_resident(d_rows, nrows, d_a, row_stride=stride, stream=stream_of(torch))
    st.scan_sets_resident(d_rows, nrows, d_b, row_stride=stride, stream=stream_of(torch))
    torch.cuda.synchronize()
    (a, ga), (b, gb) = recs_of(ro, d_a, nrows), recs_of(ro, d_b, nrows)
    assert ga and gb, "a record behind the last row was written"
    return a, b


def judge(failures, name, want, **got):
    for route, recs in got.items():
        if not se.same_bits(recs, want):
            failures.append("%s, %s: %s" % (name, route, se.describe(recs, want)))


# ---- A: the window leaves the row, rows in HBM ---------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "strided"])
def test_average_window_leaving_the_row(ro, torch_cuda, layout):
    """scan_kernel<E> and scan_sets_kernel<E> at the row's ends.  `strided`: the rows are a view inside a buffer of NaN,
    with a stride of NaN in front of row 0 and one behind the last row, so a read outside the row makes `average` NaN
    instead of a plausible number; the NaN words are intact afterwards."""
    torch = torch_cuda
    failures, handles, staged = [], {}, {}
    try:
        for name, rows, bands in se.hbm_window_cases():
            nrows, bins = rows.shape
            if bins not in handles:
                handles[bins] = ro.Stft(bins=bins, overlap=0, bands=mk(ro, bands))
                if layout == "dense":
                    staged[bins] = (torch.from_numpy(rows.copy()).cuda(), bins, None, None)
                else:
                    stride = bins + se.A_STRIDE_EXTRA
                    host = np.full((nrows + 2) * stride, np.nan, np.float32)
                    for r in range(nrows):
                        host[(r + 1) * stride:(r + 1) * stride + bins] = rows[r]
                    buf = torch.from_numpy(host).cuda()
                    staged[bins] = (buf[stride:], stride, buf, host)
            d_rows, stride, _, _ = staged[bins]
            primary, extra = two_routes(ro, torch, handles[bins], d_rows, nrows, stride, bands)
            judge(failures, name, se.scan_reference(rows, bands, bins), scan_kernel=primary, scan_sets_kernel=extra)
            if not se.same_bits(primary, extra):
                failures.append("%s: the two routes differ: %s" % (name, se.describe(primary, extra)))
        for bins, (_, _, buf, host) in staged.items():
            if buf is not None:
                assert np.array_equal(buf.cpu().numpy().view(np.uint32), host.view(np.uint32)), "the rows' buffer was written"
    finally:
        for st in handles.values():
            st.close()
    assert not failures, "\n".join(failures)


# ---- B: values at float32's edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", se.B_FIXTURES)
def test_float32_edge_values_in_a_band(ro, torch_cuda, fixture):
    """denormals (a compare that flushes them calls a faint band all equal), keys that differ in their low byte only
    (the radix select's first pass is its last) or at bit 8 (shift = 1), FLT_MAX (noise doubles to +inf), +inf"""
    torch = torch_cuda
    failures = []
    with ro.Stft(bins=se.B_BINS, overlap=0, bands=mk(ro, (0, 1, 0, 1, 1))) as st:
        for name, fx, rows, bands in se.float_edge_cases():
            if fx != fixture:
                continue
            d_rows = torch.from_numpy(rows.copy()).cuda()
            primary, extra = two_routes(ro, torch, st, d_rows, se.B_ROWS, se.B_BINS, bands)
            judge(failures, name, se.scan_reference(rows, bands, se.B_BINS), scan_kernel=primary, scan_sets_kernel=extra)
    assert not failures, "\n".join(failures)


# ---- C: the fused epilogue's own forms, through the transform -------------------------------------------------------
@pytest.mark.parametrize("bins,overlap", se.C_SHAPES)
def test_epilogue_forms_through_the_transform(ro, torch_cuda, bins, overlap):
    """32768 bins: the primary's record comes from stft32k_kernel's epilogue on the LDS image (scan_noise<8> / <0>,
    scan_peak<8> and its batched loop, the image's wrap at column 16384, windows clipped at both ends).  4096 bins is the
    control: the primary's route there is scan_kernel, so a failure at 32768 only points at the epilogue.  Four answers
    per band set: fused (or scan_kernel) primary, scan_sets_kernel extra, a separate scan_resident of the rows just
    written, and the reference on those rows."""
    torch = torch_cuda
    failures, signals = [], {}
    s = stream_of(torch)
    R = se.C_ROWS
    cases = se.epilogue_cases(bins)
    with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, cases[0][1])) as st:
        for name, bands, tones in cases:
            if tones not in signals:
                signals[tones] = torch.from_numpy(se.tone_signal(bins, overlap, tones).copy()).cuda()
            d_iq = signals[tones]
            b = mk(ro, bands)
            st.set_bands(b)
            st.set_extra_bands([b])
            d_rows = torch.zeros((R, bins), dtype=torch.float32, device="cuda")
            d_recs, d_extra, d_again = rec_buffer(torch, R), rec_buffer(torch, R), rec_buffer(torch, R)
            st.run_resident_sets(d_iq, ro.RO_IQ_F32, d_iq.shape[0], 0, R, d_rows, d_records=d_recs, d_extra=d_extra, stream=s)
            st.scan_resident(d_rows, R, d_again, stream=s)
            torch.cuda.synchronize()
            rows = d_rows.cpu().numpy()
            assert se.peaks_on_tones(rows, bands, tones), "%s: the tone is not its band's maximum (fixture)" % name
            (primary, g0), (extra, g1), (again, g2) = recs_of(ro, d_recs, R), recs_of(ro, d_extra, R), recs_of(ro, d_again, R)
            assert g0 and g1 and g2, "%s: a record behind the last row was written" % name
            judge(failures, name, se.scan_reference(rows, bands, bins), primary=primary, scan_sets_kernel=extra, scan_resident=again)
    assert not failures, "\n".join(failures)


# ---- D: the epilogue's tile cut and its log ---------------------------------------------------------------------------
@pytest.mark.parametrize("first,cols", se.D_TILES)
def test_epilogue_tile_cut_and_log(ro, oracle, torch_cuda, first, cols):
    """waves 2 and 3 of the epilogue split the tile at ((cols + 127) >> 7) << 6: tiles across column 16384, narrower
    than 64 columns, no multiple of 64, at either end of the row, as wide as the row.  Every output has one guard row."""
    torch = torch_cuda
    bins, overlap, R = se.D_BINS, se.D_OVERLAP, se.C_ROWS
    iq = se.tone_signal(bins, overlap, se.D_TONES)
    d_iq = torch.from_numpy(iq.copy()).cuda()
    s = stream_of(torch)

    def outputs(n):
        return [torch.full((R + 1, w), SENTINEL, dtype=torch.float32, device="cuda") for w in n]

    rows0, tile0 = outputs((bins, cols))
    with ro.Stft(bins=bins, overlap=overlap, tile=(first, cols)) as st:
        st.run_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, R, rows0, d_tile=tile0, stream=s)
        torch.cuda.synchronize()
    rows1, tile1, d_ln, d_mm = outputs((bins, cols, cols, 2))
    with ro.Stft(bins=bins, overlap=overlap, tile=(first, cols), tile_ln=True) as st:
        st.run_resident_ln(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, R, rows1, tile1, d_ln=d_ln, d_minmax=d_mm, stream=s)
        torch.cuda.synchronize()
    rows0, tile0, rows1, tile1, ln, mm = (t.cpu().numpy() for t in (rows0, tile0, rows1, tile1, d_ln, d_mm))
    for out in (rows0, tile0, rows1, tile1, ln, mm):
        assert (out[R] == np.float32(SENTINEL)).all(), "the guard row was written"
    rows0, tile0, rows1, tile1, ln, mm = (a[:R] for a in (rows0, tile0, rows1, tile1, ln, mm))
    assert np.array_equal(rows0.view(np.uint32), rows1.view(np.uint32))
    image = np.ascontiguousarray(rows0[:, first:first + cols])
    assert np.array_equal(tile0.view(np.uint32), image.view(np.uint32))
    assert np.array_equal(tile1.view(np.uint32), image.view(np.uint32))
    # ... as test_fused_ln_tile_of_the_transform checks the log and the rows' min / max
    assert (image != 0).all()
    want_ln, _, (mn, mx) = oracle.ln_levels(image)
    assert ln_close(ln, want_ln)
    assert np.array_equal(mm[:, 0], ln.min(axis=1)) and np.array_equal(mm[:, 1], ln.max(axis=1))   # reductions are exact
    gmn, gmx = mm[:, 0].min(), mm[:, 1].max()
    assert ln_close(np.array([gmn, gmx], np.float32), np.array([mn, mx], np.float32))
    assert np.array_equal(ro.ln_levels(ln, gmn, gmx), viewer_levels(ln, image, gmn, gmx))


# ---- E: silence -------------------------------------------------------------------------------------------------------
def silent_stream(ro, torch, fmt, samples):
    dtype = torch.float32 if fmt == ro.RO_IQ_F32 else torch.int16
    return torch.zeros((samples, 2), dtype=dtype, device="cuda")


def all_plus_zero(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == 0).all())


def silent_records(recs, detect_width):
    """noise = +0.0, peak = the last column of the band (all ties), average = +0.0"""
    return (all_plus_zero(recs["noise"]) and all_plus_zero(recs["average"]) and (recs["peak"] == detect_width - 1).all())


@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("bins,overlap,R", se.E_SHAPES)
def test_digital_silence(ro, torch_cuda, bins, overlap, R, fmt):
    """a muted card or an empty WAV: rows of +0.0 exactly; the scan takes its kmin == kmax exit and the all-ties peak on
    the fused and the separate routes; the tile's log is -inf and every row's min / max is (+inf, -inf)"""
    torch = torch_cuda
    fmt = ro.RO_IQ_F32 if fmt == "f32" else ro.RO_IQ_I16
    samples = bins + (R - 1) * (bins - overlap)
    d_iq = silent_stream(ro, torch, fmt, samples)
    bands, tile = se.silence_bands(bins)
    s = stream_of(torch)
    full = lambda w: torch.full((R, w), 7.0, dtype=torch.float32, device="cuda")
    rows_ln, d_tile, d_ln, d_mm, rows_sets = full(bins), full(tile[1]), full(tile[1]), full(2), full(bins)
    recs_ln, recs_sets, recs_extra, recs_again = (rec_buffer(torch, R) for _ in range(4))
    with ro.Stft(bins=bins, overlap=overlap, iq_gain=0.0, bands=mk(ro, bands), tile=tile, tile_ln=True,
                 extra_bands=[mk(ro, bands)]) as st:
        st.run_resident_ln(d_iq, fmt, samples, 0, R, rows_ln, d_tile, d_ln=d_ln, d_minmax=d_mm, d_records=recs_ln, stream=s)
        st.run_resident_sets(d_iq, fmt, samples, 0, R, rows_sets, d_records=recs_sets, d_extra=recs_extra, stream=s)
        st.scan_resident(rows_sets, R, recs_again, stream=s)
        torch.cuda.synchronize()
    assert all_plus_zero(rows_ln.cpu().numpy()) and all_plus_zero(rows_sets.cpu().numpy())
    assert all_plus_zero(d_tile.cpu().numpy())
    assert np.isneginf(d_ln.cpu().numpy()).all()
    mm = d_mm.cpu().numpy()
    assert np.isposinf(mm[:, 0]).all() and np.isneginf(mm[:, 1]).all()
    want = se.scan_reference(np.zeros((R, bins), np.float32), bands, bins)
    assert silent_records(want, bands[3])
    for name, d in (("transform with the log", recs_ln), ("transform with sets", recs_sets), ("extra set", recs_extra),
                    ("separate scan", recs_again)):
        got, guard = recs_of(ro, d, R)
        assert guard, name
        assert silent_records(got, bands[3]) and se.same_bits(got, want), (name, got)


@pytest.mark.parametrize("fmt", ["f32", "i16"])
def test_digital_silence_band_only(ro, torch_cuda, fmt):
    torch = torch_cuda
    bins, overlap, R, first, cols = se.E_BAND
    fmt = ro.RO_IQ_F32 if fmt == "f32" else ro.RO_IQ_I16
    samples = bins + (R - 1) * (bins - overlap)
    d_iq = silent_stream(ro, torch, fmt, samples)
    d_band = torch.full((R, cols), 7.0, dtype=torch.float32, device="cuda")
    d_recs = rec_buffer(torch, R)
    with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, se.E_BAND_BANDS)) as st:
        st.band_resident(d_iq, fmt, samples, 0, R, first, cols, d_band, d_records=d_recs, stream=stream_of(torch))
        torch.cuda.synchronize()
    assert all_plus_zero(d_band.cpu().numpy())
    got, guard = recs_of(ro, d_recs, R)
    assert guard and silent_records(got, se.E_BAND_BANDS[3]), got


def test_silence_then_noise(ro, oracle, torch_cuda):
    """silent in its first half: the rows fed by zeros only are exactly zero, the others meet the rows' bar"""
    torch = torch_cuda
    bins, overlap, R = 32768, 24576, 8
    hop = bins - overlap
    samples = bins + (R - 1) * hop
    quiet = 2 * hop + bins                                 # rows 0, 1, 2 read zeros only
    iq = noise_iq(np.random.default_rng(0xE5), samples)
    iq[:quiet] = 0.0
    bands, _ = se.silence_bands(bins)
    d_iq = torch.from_numpy(iq).cuda()
    d_rows = torch.full((R, bins), 7.0, dtype=torch.float32, device="cuda")
    d_recs = rec_buffer(torch, R)
    with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, bands)) as st:
        st.run_resident(d_iq, ro.RO_IQ_F32, samples, 0, R, d_rows, d_records=d_recs, stream=stream_of(torch))
        torch.cuda.synchronize()
    rows = d_rows.cpu().numpy()
    assert all_plus_zero(rows[:3]) and (rows[3:].max(axis=1) > 0).all()
    want = oracle.stft(iq, bins, overlap)
    assert not want[:3].any()
    err = rel_to_row_max(rows[3:], want[3:])
    print("silence then noise: max err / row max %.3e" % err)
    assert err <= 1e-5, err
    got, guard = recs_of(ro, d_recs, R)
    assert guard and silent_records(got[:3], bands[3])
    assert se.same_bits(got, se.scan_reference(rows, bands, bins))
