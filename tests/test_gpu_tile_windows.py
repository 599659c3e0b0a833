"""GPU checks of the tile windows: up to 8 column windows cut from each FULL row (csrc/ro_cut_windows.hip) into the image
layout of ro_stft_band_windows_resident -- what several recorders with their own column range keep of a row
(src/WaterfallBackend.cpp:174-205, :368-374).

The cut is a copy: every comparison of an image with its rows is bit for bit, no tolerance.  Against the oracle the rows
behind the image are held to their family's existing bar (float32 plans: 1e-5 of the row's maximum, tests/test_gpu_stft.py;
RO_PRECISION_F64: every bin within 2e-7 of itself, one float32 ulp, tests/test_gpu_strict.py).  The one tolerance of this
file's own is where the image meets the band call's: both are documented within 1e-5 of the full row's maximum against the
oracle, so they agree within 2e-5 of it."""
import numpy as np
import pytest

from util import add_tone, noise_iq, rel_to_row_max

pytestmark = pytest.mark.gpu

FS = 48000
GUARD = -7                                    # as int32; the bit pattern of a NaN


def columns(windows):
    """row column of every image column"""
    return np.concatenate([np.arange(f, f + n) for f, n in windows])


def offsets(windows):
    return np.concatenate([[0], np.cumsum([n for _, n in windows])]).tolist()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the cut alone -------------------------------------------------------------------------------------------------
def index_rows(torch, rows, row_stride):
    """(rows + 2) x row_stride int32, every cell its own index + 1 (unique per row and column, padding included), to be
    read as float32 bit patterns: a misplaced float shows whichever way it went"""
    return (torch.arange((rows + 2) * row_stride, dtype=torch.int32, device="cuda") + 1).reshape(rows + 2, row_stride)


def cut_and_check(ro, torch, st, bins, rows, windows, row_stride, pad):
    total = sum(n for _, n in windows)
    image_stride = total + pad
    src = index_rows(torch, rows, row_stride)
    before = src.clone()
    image = torch.full((rows + 2, image_stride), GUARD, dtype=torch.int32, device="cuda")      # a guard row either side
    st.cut_windows_resident(src[1:].view(torch.float32), rows, windows, image[1:].view(torch.float32), row_stride=row_stride,
                            image_stride=image_stride, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cols = torch.from_numpy(columns(windows)).cuda()
    assert torch.equal(image[1:rows + 1, :total], src[1:rows + 1][:, cols]), "the image is not rows[:, columns]"
    assert (image[0] == GUARD).all().item() and (image[rows + 1] == GUARD).all().item(), "a guard row was written"
    assert (image[:, total:] == GUARD).all().item(), "floats past the total were written"
    assert torch.equal(src, before), "the rows were written"


def lists_for(bins):
    out = {
        "the whole row": [(0, bins)],
        "eight single columns": [(0, 1), (1, 1), (bins // 3, 1), (bins // 2 - 1, 1), (bins // 2, 1), (bins - 9, 1),
                                 (bins - 2, 1), (bins - 1, 1)],
        "across the middle": [(bins // 2 - 37, 75)],
    }
    if bins >= 4096:
        out["odd widths and offsets, 1024 in all"] = [(1001, 333), (bins // 2 + 77, 691)]
        out["odd widths and offsets, 1025 in all"] = [(1001, 333), (bins // 2 + 77, 692)]
    else:
        out["odd widths and offsets"] = [(3, 33), (bins // 2 + 5, 71)]
    return out


CUT_CASES = [(bins, name) for bins in (256, 32768) for name in lists_for(bins)]


@pytest.mark.parametrize("bins,name", CUT_CASES)
def test_cut_alone(ro, torch_cuda, bins, name):
    windows = lists_for(bins)[name]
    assert ro.tile_windows_supported(bins, windows)
    rows = 9 if bins == 256 else 5
    with ro.Stft(bins=bins, overlap=0) as st:
        cut_and_check(ro, torch_cuda, st, bins, rows, windows, row_stride=bins + 3, pad=3)
        cut_and_check(ro, torch_cuda, st, bins, 1, windows, row_stride=bins, pad=0)


def test_cut_no_rows_writes_nothing(ro, torch_cuda):
    torch = torch_cuda
    with ro.Stft(bins=256, overlap=0) as st:
        src = index_rows(torch, 2, 259)
        image = torch.full((4, 50), GUARD, dtype=torch.int32, device="cuda")
        st.cut_windows_resident(src.view(torch.float32), 0, [(3, 33), (100, 14)], image.view(torch.float32), row_stride=259,
                                image_stride=50)
        torch.cuda.synchronize()
        assert (image == GUARD).all().item()


def test_cut_more_rows_than_a_grid_dimension(ro, torch_cuda):
    """70000 rows of 256 bins: past 65535, the limit of a grid's second and third dimension"""
    with ro.Stft(bins=256, overlap=0) as st:
        cut_and_check(ro, torch_cuda, st, 256, 70000, [(3, 33), (133, 71)], row_stride=259, pad=3)
        cut_and_check(ro, torch_cuda, st, 256, 70001, [(255, 1)], row_stride=256, pad=0)


# ---- behind every plan family --------------------------------------------------------------------------------------
FAMILIES = {
    "float32 single kernel, 256": (256, 192, 9, False),
    "float32 single kernel, 4096": (4096, 2048, 7, False),
    "fused epilogue": (32768, 24576, 5, False),
    "FP64 register kernel": (1024, 512, 5, True),
    "chirp-z": (258, 0, 3, False),
    "four-step": (262144, 131072, 2, False),
    "FP64 through scratch": (131072, 98304, 2, True),
}


def mk(ro, t):
    return ro.Bands(low_noise=t[0], noise_width=t[1], low_detect=t[2], detect_width=t[3], avg_bins=t[4])


@pytest.mark.parametrize("family", list(FAMILIES))
def test_behind_every_plan_family(ro, oracle, torch_cuda, family):
    """run_resident_windows gives the row bits, records and extra records of run_resident_sets; the image is those rows'
    columns; and one row is the oracle's, at the family's bar"""
    torch = torch_cuda
    bins, overlap, nrows, f64 = FAMILIES[family]
    hop = bins - overlap
    prec = ro.RO_PRECISION_F64 if f64 else ro.RO_PRECISION_F32
    primary = (bins // 4, bins // 16, bins // 2, bins // 16, 3)
    sets = [(bins // 8, bins // 32 + 1, bins // 2 + bins // 8, bins // 20, 2), (5, bins // 5, bins // 16, bins // 3, 5)]
    windows = [(3, bins // 8 + 1), (bins // 2 - 5, 11), (bins - 7, 7)]          # an edge run, across the middle, the last columns
    total, stride = sum(n for _, n in windows), bins + 5
    iq = add_tone(noise_iq(np.random.default_rng(bins), bins + (nrows - 1) * hop), 3000.0, 20.0)
    d_iq = torch.from_numpy(iq).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def buffers():
        return (torch.full((nrows, stride), float("nan"), dtype=torch.float32, device="cuda"),
                torch.zeros((nrows, 3), dtype=torch.float32, device="cuda"),
                torch.zeros((nrows, len(sets), 3), dtype=torch.float32, device="cuda"))

    rows_a, recs_a, extra_a = buffers()
    rows_b, recs_b, extra_b = buffers()
    image = torch.full((nrows, total + 3), float("nan"), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, precision=prec, bands=mk(ro, primary), extra_bands=[mk(ro, t) for t in sets]) as st:
        st.run_resident_sets(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, rows_a, row_stride=stride, d_records=recs_a,
                             d_extra=extra_a, stream=s)
        st.run_resident_windows(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, rows_b, windows, image, row_stride=stride,
                                image_stride=total + 3, d_records=recs_b, d_extra=extra_b, stream=s)
        torch.cuda.synchronize()
    a, b, img = rows_a.cpu().numpy(), rows_b.cpu().numpy(), image.cpu().numpy()
    assert np.isfinite(a[:, :bins]).all() and same_bits(a, b)                   # (the stride padding stays NaN in both)
    assert same_bits(recs_a.cpu().numpy(), recs_b.cpu().numpy()) and recs_a.abs().sum().item() > 0
    assert same_bits(extra_a.cpu().numpy(), extra_b.cpu().numpy()) and extra_a.abs().sum().item() > 0
    assert same_bits(img[:, :total], b[:, columns(windows)])
    assert np.isnan(img[:, total:]).all()
    # one row against the oracle at the family's bar, and the image's row with it
    want = oracle.stft(iq, bins, overlap, max_rows=1)
    if f64:
        rel = np.abs(b[:1, :bins].astype(np.float64) - want) / np.maximum(want.astype(np.float64), 1e-300)
        print("%s: per-bin rel err max %.3g" % (family, rel.max()))
        assert rel.max() <= 2e-7
        rel_img = np.abs(img[:1, :total].astype(np.float64) - want[:, columns(windows)]) / want[:, columns(windows)]
        assert rel_img.max() <= 2e-7
    else:
        err = rel_to_row_max(b[:1, :bins], want)
        print("%s: rel-to-row-max err %.3g" % (family, err))
        assert err <= 1e-5
        assert np.abs(img[0, :total].astype(np.float64) - want[0, columns(windows)]).max() <= 1e-5 * want[0].max()


# ---- the same layout as the band call ----------------------------------------------------------------------------
def test_same_layout_as_the_band_call(ro, torch_cuda):
    torch = torch_cuda
    bins, overlap, nrows = 16384, 8192, 4
    windows = [(3000, 300), (9000, 400)]
    total, off = 700, offsets(windows)
    hop = bins - overlap
    iq = noise_iq(np.random.default_rng(16), bins + (nrows - 1) * hop)
    add_tone(iq, (6000.21 - bins / 2) * FS / bins, 300.0, fs=FS)               # a 40 dB carrier between the windows
    for i, (f, n) in enumerate(windows):                                        # a weak tone in the middle of each
        add_tone(iq, (f + n // 2 + 0.37 - bins / 2) * FS / bins, 3.0, fs=FS, phase=0.5 + i)
    d_iq = torch.from_numpy(iq).cuda()
    rows = torch.empty((nrows, bins), dtype=torch.float32, device="cuda")
    cut = torch.zeros((nrows, total), dtype=torch.float32, device="cuda")
    band = torch.zeros((nrows, total), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap) as st:
        st.run_resident_windows(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, rows, windows, cut)
        st.band_windows_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, windows, band)
        torch.cuda.synchronize()
    full, cut, band = rows.cpu().numpy().astype(np.float64), cut.cpu().numpy(), band.cpu().numpy()
    worst = (np.abs(cut.astype(np.float64) - band).max(axis=1) / full.max(axis=1)).max()
    print("cut image against band image: max difference / full row max %.3g" % worst)
    assert worst <= 2e-5
    # the offsets are the same: each window's tone stands at the same image column in both, the one its offset says
    for i, (f, n) in enumerate(windows):
        for r in range(nrows):
            at_cut = off[i] + int(cut[r, off[i]:off[i + 1]].argmax())
            at_band = off[i] + int(band[r, off[i]:off[i + 1]].argmax())
            assert at_cut == at_band and abs(at_cut - (off[i] + n // 2)) <= 1, (i, r, at_cut, at_band)


# ---- streaming -----------------------------------------------------------------------------------------------------
def push_all(st, iq, cuts):
    """the samples in uneven calls, a flush, then everything that waits"""
    at = 0
    for n in cuts:
        st.push(iq[at:at + n])
        at += n
    st.push(iq[at:])
    return st.flush()


def stream_check(ro, bins, overlap, batch, nrows, cuts, windows):
    hop = bins - overlap
    total = sum(n for _, n in windows)
    bands = mk(ro, (bins // 4, bins // 16, bins // 2, bins // 16, 3))
    iq = add_tone(noise_iq(np.random.default_rng(bins + nrows), bins + (nrows - 1) * hop + hop // 2), 3000.0, 20.0)
    with ro.Stft(bins=bins, overlap=overlap, max_batch_rows=batch, bands=bands) as plain:
        assert push_all(plain, iq, cuts) == nrows
        first_p, rows_p, recs_p = plain.fetch(nrows + 5)
    assert first_p == 0 and rows_p.shape == (nrows, bins) and rows_p.max() > 0
    want = rows_p[:, columns(windows)]
    with ro.Stft(bins=bins, overlap=overlap, max_batch_rows=batch, bands=bands) as st:
        assert st.tile_windows == []
        st.set_tile_windows(windows)
        assert [(w.first_col, w.cols) for w in st.tile_windows] == list(windows) and st.image_cols == total
        assert push_all(st, iq, cuts) == nrows
        first, image, recs = st.fetch(nrows + 5)                       # the default columns: the whole image
        assert first == 0 and same_bits(image, want)
        assert recs.tobytes() == recs_p.tobytes()                       # the full row's records, in row coordinates
        # a sub-range in IMAGE columns, fetched batch by batch: the row indices follow the stream
        st.reset()
        assert push_all(st, iq, cuts) == nrows
        got, firsts = [], []
        while True:
            f, part, _ = st.fetch(batch, first_col=5, cols=total - 9)
            if len(part) == 0:
                break
            firsts.append(f)
            got.append(part)
        assert firsts == list(range(0, nrows, batch))
        assert same_bits(np.concatenate(got), want[:, 5:total - 4])
        # without the windows the next stream brings full rows again
        st.reset()
        st.set_tile_windows([])
        assert st.tile_windows == [] and st.image_cols == 0
        assert push_all(st, iq, cuts) == nrows
        first, rows, recs = st.fetch(nrows + 5)
        assert first == 0 and same_bits(rows, rows_p) and recs.tobytes() == recs_p.tobytes()


def test_streaming_three_batch_boundaries_and_a_flush(ro, torch_cuda):
    # 10 rows in batches of 3: three full batches (completed in the 2nd, the 4th and the last call) and one row left to the flush
    stream_check(ro, 4096, 3072, 3, 10, cuts=(1000, 5500, 77, 3000, 2100), windows=((1001, 333), (2048 + 77, 692)))


def test_streaming_fused_plan(ro, torch_cuda):
    stream_check(ro, 32768, 24576, 3, 4, cuts=(40000, 1234), windows=((22528, 409), (23278, 615)))


# ---- refusals --------------------------------------------------------------------------------------------------------
def refused(ro, code, word, call, *args, **kw):
    with pytest.raises(ro.StftError) as e:
        call(*args, **kw)
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)


def test_refusals(ro, torch_cuda):
    torch = torch_cuda
    bins, overlap, batch = 4096, 3072, 3
    good = [(100, 50), (1000, 70)]
    iq = noise_iq(np.random.default_rng(5), bins + 2 * (bins - overlap))          # one full batch
    with ro.Stft(bins=bins, overlap=overlap, max_batch_rows=batch) as st:
        assert st.push(iq) == batch
        refused(ro, -5, "idle stream", st.set_tile_windows, good)                 # rows wait to be fetched
        st.fetch(batch)
        st.push(iq[:100])
        refused(ro, -5, "idle stream", st.set_tile_windows, good)                 # samples are staged
        st.reset()
        refused(ro, -1, "window 1", st.set_tile_windows, [(100, 50), (149, 70)])
        refused(ro, -1, "1 ... 8 windows", st.set_tile_windows, [(10 * i, 5) for i in range(9)])
        assert st.tile_windows == []
        # a sink and windows refuse each other, whichever comes second
        ring = ro.PinnedArray(2 * batch, bins)
        st.set_row_sink(ring.array)
        refused(ro, -5, "row sink", st.set_tile_windows, good)
        st.set_row_sink(None)
        st.set_tile_windows(good)
        refused(ro, -5, "tile windows", st.set_row_sink, ring.array)
        # fetch counts in image columns
        for first_col, cols in ((0, 121), (-1, 5), (120, 1), (100, 50)):
            refused(ro, -1, "image columns", st.fetch, 1, first_col=first_col, cols=cols)
        st.fetch(1, first_col=119, cols=1)
        refused(ro, -5, "tile_ln", fetch_ln_raw, ro, st)
        ring.close()
        # the resident calls
        d_rows = torch.zeros((2, bins), dtype=torch.float32, device="cuda")
        d_image = torch.full((2, 120), 5.5, dtype=torch.float32, device="cuda")
        d_iq = torch.from_numpy(iq).cuda()
        refused(ro, -1, "image_stride", st.cut_windows_resident, d_rows, 2, good, d_image, image_stride=119)
        refused(ro, -1, "image_stride", st.run_resident_windows, d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 2, d_rows, good, d_image,
                image_stride=119)
        refused(ro, -1, "window 1, columns [4090,+7)", st.cut_windows_resident, d_rows, 2, [(5, 5), (4090, 7)], d_image)
        refused(ro, -1, "window 0", st.run_resident_windows, d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 2, d_rows, [(5, 0)], d_image)
        refused(ro, -1, "null", st.cut_windows_resident, None, 2, good, d_image)
        refused(ro, -1, "null", st.cut_windows_resident, d_rows, 2, good, None)
        refused(ro, -1, "null", st.run_resident_windows, d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 2, d_rows, good, None)
        refused(ro, -1, "d_rows", st.run_resident_windows, d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 2, None, good, d_image)
        refused(ro, -1, "row_stride", st.cut_windows_resident, d_rows, 2, good, d_image, row_stride=bins - 1)
        st.run_resident_windows(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 0, d_rows, good, d_image)      # no rows: RO_OK, nothing written
        torch.cuda.synchronize()
        assert (d_image == 5.5).all().item()
    for kw in (dict(tile=(100, 200)), dict(tile=(100, 200), tile_ln=True)):
        with ro.Stft(bins=bins, overlap=overlap, **kw) as st:
            refused(ro, -2, "without a tile", st.set_tile_windows, good)
            # ... while the resident call serves such a handle: its tile is simply not produced
            d_rows = torch.zeros((2, bins), dtype=torch.float32, device="cuda")
            d_image = torch.zeros((2, 120), dtype=torch.float32, device="cuda")
            d_iq = torch.from_numpy(iq).cuda()
            st.run_resident_windows(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 2, d_rows, good, d_image)
            torch.cuda.synchronize()
            assert same_bits(d_image.cpu().numpy(), d_rows.cpu().numpy()[:, columns(good)]) and d_image.max().item() > 0


def fetch_ln_raw(ro, st):
    """ro_stft_fetch_ln on a handle without tile_ln: refused as ever, windows or not"""
    import ctypes as C
    got = C.c_int64()
    rc = ro.library().ro_stft_fetch_ln(st._h, 1, None, None, None, None, None, C.byref(got))
    if rc != 0:
        raise ro.StftError(rc, (ro.library().ro_last_error() or b"").decode())
