"""GPU parity of several band sets per row (ro_stft_set_extra_bands, csrc/ro_scan_sets.hip): every extra set's record is
BolidRecorder::noise / peak / average over ITS bands (src/BolidRecorder.cpp:84-104, :121-132, :313-347) as restated by
the oracle, one oracle scan per set.  Integer / index work and exact float results: bit-exact on all three fields."""
import numpy as np
import pytest

from util import add_chirp, add_tone, noise_iq

pytestmark = pytest.mark.gpu

A_FREQS = (10300.0, 10900.0, 9000.0, 9600.0)            # radio-observer.json:62-87
B_FREQS = (5300.0, 5900.0, 4000.0, 4600.0)


def mk(ro, t):
    """(low_noise, noise_width, low_detect, detect_width, avg_bins) -> ro.Bands"""
    return ro.Bands(low_noise=t[0], noise_width=t[1], low_detect=t[2], detect_width=t[3], avg_bins=t[4])


def inside(t, bins):
    """the averaging window stays in the row whatever the peak, as in tests/test_gpu_scan.py"""
    return t[2] >= t[4] and t[2] + t[3] + t[4] <= bins and t[0] >= 0 and t[0] + t[1] <= bins


def recs_of(ro, d, shape):
    return d.cpu().numpy().view(ro.capi.SCAN_DTYPE).reshape(shape)


def same_bits(got, want):
    return all(np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)) for f in ("noise", "peak", "average"))


def oracle_recs(ro, oracle, rows, sets):
    """[rows, len(sets)] records: one oracle.scan_rows call per set"""
    out = np.zeros((rows.shape[0], len(sets)), ro.capi.SCAN_DTYPE)
    for s, t in enumerate(sets):
        assert inside(t, rows.shape[1]), t
        n, p, a = oracle.scan_rows(rows, t[0], t[1], t[2], t[3], t[4])
        out["noise"][:, s], out["peak"][:, s], out["average"][:, s] = n, p, a
    return out


def scan_sets_gpu(ro, torch, st, d_rows, rows, count, guard=0, d_records=None):
    d_extra = torch.full(((rows + guard) * count, 3), 12345.0, dtype=torch.float32, device="cuda")
    st.scan_sets_resident(d_rows, rows, d_extra, d_records=d_records, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return recs_of(ro, d_extra, (rows + guard, count))


def check_sets(ro, oracle, torch, rows, primary, sets, guard=0):
    d_rows = torch.from_numpy(rows).cuda()
    with ro.Stft(bins=rows.shape[1], overlap=0, bands=mk(ro, primary), extra_bands=[mk(ro, t) for t in sets]) as st:
        assert [tuple(getattr(b, f) for f, _ in ro.Bands._fields_) for b in st.extra_bands] == [tuple(t) for t in sets]
        got = scan_sets_gpu(ro, torch, st, d_rows, rows.shape[0], len(sets), guard)
    assert same_bits(got[:rows.shape[0]], oracle_recs(ro, oracle, rows, sets))
    return got


@pytest.mark.parametrize("nrows", [1, 5])
def test_smallest_row_and_ragged_grid(ro, oracle, torch_cuda, nrows):
    """256 bins, widths 1 ... the whole row; rows x count is no multiple of a workgroup's four waves, and the records
    behind the last one stay what they were"""
    sets = [(0, 1, 8, 1, 1), (10, 3, 20, 3, 3), (64, 64, 130, 65, 5), (0, 256, 100, 100, 7)]
    rows = np.abs(np.random.default_rng(nrows).standard_normal((nrows, 256))).astype(np.float32)
    got = check_sets(ro, oracle, torch_cuda, rows, sets[1], sets, guard=1)
    sentinel = got[nrows:]
    assert (sentinel["noise"] == 12345.0).all() and (sentinel["average"] == 12345.0).all()
    assert (sentinel["peak"].view(np.float32) == 12345.0).all()


def test_all_three_register_forms_in_one_launch(ro, oracle, torch_cuda):
    """bands of up to 1024, up to 4096 and more columns side by side (the launch takes the widest's form), and each set
    alone (its own form) gives the same bits"""
    bins = 16384
    sets = [(100, 1024, 2000, 777, 27), (1500, 1025, 9000, 64, 2), (5000, 4096, 10000, 4096, 5), (12000, 4097, 300, 100, 5)]
    rows = np.abs(np.random.default_rng(16).standard_normal((9, bins))).astype(np.float32)
    together = check_sets(ro, oracle, torch_cuda, rows, sets[0], sets)
    for s, t in enumerate(sets):
        alone = check_sets(ro, oracle, torch_cuda, rows, sets[0], [t])
        assert same_bits(alone[:, 0], together[:, s])


def test_seven_sets(ro, oracle, torch_cuda):
    bins, rng = 4096, np.random.default_rng(7)
    sets = []
    for _ in range(7):
        nw, dw, avg = int(rng.integers(1, 700)), int(rng.integers(1, 700)), int(rng.integers(1, 40))
        sets.append((int(rng.integers(0, bins - nw + 1)), nw, int(rng.integers(avg, bins - dw - avg + 1)), dw, avg))
    rows = np.abs(rng.standard_normal((33, bins))).astype(np.float32)
    check_sets(ro, oracle, torch_cuda, rows, sets[0], sets)


def json_tuple(oracle, bins=32768, overlap=24576, freqs=A_FREQS):
    b = oracle.bolid_bands(bins, 48000, overlap, freqs[0], freqs[1], freqs[2], freqs[3], 2, 5, 40)
    return (b.low_noise, b.noise_width, b.low_detect, b.detect_width, b.avg_bins)


def tie_rows(rng, n, bins, low_detect, detect_width, value=7.5):
    rows = rng.random((n, bins)).astype(np.float32)
    for r in range(n):
        rows[r, low_detect + rng.choice(detect_width, size=1 + r % 5, replace=False)] = value
    return rows


@pytest.mark.parametrize("bins,band", [(32768, None), (65536, (1000, 3000, 30000, 3000, 9))])
def test_ties_and_duplicates_in_an_extra_set(ro, oracle, torch_cuda, bins, band):
    """the recipes of test_scan_ties_take_last_index and test_scan_duplicates_and_quartile_index on an extra set; an
    extra set equal to the primary gives the primary's bits"""
    torch = torch_cuda
    t = band or json_tuple(oracle)
    rng = np.random.default_rng(bins)
    batches = [tie_rows(rng, 16, bins, t[2], t[3]),
               rng.integers(0, 6, size=(16, bins)).astype(np.float32),
               (rng.standard_normal((16, bins)) * 1e-3).astype(np.float32),
               np.full((4, bins), 3.25, np.float32)]
    with ro.Stft(bins=bins, overlap=0, bands=mk(ro, t), extra_bands=[mk(ro, t)]) as st:
        for rows in batches:
            d_rows = torch.from_numpy(rows).cuda()
            d_recs = torch.zeros((rows.shape[0], 3), dtype=torch.float32, device="cuda")
            extra = scan_sets_gpu(ro, torch, st, d_rows, rows.shape[0], 1, d_records=d_recs)[:, 0]
            primary = recs_of(ro, d_recs, -1)
            assert same_bits(extra, primary)
            assert same_bits(extra, oracle_recs(ro, oracle, rows, [t])[:, 0])
    for r in range(16):                                   # ties go to the highest index (src/BolidRecorder.cpp:329-332)
        bandv = batches[0][r, t[2]:t[2] + t[3]]
        assert oracle_recs(ro, oracle, batches[0][r:r + 1], [t])["peak"][0, 0] == np.flatnonzero(bandv == bandv.max()).max()


@pytest.mark.parametrize("bins,overlap,nrows,f64", [(32768, 24576, 8, False), (256, 128, 5, False), (1024, 512, 5, True),
                                                    (258, 0, 3, False), (262144, 0, 2, False)])
def test_every_transform_family_through_run_resident_sets(ro, oracle, torch_cuda, bins, overlap, nrows, f64):
    """fused epilogue, small single-pass, FP64 register kernel, chirp-z, four-step: rows and primary records are what a
    handle without extra sets gives, the extra records are the scan of the rows written"""
    torch = torch_cuda
    hop = bins - overlap
    prec = ro.RO_PRECISION_F64 if f64 else ro.RO_PRECISION_F32
    primary = (bins // 4, bins // 16, bins // 2, bins // 16, 3)
    sets = [(bins // 8, bins // 32 + 1, bins // 2 + bins // 8, bins // 20, 2), (5, bins // 5, bins // 16, bins // 3, 5)]
    iq = add_tone(noise_iq(np.random.default_rng(bins), bins + (nrows - 1) * hop), 3000.0, 2.0)
    d_iq = torch.from_numpy(iq).cuda()
    s = torch.cuda.current_stream().cuda_stream

    def run(extra):
        d_rows = torch.zeros((nrows, bins), dtype=torch.float32, device="cuda")
        d_recs = torch.zeros((nrows, 3), dtype=torch.float32, device="cuda")
        d_extra = torch.zeros((nrows * 2, 3), dtype=torch.float32, device="cuda") if extra else None
        with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, primary), precision=prec,
                     extra_bands=[mk(ro, t) for t in sets] if extra else None) as st:
            if extra:
                st.run_resident_sets(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, d_rows, d_records=d_recs, d_extra=d_extra, stream=s)
                torch.cuda.synchronize()
                again = scan_sets_gpu(ro, torch, st, d_rows, nrows, 2)
            else:
                st.run_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, d_rows, d_records=d_recs, stream=s)
                torch.cuda.synchronize()
                again = None
        return d_rows.cpu().numpy(), recs_of(ro, d_recs, -1), recs_of(ro, d_extra, (nrows, 2)) if extra else None, again

    rows0, recs0, _, _ = run(False)
    rows1, recs1, extra, again = run(True)
    assert np.array_equal(rows0.view(np.uint32), rows1.view(np.uint32))
    assert same_bits(recs0, recs1)
    assert same_bits(extra, again)
    assert same_bits(extra, oracle_recs(ro, oracle, rows1, sets))
    assert same_bits(recs1, oracle_recs(ro, oracle, rows1, [primary])[:, 0])


@pytest.mark.parametrize("sink", [False, True])
def test_streaming_fetch_sets_equals_one_resident_run(ro, oracle, torch_cuda, sink):
    """64 rows in batches of 4, pushed 700 samples at a time; with a row sink every slot's batch runs as a captured graph
    (16 batches over 3 slots: one plain, then the graph four or five times each).  All three sets' records are those of
    ONE run_resident_sets over the stream."""
    torch = torch_cuda
    bins, overlap, hop, nrows, batch = 1024, 512, 512, 64, 4
    primary = (100, 60, 700, 50, 5)
    sets = [(300, 33, 200, 64, 3), (0, 128, 850, 100, 7)]
    iq = add_tone(noise_iq(np.random.default_rng(0x5E), bins + (nrows - 1) * hop), 9000.0, 3.0)
    d_iq = torch.from_numpy(iq).cuda()
    d_rows = torch.zeros((nrows, bins), dtype=torch.float32, device="cuda")
    d_recs = torch.zeros((nrows, 3), dtype=torch.float32, device="cuda")
    d_extra = torch.zeros((nrows * 2, 3), dtype=torch.float32, device="cuda")
    extra_bands = [mk(ro, t) for t in sets]
    with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, primary), extra_bands=extra_bands) as ref:
        ref.run_resident_sets(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, nrows, d_rows, d_records=d_recs, d_extra=d_extra,
                              stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    want_recs, want_extra = recs_of(ro, d_recs, -1), recs_of(ro, d_extra, (nrows, 2))
    assert same_bits(want_extra, oracle_recs(ro, oracle, d_rows.cpu().numpy(), sets))
    pinned = ro.PinnedArray(16, bins) if sink else None
    with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, primary), max_batch_rows=batch, extra_bands=extra_bands) as st:
        if sink:
            st.set_row_sink(pinned.array)
        got_recs, got_extra, seen = [], [], 0

        def take():
            nonlocal seen
            while True:
                first, rows, recs, extra = st.fetch_sets(8)
                if len(recs) == 0:
                    return
                assert first == seen and extra.shape == (len(recs), 2) and (rows is None) == sink
                seen += len(recs)
                got_recs.append(recs.copy())
                got_extra.append(extra.copy())

        for at in range(0, iq.shape[0], 700):
            st.push(iq[at:at + 700])
            take()
        st.flush()
        take()
        assert seen == nrows
        assert same_bits(np.concatenate(got_recs), want_recs)
        assert same_bits(np.concatenate(got_extra), want_extra)
        # without the sets again: the handle streams as it always has, and there are no extra records to ask for
        st.reset()
        st.set_extra_bands([])
        assert st.extra_bands == []
        for at in range(0, bins + 11 * hop, 700):
            st.push(iq[at:min(at + 700, bins + 11 * hop)])
        st.flush()
        with pytest.raises(ro.StftError) as e:
            st.fetch_sets(100)
        assert e.value.code == -5
        first, rows, recs, extra = st.fetch_sets(100, want_extra=False)
        assert first == 0 and extra is None and len(recs) == 12 and same_bits(recs, want_recs[:12])


def test_refusals_leave_the_handle_working(ro, oracle, torch_cuda):
    torch = torch_cuda
    bins = 1024
    good, other = (100, 60, 700, 50, 5), (300, 33, 200, 64, 3)
    rows = np.abs(np.random.default_rng(3).standard_normal((6, bins))).astype(np.float32)
    d_rows = torch.from_numpy(rows).cuda()

    def still_works(st, sets):
        got = scan_sets_gpu(ro, torch, st, d_rows, 6, len(sets))
        assert same_bits(got, oracle_recs(ro, oracle, rows, sets))

    with ro.Stft(bins=bins, overlap=512, bands=mk(ro, good), max_batch_rows=2, extra_bands=[mk(ro, other)]) as st:
        with pytest.raises(ro.StftError) as e:
            st.set_extra_bands([mk(ro, other)] * 8)                          # count = 8
        assert e.value.code == -1
        still_works(st, [other])
        with pytest.raises(ro.StftError) as e:
            st.set_extra_bands([mk(ro, other), mk(ro, (0, 10, 1000, 25, 3)), mk(ro, good)])     # set 1 leaves the row
        assert e.value.code == -1 and "extra band set 1" in str(e.value) and "detect band" in str(e.value)
        still_works(st, [other])
        iq = noise_iq(np.random.default_rng(4), bins + 3 * 512)
        st.push(iq)
        st.flush()
        with pytest.raises(ro.StftError) as e:
            st.set_extra_bands([mk(ro, good)])                               # rows wait to be fetched
        assert e.value.code == -5
        first, got_rows, recs, extra = st.fetch_sets(10)
        assert first == 0 and len(recs) == 4 and same_bits(extra, oracle_recs(ro, oracle, got_rows, [other]))
        with pytest.raises(ro.StftError) as e:
            st.set_extra_bands([mk(ro, good)])                               # samples short of a row are still staged
        assert e.value.code == -5
        st.reset()
        st.set_extra_bands([mk(ro, good), mk(ro, other)])
        still_works(st, [good, other])
        st.set_extra_bands([])
        d_iq = torch.from_numpy(iq).cuda()
        d_out = torch.zeros((4, bins), dtype=torch.float32, device="cuda")
        d_extra = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(ro.StftError) as e:
            st.run_resident_sets(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 4, d_out, d_extra=d_extra)   # no sets
        assert e.value.code == -5
        st.run_resident_sets(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 4, d_out)                         # = run_resident
        d_out2 = torch.zeros((4, bins), dtype=torch.float32, device="cuda")
        st.run_resident(d_iq, ro.RO_IQ_F32, iq.shape[0], 0, 4, d_out2)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), d_out2.cpu().numpy().view(np.uint32))
        assert np.abs(d_out.cpu().numpy() - got_rows).max() <= 1e-5 * got_rows.max()
    with ro.Stft(bins=bins, overlap=512) as st:                              # no primary
        with pytest.raises(ro.StftError) as e:
            st.set_extra_bands([mk(ro, good)])
        assert e.value.code == -5
        st.set_bands(mk(ro, good))
        st.set_extra_bands([mk(ro, other)])
        still_works(st, [other])


_pipeline_reference = {}


def pipeline_signal(oracle):
    """the signal of test_bolid_detection_through_the_pipeline plus two chirps in detector B's band; the oracle's rows
    and both detectors' scans of them, computed once"""
    if not _pipeline_reference:
        bins, overlap, hop, rows = 32768, 24576, 8192, 120
        rng = np.random.default_rng(0xC4)
        iq = noise_iq(rng, bins + (rows - 1) * hop)
        add_chirp(iq, 20 * hop, 2.0, 10800.0, -100.0, 3.0)
        add_chirp(iq, 70 * hop + 1234, 1.0, 10700.0, -100.0, 3.0)
        add_chirp(iq, 14 * hop + 77, 1.5, 5800.0, -100.0, 3.0)
        add_chirp(iq, 55 * hop, 1.0, 5500.0, 80.0, 3.0)
        want = oracle.stft(iq, bins, overlap)
        scans = []
        for freqs in (A_FREQS, B_FREQS):
            t = json_tuple(oracle, freqs=freqs)
            scans.append(oracle.scan_rows(want, t[0], t[1], t[2], t[3], t[4]))
        _pipeline_reference.update(iq=iq, scans=scans)
    return _pipeline_reference["iq"], _pipeline_reference["scans"]


def fsm_replay(oracle, bins, overlap, freqs, cap, n, pk, a):
    b = oracle.bolid_bands(bins, 48000, overlap, freqs[0], freqs[1], freqs[2], freqs[3], 2, 5, 40)
    rate = oracle.lib().ro_oracle_fft_sample_rate(48000, bins, overlap)
    fsm = oracle.BolidFsm(b.advance, b.jitter, rate, 48000, freqs[0], freqs[1])
    out = []
    for r in range(len(n)):
        ev = fsm.update(n[r], a[r], oracle.lib().ro_oracle_bin_to_frequency(bins, 48000, b.low_detect + int(pk[r])), (r + 1) % cap)
        if ev.fired:
            out.append((r, ev.snap_start, ev.snap_length, ev.raw_length, ev.peak_freq, ev.fmin, ev.fmax))
    return out, fsm.f.state


@pytest.mark.parametrize("f64", [False, True])
def test_two_detectors_through_the_pipeline(ro, oracle, torch_cuda, f64):
    """Frontend -> HipWaterfallBackend -> two BolidRecorders with their own bands: each detector's events are the
    oracle's FSM on the oracle's scan of ITS bands (A fires at rows 59 and 104, B at rows 51 and 89), and its event
    frequencies are those of the FSM on the records ro_stft_fetch_sets hands out for the same samples and batch size"""
    from detectorslib import DetectorPipeline
    bins, overlap, rows = 32768, 24576, 120
    prec = ro.RO_PRECISION_F64 if f64 else ro.RO_PRECISION_F32
    iq, scans = pipeline_signal(oracle)
    z = iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)
    p = DetectorPipeline(bins, overlap, [A_FREQS, B_FREQS], precision=prec, max_batch_rows=16)
    for i in range(0, len(z), 4096):
        p.process(z[i:i + 4096])
    p.end()
    assert p.error == "" and p.rows == rows
    assert p.bands(0) == (23415, 410, 22528, 409, 11, 29, 27, 0)
    assert p.bands(1) == (20002, 409, 19114, 410, 11, 29, 27, 1)
    cap = p.ring_capacity()
    got = [[(e.row, e.start, e.length, e.rawLength, e.peakFreq, e.fmin, e.fmax) for e in p.events(i)] for i in range(2)]
    states = [p.state(0), p.state(1)]
    p.close()
    # no row of either detector is marginal: float32 rounding cannot move an event
    for n, pk, a in scans:
        assert np.abs(a.astype(np.float64) / (2 * n.astype(np.float64)) - 1).min() > 0.027
    # the records of the same stream through the C ABI
    tA, tB = json_tuple(oracle, freqs=A_FREQS), json_tuple(oracle, freqs=B_FREQS)
    with ro.Stft(bins=bins, overlap=overlap, bands=mk(ro, tA), extra_bands=[mk(ro, tB)], max_batch_rows=16, precision=prec) as st:
        recs, extra = [], []
        for i in range(0, len(z), 4096):
            st.push(z[i:i + 4096])
        st.flush()
        while True:
            first, _, r, e = st.fetch_sets(64, want_rows=False)
            if len(r) == 0:
                break
            recs.append(r.copy())
            extra.append(e[:, 0].copy())
    fetched = [np.concatenate(recs), np.concatenate(extra)]
    assert len(fetched[0]) == rows and len(fetched[1]) == rows
    for i, (freqs, fired) in enumerate(((A_FREQS, [59, 104]), (B_FREQS, [51, 89]))):
        n, pk, a = scans[i]
        want, state = fsm_replay(oracle, bins, overlap, freqs, cap, n, pk, a)
        assert [w[0] for w in want] == fired
        assert [g[:4] for g in got[i]] == [w[:4] for w in want]          # row, start, length, raw length
        assert states[i] == state
        mine, _ = fsm_replay(oracle, bins, overlap, freqs, cap, fetched[i]["noise"], fetched[i]["peak"], fetched[i]["average"])
        assert got[i] == mine                                            # ... and peakFreq, fmin, fmax from its own records
    assert got[0] != got[1]
