"""GPU: WaterfallConfig::precision = RO_PRECISION_F64 behind the reference's interface -- Frontend -> Backend::process
(vector<Complex>, two doubles per sample) -> HipWaterfallBackend -> Recorder::update -- through the test-only shim
tests/harness_precision/ (tests/precisionlib.py).  The rows are the reference's own arithmetic (src/FFTBackend.cpp:
117-120,229-236): every bin within one float32 ulp of the oracle's FP64 rows; everything that is not arithmetic (row
stamps, raw marks, the raw I/Q ring, detector events, file headers) equals the float32 mode's."""
import numpy as np
import pytest

import precisionlib as P
from util import add_chirp, add_tone, noise_iq

pytestmark = pytest.mark.gpu

F32, F64 = P.RO_PRECISION_F32, P.RO_PRECISION_F64
ONE_ULP = 2e-7


@pytest.fixture(autouse=True)
def _need_shim():
    assert P.precision_library() is not None, \
        "tests/harness_precision/libro_precision_harness.so missing: run __graft_entry__.build()"


def per_bin(got, want):
    """|got - want| / want per bin (tests/test_gpu_strict.py's measure)"""
    want = want.astype(np.float64)
    return np.abs(got.astype(np.float64) - want) / np.maximum(want, 1e-300)


def c3_doubles(rng, samples, fs=48000):
    """C3's signal model in true doubles: sigma = 1 noise plus a 30 sigma CW carrier at 10.6 kHz, plus 1e-9 offsets --
    low-order bits a float32 cannot hold"""
    z = rng.standard_normal(samples) + 1j * rng.standard_normal(samples)
    t = np.arange(samples, dtype=np.float64)
    z += 30.0 * np.exp(2j * np.pi * 10600.0 * t / fs)
    z += 1e-9 * (1 + 1j) * np.where(t % 3 == 0, 1.0, -1.0)
    return z


def cards_but_date(cards):
    """a FITS header's cards less DATE (the file's creation time, FITSWriter::date: the wall clock)"""
    return [c for c in cards if c[:8].strip() != "DATE"]


def feed(p, z, calls):
    at, i = 0, 0
    while at < len(z):
        n = calls[i % len(calls)]
        p.process(z[at:at + n])
        at += n
        i += 1
    p.end()


@pytest.mark.parametrize("bins,overlap", [(32768, 24576), (1024, 512), (65536, 49152)])
def test_f64_stream_per_bin_true_doubles(oracle, bins, overlap):
    """~60 rows of C3's model through Backend::process at the latency-bound default batch: every bin of every FP64 row
    within one float32 ulp of the oracle on the same doubles, relative to that bin.  (The float32 mode misses 1e-5 on
    ~2.5 % of these bins.)  1024 bins: the register kernel batches rows per workgroup; 65536: D = 4."""
    rng = np.random.default_rng(bins + 0xF64)
    hop = bins - overlap
    R = 60
    z = c3_doubles(rng, bins + (R - 1) * hop + hop // 2)
    p = P.PrecisionPipeline(bins, overlap, F64, start=(1700000000, 0))
    assert p.precision() == F64
    assert p.ring_capacity() > R
    feed(p, z, [4096])
    assert p.error == "" and p.rows == R
    got = p.newest_rows(R)
    want = oracle.stft(z, bins, overlap)
    assert want.shape == got.shape
    e = per_bin(got, want)
    print("FP64 through Backend::process, %d bins: per-bin rel err max %.3g, bit-identical floats %.4f"
          % (bins, e.max(), (got == want).mean()))
    assert e.max() <= ONE_ULP
    p.close()


def test_f64_rows_times_marks_and_raw_ring_equal_f32(oracle):
    """Odd call sizes, then one long call on a ring that wraps: DataInfo (offset, time) and rawMark of every row, the
    raw handles and the raw I/Q ring itself (float pairs in both modes, src/FFTBackend.cpp:217-223) equal the float32
    run's for the same stream; the FP64 rows are the oracle's per bin."""
    bins, overlap, hop = 4096, 3072, 1024
    rng = np.random.default_rng(0xB1)
    R = 1500
    T = bins + (R - 1) * hop + 17
    z = rng.standard_normal(T) + 1j * rng.standard_normal(T) + 1e-9
    start = (1700000000, 250000)
    odd = [1, 7, 333, 1023, 4097, 20011]
    runs = {}
    for prec in (F32, F64):
        p = P.PrecisionPipeline(bins, overlap, prec, start=start, snapshot_length=1)
        cap = p.ring_capacity()
        assert R > 3 * cap, (R, cap)                            # the ring wraps more than three times
        head = 60000
        at, i = 0, 0
        while at < head:                                        # odd call sizes ...
            n = min(odd[i % len(odd)], head - at)
            p.process(z[at:at + n])
            at += n
            i += 1
        p.process(z[head:])                                     # ... then the rest in ONE call
        p.end()
        assert p.error == "" and p.rows == R
        runs[prec] = dict(info=[p.row_info(i) for i in range(R)],
                          handles=[p.raw_handle(m) for m in range(cap)],
                          raw=p.raw_ring(), raw_mark=p.raw_mark(), mark=p.ring_mark(),
                          rows=p.newest_rows(min(cap - 1, 64)))
        p.close()
    a, b = runs[F32], runs[F64]
    assert a["info"] == b["info"]
    assert a["handles"] == b["handles"]
    assert a["mark"] == b["mark"] and a["raw_mark"] == b["raw_mark"]
    assert a["raw"].shape == b["raw"].shape and a["raw"].tobytes() == b["raw"].tobytes()
    o = oracle.Stream(bins, overlap, start=start)
    want_info = []
    at, i = 0, 0
    while at < 60000:
        n = min(odd[i % len(odd)], 60000 - at)
        want_info += o.process(z[at:at + n])[1]
        at += n
        i += 1
    want_info += o.process(z[60000:])[1]
    assert [x[:3] for x in b["info"]] == [x[:3] for x in want_info]     # offset and time: the oracle's
    keep = b["rows"].shape[0]
    want = oracle.stft(z, bins, overlap, first_row=R - keep)
    assert per_bin(b["rows"], want).max() <= ONE_ULP


def test_f64_bolid_detection_snapshots_and_raw_captures(oracle, tmp_path):
    """C4 (test_bolid_detection_through_the_pipeline's chirps) in FP64, with the detector writing its files: events
    equal the oracle FSM on the oracle's rows and the float32 pipeline's events; the band snapshots are the oracle's rows
    per bin; the raw I/Q captures are byte-identical to the float32 run's."""
    from test_host_cpu import read_fits
    bins, overlap, hop = 32768, 24576, 8192
    rng = np.random.default_rng(0xC4)
    rows = 120
    iq = noise_iq(rng, bins + (rows - 1) * hop)
    add_chirp(iq, 20 * hop, 2.0, 10800.0, -100.0, 3.0)
    add_chirp(iq, 70 * hop + 1234, 1.0, 10700.0, -100.0, 3.0)
    z = iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)
    res = {}
    for prec, name in ((F32, "f32"), (F64, "f64")):
        d = tmp_path / name
        d.mkdir()
        p = P.PrecisionPipeline(bins, overlap, prec, start=(1700000000, 0), max_batch_rows=16, snapshot_length=60,
                                out_dir=d)
        p.set_clock(1700000000, 0)
        for i in range(0, len(z), 4096):
            p.process(z[i:i + 4096])
        p.end()
        assert p.error == "" and p.rows == rows
        res[prec] = dict(bands=p.bands(), cap=p.ring_capacity(), state=p.state(),
                         events=[(e.row, e.start, e.length, e.rawLength, e.duration, e.peakFreq, e.fmin, e.fmax)
                                 for e in p.events()],
                         blid=[read_fits(f) for f in p.files(1)], raws=[read_fits(f) for f in p.files(2)])
        p.close()
    f32, f64 = res[F32], res[F64]
    assert f64["bands"] == f32["bands"] == [23415, 410, 22528, 409, 11, 29, 27]
    ld, dw, ln, nw, adv, jit, avg = f64["bands"]
    want = oracle.stft(iq, bins, overlap)
    n, pk, a = oracle.scan_rows(want, ln, nw, ld, dw, avg)
    rate = oracle.lib().ro_oracle_fft_sample_rate(48000, bins, overlap)
    fsm = oracle.BolidFsm(adv, jit, rate, 48000, 10300.0, 10900.0)
    expect = []
    for r in range(rows):
        ev = fsm.update(n[r], a[r], oracle.lib().ro_oracle_bin_to_frequency(bins, 48000, ld + int(pk[r])),
                        (r + 1) % f64["cap"])
        if ev.fired:
            expect.append((r, ev.snap_start, ev.snap_length, ev.raw_length, ev.duration_s, ev.peak_freq,
                           ev.fmin, ev.fmax))
    assert len(expect) == 2, expect
    assert f64["events"] == expect
    assert f64["events"] == f32["events"]
    assert f64["state"] == f32["state"] == fsm.f.state
    # band snapshots: the FP64 rows the detector saw, per bin
    lo = oracle.lib().ro_oracle_frequency_to_bin(bins, 48000, 9000.0)
    hi = oracle.lib().ro_oracle_frequency_to_bin(bins, 48000, 12000.0)
    assert len(f64["blid"]) == len(f32["blid"]) == 2
    for (hdr, data, _), e in zip(f64["blid"], expect):
        start, length = e[1], e[2]
        assert data.shape == (length, hi - lo)
        assert per_bin(data, want[start:start + length, lo:hi]).max() <= ONE_ULP
    # raw captures: the same float pairs, byte for byte, with the same headers
    assert len(f64["raws"]) == len(f32["raws"]) == 2
    for (h64, d64, c64), (h32, d32, c32) in zip(f64["raws"], f32["raws"]):
        assert d64.tobytes() == d32.tobytes()
        assert cards_but_date(c64) == cards_but_date(c32)


def test_c1_wav_to_fits_f64(oracle, tmp_path):
    """C1 (test_c1_wav_to_fits_end_to_end's WAV) in FP64: the FITS headers equal the float32 run's card for card (all
    but DATE, the files' creation time), the images are the oracle's rows per bin."""
    from test_host_cpu import read_fits, wav_bytes
    rng = np.random.default_rng(0xC1)
    frames = 1024 * 200
    f = add_tone(noise_iq(rng, frames, 300.0), 10400.0, 8000.0)
    i16 = np.clip(np.rint(f), -32768, 32767).astype(np.int16)
    payload = wav_bytes(i16, rate=48000)
    out = {}
    for prec, name in ((F32, "f32"), (F64, "f64")):
        d = tmp_path / name
        d.mkdir()
        rows, files, err = P.wav_to_fits(prec, payload, 1024, 512, 16, 1, 9000.0, 12000.0, d, "c1test",
                                         clock_sec=1700000000)
        assert err == "", err
        out[prec] = (rows, [read_fits(x) for x in files], [x.rsplit("/", 1)[-1] for x in files])
    want = oracle.stft(i16.astype(np.float64), 1024, 512)
    rows, fits64, names64 = out[F64]
    assert rows == out[F32][0] == want.shape[0]
    assert names64 == out[F32][2]
    assert len(fits64) == len(out[F32][1]) == int(np.ceil(rows / 94))
    for (h64, _, c64), (h32, _, c32) in zip(fits64, out[F32][1]):
        assert cards_but_date(c64) == cards_but_date(c32)
    lo = oracle.lib().ro_oracle_frequency_to_bin(1024, 48000, 9000.0)
    hi = oracle.lib().ro_oracle_frequency_to_bin(1024, 48000, 12000.0)
    got = np.concatenate([x[1] for x in fits64])
    assert got.shape == (rows, hi - lo)
    e = per_bin(got, want[:, lo:hi])
    print("C1 in FP64: per-bin rel err max %.3g" % e.max())
    assert e.max() <= ONE_ULP


@pytest.mark.parametrize("bins,overlap,rows", [(32768, 24576, 120), (4096, 3072, 800)])
def test_f64_graph_replay_equals_resident(ro, torch_cuda, bins, overlap, rows):
    """An FP64 stream at the latency-bound default batch, long enough that each of the three streaming slots replays
    its captured graph several times (>= 3 full batches per slot after its first, plain one): its rows equal a
    run_resident of the same doubles on an FP64 handle, bit for bit."""
    torch = torch_cuda
    hop = bins - overlap
    rng = np.random.default_rng(bins ^ 0x6A)
    T = bins + (rows - 1) * hop
    z = c3_doubles(rng, T)
    p = P.PrecisionPipeline(bins, overlap, F64, snapshot_length=60)
    br = p.batch_rows()
    assert rows >= br * 3 * 4, (rows, br)                     # 3 slots x (1 plain + >= 3 graphed) full batches
    assert rows < p.ring_capacity()
    feed(p, z, [4096])
    assert p.error == "" and p.rows == rows
    t = p.timing()
    got = p.newest_rows(rows)
    p.close()
    d_iq = torch.from_numpy(np.ascontiguousarray(z).view(np.float64).reshape(-1, 2).copy()).cuda()
    d_rows = torch.full((rows, bins), float("nan"), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, precision=ro.RO_PRECISION_F64) as st:
        st.run_resident(d_iq, ro.RO_IQ_F64, T, 0, rows, d_rows, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    want = d_rows.cpu().numpy()
    print("FP64 stream, %d bins: %d rows per batch, %d batches, push %.3f ms avg"
          % (bins, br, t["batches"], t["push_ms_avg"]))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_f64_on_a_length_without_a_double_plan_is_refused():
    """FP64 at a chirp-z length (32728 bins, src/BolidRecorder.h:35): ro_stft_create refuses it, lastError() carries
    the library's text, no rows come -- nothing falls back to float32."""
    bins, overlap = 32728, 24546
    p = P.PrecisionPipeline(bins, overlap, F64)
    assert "RO_PRECISION_F64" in p.error and "power-of-two" in p.error, p.error
    rng = np.random.default_rng(7)
    z = rng.standard_normal(bins * 4) + 0j
    feed(p, z, [4096])
    assert p.rows == 0
    p.close()
    q = P.PrecisionPipeline(bins, overlap, F32)                # the same length in float32 runs (chirp-z)
    feed(q, z, [4096])
    assert q.error == "" and q.rows > 0
    q.close()
