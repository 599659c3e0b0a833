"""GPU: every kernel family's addressing beyond 2^32 and 2^33 bytes, and the stream calls beyond 2^31 rows
(tests/wide_offsets.py has the case table and the layout arithmetic; tests/test_wide_offsets_cpu.py holds the table to its
promises and runs the host twins' half of the long streams).

One allocation for the whole file, the arena of 2^34 + 2^28 bytes; the large pointer of every case is BASE = arena + 2^33,
so whatever address a 32-bit slip computes lies inside the arena (wide_offsets.wrong_addresses).  Around every case the
arena is filled with the NaN pattern 0x7fc00000 and looked at afterwards, 1 GiB at a time: what the case was to write holds
what it was to hold, every other word still holds the pattern.  A wrong read poisons a result, a wrong write changes a word.

  1. samples at BASE, three rows -- one across the threshold, two above it -- into a small output: bit for bit the same entry
     point on a compact copy of those samples with first_row = 0 (rows, tile and records), and that compact baseline is held
     to the oracle at the bar the family's own test file has (imported, no new bar);
  2. three output rows at BASE, 2^30 + 4 floats apart: bit for bit the dense run of the same call; and the rows' readers,
     the window cuts, the ring;
  3. one dense output of more than 2^32 bytes from a single call: all of it finite, the rows either side of byte 2^32 and the
     first and the last bit for bit separate one-row calls;
  4. the stream calls K rows later (wide_offsets.translating): the device against the host twin at both places, and against
     itself;
  5. four ring_put -> snapshots -> raw steps on one stream with nothing waited for, the capacities doubling from step to
     step so that both of the handle's scratch blocks are regrown three times while the step before is still queued: every
     step equals the host twins' chain byte for byte.
Nothing here has a tolerance of its own.  Beside the arena the file holds well under 1 GiB: the looks at the arena go 1 GiB
at a time and make a byte per word."""
import time
from collections import namedtuple

import numpy as np
import pytest

import rawlib
import snapshotslib
import wide_offsets as W
import test_gpu_events as GE
import test_gpu_raw as GR
import test_gpu_snapshots as GS
from eventslib import random_decisions, records_for, same_bytes
from test_gpu_band import make_signal as band_signal
from test_gpu_band_f64 import make_signal as band64_signal
from test_gpu_band_windows import make_signal as windows_signal
from test_gpu_band_windows_f64 import make_signal as windows64_signal
from test_gpu_chunk_seams import oracle_check                  # each path's own measure and bar, named there
from test_gpu_spectra import per_component                     # FP64 handles' spectra: per component of every bin ...
from util import add_tone, noise_iq

FP64_SPECTRA_BAR = 1.2e-7       # ... within a float32 ulp (tests/test_gpu_spectra.py::test_fp64_mode_spectra_are_the_double_transform)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SLICE_WORDS = (1 << 30) // 4                                   # the arena is looked at 1 GiB at a time


# ---- the arena ----------------------------------------------------------------------------------------------------------
class Arena:
    def __init__(self, torch):
        self.torch = torch
        self.bytes = torch.empty(W.ARENA_BYTES, dtype=torch.uint8, device="cuda")
        self.words = self.bytes.view(torch.int32)
        self.floats = self.bytes.view(torch.float32)
        self.base = self.bytes.data_ptr() + W.BASE             # what the library is handed

    def fill(self):
        self.words.fill_(W.FILL_WORD)

    def put(self, offset, t):
        """the bytes of tensor t at `offset` bytes from BASE"""
        flat = t.contiguous().view(self.torch.uint8).reshape(-1)
        self.bytes[W.BASE + offset:W.BASE + offset + flat.numel()] = flat

    def get(self, offset, count, dtype):
        """`count` elements of `dtype` from `offset` bytes from BASE, as a copy"""
        n = count * self.torch.empty((), dtype=dtype).element_size()
        return self.bytes[W.BASE + offset:W.BASE + offset + n].clone().view(dtype)

    def finite(self, ext):
        lo, hi, step = (W.BASE + ext.lo) // 4, (W.BASE + ext.hi) // 4, SLICE_WORDS // 4      # (isfinite makes a copy: 256 MiB each)
        return all(bool(self.torch.isfinite(self.floats[a:min(a + step, hi)]).all()) for a in range(lo, hi, step))

    def restore(self, extents):
        for e in extents:
            assert e.lo % 4 == 0 and e.hi % 4 == 0
            self.words[(W.BASE + e.lo) // 4:(W.BASE + e.hi) // 4].fill_(W.FILL_WORD)

    def changed_words(self):
        """how many words of the whole arena do not hold the fill pattern, and the byte offset from BASE of the first"""
        torch = self.torch
        dirty = torch.zeros((), dtype=torch.bool, device=self.words.device)
        for a in range(0, self.words.numel(), SLICE_WORDS):
            dirty |= (self.words[a:a + SLICE_WORDS] != W.FILL_WORD).any()
        if not bool(dirty):
            return 0, None
        bad, first = 0, None                                   # (only a failing case gets here: count, and name the first)
        for a in range(0, self.words.numel(), SLICE_WORDS):
            hit = torch.nonzero(self.words[a:a + SLICE_WORDS] != W.FILL_WORD)
            bad += hit.numel()
            if hit.numel() and first is None:
                first = (a + int(hit[0])) * 4 - W.BASE
        return bad, first

    def untouched_but(self, extents):
        """after the extents' contents have been checked: put the pattern back there, and the whole arena must hold it"""
        self.restore(extents)
        bad, where = self.changed_words()
        assert bad == 0, "%d words outside the case's extents were written, the first at BASE %+d bytes" % (bad, where)


@pytest.fixture(scope="module")
def arena(torch_cuda):
    torch = torch_cuda
    box = Arena(torch)
    yield box
    torch.cuda.synchronize()
    print("peak device memory of the file in torch: %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9))
    box.bytes = box.words = box.floats = None
    del box
    torch.cuda.empty_cache()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def filled(torch, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- signals and launches of the kernel table ---------------------------------------------------------------------------
Shape = namedtuple("Shape", "name path bins hop precision windows")     # what test_gpu_chunk_seams.oracle_check reads of a case
_signals = {}


def shape_of(k):
    return Shape(k.name, k.path, k.bins, W.hop(k), k.precision, k.windows)


def compact_signal(k, fmt):
    """(what the oracle is given, what is uploaded) for the three rows of a kernel: each path's recipe from its own test file
    (named in test_gpu_chunk_seams.signal); int16 frames are un-normalised, doubles hold the float32 values"""
    if (k.name, fmt) not in _signals:
        n, seed = k.bins + (W.ROWS - 1) * W.hop(k), 0x1DE + W.KERNELS.index(k)
        if k.path == "rows" and k.precision == W.F64:
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 7000.0, 1000.0)
        elif k.path == "rows":
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 10600.0, 20.0)
        elif k.path == "spectra" and k.precision == W.F64:     # tests/test_gpu_spectra.py: noise + a 1000 sigma tone
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 9100.0, 1000.0)
        elif k.path == "spectra":
            iq = add_tone(noise_iq(np.random.default_rng(seed), n), 7000.0, 5.0)
        elif k.path == "band":
            iq = (band64_signal if k.precision == W.F64 else band_signal)(seed, n, k.bins, *k.windows[0])
        else:
            iq = (windows64_signal if k.precision == W.F64 else windows_signal)(seed, n, k.bins, k.windows)
        send = iq
        if fmt == W.IQ_I16:
            send = np.clip(np.rint(iq * 16.0), -32768, 32767).astype(np.int16)
            iq = send.astype(np.float32)
        elif fmt == W.IQ_F64:
            send = iq.astype(np.float64)
        iq.setflags(write=False)
        send.setflags(write=False)
        _signals[(k.name, fmt)] = (iq, send)
    return _signals[(k.name, fmt)]


def baseline_check(ro, oracle, k, r, got, iq, window):
    """row r of the compact baseline against the oracle, at the bar of the family's own test file; returns (figure, bar)"""
    if k.path == "spectra" and k.precision == W.F64:
        z = iq[r * W.hop(k):r * W.hop(k) + k.bins].astype(np.float64)
        _, want = oracle.row_with_spectrum(z[:, 0] + 1j * z[:, 1], window)
        x = got.astype(np.float64).reshape(k.bins, 2)
        return per_component(x[:, 0] + 1j * x[:, 1], want), FP64_SPECTRA_BAR
    return oracle_check(ro, oracle, shape_of(k), r, got, iq, window)


def handle_for(ro, k):
    kw = dict(bins=k.bins, overlap=W.overlap(k), precision=k.precision)
    if k.path == "rows":                                       # bands and a tile: the fused and the separate scan and tile
        bands, tile = W.bands_of(k.bins)
        kw.update(bands=ro.Bands(*bands), tile=tile)
    return ro.Stft(**kw)


class Outputs:
    """the small outputs of one launch: rows (or spectra, or the band image), and for the transform cases tile and records"""

    def __init__(self, torch, k, rows=True):
        comp = 2 if k.path == "spectra" else 1
        self.rows = filled(torch, W.ROWS, W.width(k) * comp) if rows else None
        self.tile = filled(torch, W.ROWS, W.bands_of(k.bins)[1][1]) if k.path == "rows" else None
        self.recs = filled(torch, W.ROWS, 3) if k.path == "rows" else None

    def same(self, torch, other):
        """bit for bit, whatever both hold (an Outputs without rows has them at BASE)"""
        pairs = ((self.rows, other.rows), (self.tile, other.tile), (self.recs, other.recs))
        return all(same_bits(torch, a, b) for a, b in pairs if a is not None and b is not None)


def launch(torch, st, k, d_iq, fmt, samples, first_row, d_out, stride, o):
    s = stream_of(torch)
    if k.path == "rows":
        st.run_resident(d_iq, fmt, samples, first_row, W.ROWS, d_out, row_stride=stride, d_tile=o.tile, d_records=o.recs, stream=s)
    elif k.path == "spectra":
        st.spectra_resident(d_iq, fmt, samples, first_row, W.ROWS, d_out, stride=stride, stream=s)
    elif k.path == "band":
        st.band_resident(d_iq, fmt, samples, first_row, W.ROWS, k.windows[0][0], k.windows[0][1], d_out, band_stride=stride, stream=s)
    else:
        st.band_windows_resident(d_iq, fmt, samples, first_row, W.ROWS, k.windows, d_out, band_stride=stride, stream=s)
    torch.cuda.synchronize()


# ---- 1. samples at BASE -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k.name for k in W.KERNELS])
def test_samples_beyond_both_thresholds(ro, oracle, torch_cuda, arena, name):
    torch, k = torch_cuda, W.kernel(name)
    t0 = time.perf_counter()
    with handle_for(ro, k) as st:
        window = st.window if k.path == "spectra" else None
        for fmt in k.formats:
            iq, send = compact_signal(k, fmt)
            d_small = torch.from_numpy(np.array(send)).cuda()
            # the compact baseline: the same entry point at first_row 0 -- and a real transform, by the oracle
            base = Outputs(torch, k)
            launch(torch, st, k, d_small, fmt, send.shape[0], 0, base.rows, W.width(k), base)
            assert bool(torch.isfinite(base.rows).all())
            for r in range(W.ROWS):
                figure, bar = baseline_check(ro, oracle, k, r, base.rows[r].cpu().numpy(), iq, window)
                print("%s %s: compact row %d against the oracle %.3e, bar %.1e" % (k.name, W.FORMAT_NAMES[fmt], r, figure, bar))
                assert figure <= bar, (k.name, fmt, r, figure)
            for threshold in W.THRESHOLDS:
                c = W.SampleCase(k, fmt, threshold)
                ext, = W.sample_extents(c)
                assert ext.hi - ext.lo == send.nbytes and W.tail_samples(c) == send.shape[0]
                arena.fill()
                arena.put(ext.lo, d_small)                     # only the tail the rows read: the rest of the arena stays NaN
                got = Outputs(torch, k)
                launch(torch, st, k, arena.base, fmt, W.samples(c), W.first_row(c), got.rows, W.width(k), got)
                assert got.same(torch, base), "%s: rows, tile or records differ from the compact baseline" % W.sample_id(c)
                assert torch.equal(arena.get(ext.lo, send.nbytes, torch.uint8), d_small.view(torch.uint8).reshape(-1)), \
                    "%s: the samples were written" % W.sample_id(c)
                arena.untouched_but([ext])
    torch.cuda.synchronize()
    print("%s: %.2f s" % (k.name, time.perf_counter() - t0))


# ---- 2. three output rows at BASE, 2^30 + 4 floats apart ----------------------------------------------------------------
def rows_at_base(torch, arena, c, want, what="rows"):
    """the case's three extents hold `want`'s three rows bit for bit"""
    for r, ext in enumerate(W.strided_extents(c)):
        got = arena.get(ext.lo, c.row_floats, torch.float32)
        assert same_bits(torch, got, want[r].reshape(-1)), "%s: %s row %d at BASE + %d differs" % (c.name, what, r, ext.lo)


@pytest.mark.parametrize("name", [c.name for c in W.STRIDED_CASES if c.role == "out"])
def test_output_rows_strided_beyond_both_thresholds(ro, torch_cuda, arena, name):
    torch, c = torch_cuda, W.strided(name)
    k = c.kernel
    _, send = compact_signal(k, W.IQ_F32)
    d_iq = torch.from_numpy(np.array(send)).cuda()
    stride = W.STRIDE_SPECTRA if k.path == "spectra" else W.STRIDE_FLOATS
    assert stride * (8 if k.path == "spectra" else 4) == c.stride_floats * 4
    with handle_for(ro, k) as st:
        dense = Outputs(torch, k)
        launch(torch, st, k, d_iq, W.IQ_F32, send.shape[0], 0, dense.rows, W.width(k), dense)
        assert bool(torch.isfinite(dense.rows).all())
        arena.fill()
        wide = Outputs(torch, k, rows=False)
        launch(torch, st, k, d_iq, W.IQ_F32, send.shape[0], 0, arena.base, stride, wide)
    rows_at_base(torch, arena, c, dense.rows)
    assert wide.same(torch, dense), "%s: tile or records differ from the dense run" % c.name
    arena.untouched_but(W.strided_extents(c))


def reader_fixture(ro, torch):
    """1024 bins, 75 % overlap, two band sets: (handle, d_iq, samples, the three dense rows)"""
    bins, overlap = W.READER_BINS, W.READER_BINS * 3 // 4
    n = bins + (W.ROWS - 1) * (bins - overlap)
    iq = add_tone(noise_iq(np.random.default_rng(0x1024), n), 6000.0, 20.0)
    st = ro.Stft(bins=bins, overlap=overlap, bands=ro.Bands(100, 64, 630, 20, 5), extra_bands=[ro.Bands(700, 64, 310, 20, 5)])
    d_iq = torch.from_numpy(iq).cuda()
    rows = filled(torch, W.ROWS, bins)
    st.run_resident(d_iq, ro.RO_IQ_F32, n, 0, W.ROWS, rows, stream=stream_of(torch))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rows).all())
    return st, d_iq, n, rows


@pytest.mark.parametrize("name", [c.name for c in W.STRIDED_CASES if c.role == "image"])
def test_window_images_strided_beyond_both_thresholds(ro, torch_cuda, arena, name):
    torch, c = torch_cuda, W.strided(name)
    s = stream_of(torch)
    st, d_iq, n, rows = reader_fixture(ro, torch)
    with st:
        image = filled(torch, W.ROWS, c.row_floats)
        arena.fill()
        if c.entry == "ro_stft_run_resident_windows":
            outs = [[filled(torch, W.ROWS, W.READER_BINS), filled(torch, W.ROWS, 3), filled(torch, W.ROWS, 3)] for _ in range(2)]
            for (r, recs, extra), d_image, stride in ((outs[0], image, None), (outs[1], arena.base, W.STRIDE_FLOATS)):
                st.run_resident_windows(d_iq, ro.RO_IQ_F32, n, 0, W.ROWS, r, W.READER_WINDOWS, d_image, image_stride=stride,
                                        d_records=recs, d_extra=extra, stream=s)
            torch.cuda.synchronize()
            assert all(same_bits(torch, a, b) and bool(torch.isfinite(a).all()) for a, b in zip(*outs))
            assert same_bits(torch, outs[0][0], rows)
        else:
            st.cut_windows_resident(rows, W.ROWS, W.READER_WINDOWS, image, stream=s)
            st.cut_windows_resident(rows, W.ROWS, W.READER_WINDOWS, arena.base, image_stride=W.STRIDE_FLOATS, stream=s)
            torch.cuda.synchronize()
    cut = torch.cat([rows[:, f:f + w] for f, w in W.READER_WINDOWS], dim=1)
    assert same_bits(torch, image, cut)
    rows_at_base(torch, arena, c, image, "image")
    arena.untouched_but(W.strided_extents(c))


@pytest.mark.parametrize("name", [c.name for c in W.STRIDED_CASES if c.role == "in"])
def test_readers_of_rows_strided_beyond_both_thresholds(ro, torch_cuda, arena, name):
    torch, c = torch_cuda, W.strided(name)
    s = stream_of(torch)
    st, _, _, rows = reader_fixture(ro, torch)
    exts = W.strided_extents(c)
    with st:
        arena.fill()
        for r, ext in enumerate(exts):
            arena.put(ext.lo, rows[r])
        results = []
        for d_rows, stride in ((rows, None), (arena.base, W.STRIDE_FLOATS)):
            if c.entry == "ro_stft_scan_resident":
                out = [filled(torch, W.ROWS, 3)]
                st.scan_resident(d_rows, W.ROWS, out[0], row_stride=stride, stream=s)
            elif c.entry == "ro_stft_scan_sets_resident":
                out = [filled(torch, W.ROWS, 3), filled(torch, W.ROWS, 3)]
                st.scan_sets_resident(d_rows, W.ROWS, out[1], d_records=out[0], row_stride=stride, stream=s)
            elif c.entry == "ro_stft_ln_tile_resident":
                out = [filled(torch, W.ROWS, 200), torch.full((W.ROWS, 200), 77, dtype=torch.uint8, device="cuda"), filled(torch, 2)]
                st.ln_tile_resident(d_rows, W.ROWS, 300, 200, d_ln=out[0], d_u8=out[1], d_minmax=out[2], row_stride=stride, stream=s)
            else:
                out = [filled(torch, W.ROWS, sum(w for _, w in W.READER_WINDOWS))]
                st.cut_windows_resident(d_rows, W.ROWS, W.READER_WINDOWS, out[0], row_stride=stride, stream=s)
            torch.cuda.synchronize()
            results.append(out)
    for a, b in zip(*results):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), c.name
        assert a.dtype == torch.uint8 or bool(torch.isfinite(a).all())
    rows_at_base(torch, arena, c, rows)                        # the rows are as they were
    arena.untouched_but(exts)


def test_ring_strided_beyond_both_thresholds(ro, torch_cuda, arena):
    """three ring slots 2^30 + 4 floats apart; rows 22, 23, 24 go to slots 1, 2, 0; one event in each of three detector slots,
    whose snapshots read one, two and all three ring slots: ro_snapshots_host over the compact ring, byte for byte"""
    torch = torch_cuda
    c = W.strided("ring_put_resident, snapshots_resident: ring")
    s = stream_of(torch)
    cols, first = W.RING_COLS, 22
    case = snapshotslib.Case(ro, {0: [(first, 1)], 1: [(first + 1, 2)], 2: [(first, 3)]}, 5, W.ROWS, cols, first + W.ROWS, cols * 6,
                             pcap=2)
    want = snapshotslib.host_call(ro, case)
    assert snapshotslib.statuses(want) == [snapshotslib.CAPTURED] * 3 and int(want.summary["arena_floats"]) == cols * 6
    image = np.stack([snapshotslib.row_values(first + i, cols) for i in range(W.ROWS)])
    d_image = torch.from_numpy(image).cuda()
    d_outs = [GS.up(torch, o) for o in snapshotslib.outputs_for(case)]
    d_events, d_summary = GS.up(torch, case.events), GS.up(torch, case.summary)
    ring = ro.capi.RowRing(arena.base, W.STRIDE_FLOATS, W.ROWS, cols, 0)
    arena.fill()
    with GS.handle(ro) as st:
        st.ring_put_resident(d_image, first, W.ROWS, ring, stream=s)
        st.snapshots_resident(case.mask, case.snapshot_rows.tolist(), ring, case.head_row, d_outs[2], d_outs[3], case.pcap,
                              d_outs[0], d_outs[1], case.arena_floats, d_outs[4], d_events=d_events, capacity=case.capacity,
                              d_summary=d_summary, stream=s)
        torch.cuda.synchronize()
    got = snapshotslib.Result(ro, case, *[o.cpu().numpy() for o in d_outs])
    assert got.summary.tobytes() == want.summary.tobytes() and got.dir.tobytes() == want.dir.tobytes(), (got.dir, want.dir)
    assert got.same_bytes(want)
    rows_at_base(torch, arena, c, torch.from_numpy(np.ascontiguousarray(case.ring[:, :cols])).cuda(), "ring")
    arena.untouched_but(W.strided_extents(c))


# ---- 3. one dense output of more than 2^32 bytes ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in W.DENSE_CASES if c.entry == "ro_stft_run_resident"])
def test_dense_rows_and_tile_beyond_2_32_bytes(ro, torch_cuda, arena, name):
    """256 bins, overlap 255, 2^22 + 3 rows in one call: 4 GiB + 3 KiB of rows at BASE, the whole-row tile behind them (it
    passes 2^33 bytes), records and one extra set's records elsewhere"""
    torch, c = torch_cuda, W.dense(name)
    s = stream_of(torch)
    R, bins = c.rows, c.bins
    n = bins + R - 1
    iq = add_tone(noise_iq(np.random.default_rng(0xDE5E), n), 10600.0, 20.0)
    d_iq = torch.from_numpy(iq).cuda()
    rows_ext, tile_ext = W.dense_extents(c)
    recs, extra = filled(torch, R, 3), filled(torch, R, 3)
    arena.fill()
    with ro.Stft(bins=bins, overlap=bins - 1, precision=c.precision, bands=ro.Bands(*W.bands_of(bins)[0]), tile=(0, bins),
                 extra_bands=[ro.Bands(40, 16, 200, 8, 3)]) as st:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.run_resident_sets(d_iq, ro.RO_IQ_F32, n, 0, R, arena.base, d_tile=arena.base + tile_ext.lo, d_records=recs,
                             d_extra=extra, stream=s)
        torch.cuda.synchronize()
        print("%s: %d rows in one call, %.3f s" % (c.name, R, time.perf_counter() - t0))
        assert arena.finite(rows_ext) and arena.finite(tile_ext), "a row or a tile row was never written"
        # (as floats: the peak column is a small int32, a denormal -- a record no launch wrote is the NaN fill throughout)
        assert bool(torch.isfinite(recs).all()) and bool(torch.isfinite(extra).all()), "a record was never written"
        for r in W.dense_probe_rows(c):
            one = [filled(torch, 1, bins), filled(torch, 1, bins), filled(torch, 1, 3), filled(torch, 1, 3)]
            st.run_resident_sets(d_iq, ro.RO_IQ_F32, n, r, 1, one[0], d_tile=one[1], d_records=one[2], d_extra=one[3], stream=s)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(one[0]).all())
            assert same_bits(torch, arena.get(r * bins * 4, bins, torch.float32), one[0][0]), (c.name, r, "row")
            assert same_bits(torch, arena.get(tile_ext.lo + r * bins * 4, bins, torch.float32), one[1][0]), (c.name, r, "tile")
            assert same_bits(torch, recs[r], one[2][0]) and same_bits(torch, extra[r], one[3][0]), (c.name, r, "records")
    arena.untouched_but([rows_ext, tile_ext])


def test_dense_band_image_beyond_2_32_bytes(ro, torch_cuda, arena):
    """16384 bins, overlap 16383, 1024 columns, 2^20 + 3 rows in one ro_stft_band_resident: 4 GiB + 12 KiB of band image"""
    torch, c = torch_cuda, W.dense("band 16384 x 1024")
    s = stream_of(torch)
    R, bins = c.rows, c.bins
    first_col, cols = W.DENSE_BAND
    n = bins + R - 1
    iq = band_signal(0xBA4D, n, bins, first_col, cols)
    d_iq = torch.from_numpy(iq).cuda()
    ext, = W.dense_extents(c)
    at = W.dense_probe_rows(c)[2]
    arena.fill()
    with ro.Stft(bins=bins, overlap=bins - 1) as st:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.band_resident(d_iq, ro.RO_IQ_F32, n, 0, R, first_col, cols, arena.base, stream=s)
        torch.cuda.synchronize()
        print("%s: %d rows in one call, %.3f s" % (c.name, R, time.perf_counter() - t0))
        assert arena.finite(ext), "a row of the band image was never written"
        for r in sorted(set(W.dense_probe_rows(c)) | {at - 2, at + 1}):
            one = filled(torch, 1, cols)
            st.band_resident(d_iq, ro.RO_IQ_F32, n, r, 1, first_col, cols, one, stream=s)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(one).all())
            assert same_bits(torch, arena.get(r * cols * 4, cols, torch.float32), one[0]), (c.name, r)
    arena.untouched_but([ext])


# ---- 4. long streams ----------------------------------------------------------------------------------------------------
def test_snapshots_translated_on_the_device(ro, torch_cuda):
    """the decision table, 20 random cases and a ring of 255 rows: the device against ro_snapshots_host where they stand and
    K = 2^33 + k rows later, and the device against itself"""
    torch = torch_cuda
    emu = snapshotslib.load_emu()
    counter = [0, 0]
    with GS.handle(ro) as st:
        call = W.translating_snapshots(GS.device_vs_host(ro, torch, st), counter)
        for case_fn in snapshotslib.TABLE:
            case_fn(ro, call)
        table = counter[0]
        assert table >= len(snapshotslib.TABLE) - 3
        rng = np.random.default_rng(2033)
        while counter[0] < table + 20:
            call(snapshotslib.case_from_emu(ro, emu.random_case(rng)))
            assert sum(counter) < 400
        first, then = W.ring_255_cases(ro)
        before = counter[0]
        call(then(call(first)))
        assert counter[0] == before + 2


@pytest.mark.parametrize("ring_rows,cols", [(255, 33), (64, 257)])
def test_ring_put_translated(ro, torch_cuda, ring_rows, cols):
    """ro_stft_ring_put_resident at first_row = K + j fills the same slots as at j, K a multiple of ring_rows beyond 2^33"""
    torch = torch_cuda
    k = W.snapshot_shift(ring_rows)
    stride = cols + 3
    rng = np.random.default_rng(ring_rows)
    with GS.handle(ro) as st:
        for j, rows in ((5 * ring_rows + ring_rows - 3, 7), (17, ring_rows), (3 * ring_rows + 1, ring_rows + 9)):
            image = rng.standard_normal((rows, cols)).astype(np.float32)
            want = np.full((ring_rows, stride), snapshotslib.PAD, np.float32)
            for i in range(max(0, rows - ring_rows), rows):
                want[(j + i) % ring_rows, :cols] = image[i]
            d_image = torch.from_numpy(image).cuda()
            rings = []
            for first in (j, k + j):
                d_ring = torch.full((ring_rows, stride), float(snapshotslib.PAD), dtype=torch.float32, device="cuda")
                st.ring_put_resident(d_image, first, rows, ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0),
                                     stream=stream_of(torch))
                torch.cuda.synchronize()
                rings.append(d_ring.cpu().numpy())
            assert rings[0].tobytes() == want.tobytes() and rings[1].tobytes() == want.tobytes(), (ring_rows, j, rows)


def test_raw_translated_on_the_device(ro, torch_cuda):
    """the decision table, 16 random cases, an odd hop and overlap 0: the device against ro_raw_host where they stand and
    K = 2^36 rows later (first_sample + K x hop, 2^44 at a hop of 256), and the device against itself"""
    torch = torch_cuda
    counter = [0, 0]
    handles = GR.Handles(ro)
    try:
        call = W.translating_raw(GR.device_vs_host(ro, torch, handles), counter)
        for case_fn in rawlib.TABLE:
            case_fn(ro, call)
        table = counter[0]
        assert table >= len(rawlib.TABLE) - 1
        rng = np.random.default_rng(2036)
        while counter[0] < table + 16:
            call(rawlib.case_from_emu(ro, rawlib.EMU.random_case(rng)))
            assert sum(counter) < 400
        for shape in W.ODD_HOP_SHAPES:
            W.odd_hop_case(ro, shape, call)
        assert counter[0] == table + 16 + len(W.ODD_HOP_SHAPES)
    finally:
        handles.close()


def test_events_translated_on_the_device(ro, torch_cuda):
    """ro_stft_events_resident over three calls with carried state at first_row 0 and at 2^33 + 5, two slots: each against
    ro_events_host, and the far one against the near one with its rows raised"""
    torch = torch_cuda
    rng = np.random.default_rng(4242)
    rows, k = 3 * GE.T + 50, W.EVENTS_SHIFT
    decisions = [random_decisions(rng, rows), random_decisions(rng, rows)]
    recs = np.stack([records_for(ro, d, seed=i) for i, d in enumerate(decisions)], axis=1)
    dets = [(12, 4), (3, 9)]
    detect_rows = np.flatnonzero(decisions[0])
    cuts = sorted({int(detect_rows[detect_rows.size // 3]) + 1, GE.T + 1})      # one right behind a detect row: a group is carried
    with GE.handle(ro, 1) as st:
        d_states = [GE.fresh_state(ro, torch, 2), GE.fresh_state(ro, torch, 2)]
        host_states = [[None, None], [None, None]]
        fired = carried = 0
        for lo, hi in zip([0] + cuts, cuts + [rows]):
            part = recs[lo:hi]
            got = [GE.device_call(ro, torch, st, np.ascontiguousarray(part[:, 0]), np.ascontiguousarray(part[:, 1:]), dets,
                                  d_states[w], first_row=base + lo) for w, base in enumerate((0, k))]
            for w, base in enumerate((0, k)):
                for slot in range(2):
                    host_states[w][slot] = GE.check_slot(ro, got[w], slot, np.ascontiguousarray(part[:, slot]), dets[slot],
                                                         first_row=base + lo, state=host_states[w][slot])
            (ev0, sm0, st0, dt0), (ev1, sm1, st1, dt1) = got
            assert sm0.tobytes() == sm1.tobytes() and np.array_equal(dt0, dt1)
            for slot in range(2):
                n = int(sm0["events"][slot])
                near = ev0[slot, :n * 40].view(ro.capi.EVENT_DTYPE)
                far = ev1[slot, :n * 40].view(ro.capi.EVENT_DTYPE).copy()
                far["fire_row"] -= k
                far["start_row"] -= k
                assert same_bytes(far, near), (slot, lo)
                back = st1[slot:slot + 1].copy()
                if back["open"][0]:
                    back["first_detect_row"] -= k
                    back["last_detect_row"] -= k
                    carried += 1
                assert same_bytes(back, st0[slot:slot + 1]), (slot, lo, st0[slot], st1[slot])
                fired += n
        assert fired >= 6 and carried > 0


# ---- 5. scratch that grows in the middle of an unsynchronised chain ---------------------------------------------------------
def padded(a, n):
    out = np.zeros(n, a.dtype)
    out[:a.size] = a.reshape(-1)
    return out


def test_scratch_regrown_in_the_middle_of_an_unsynchronised_chain(ro, torch_cuda):
    """four ring_put -> snapshots_resident -> raw_resident steps at 256 bins on one stream, nothing waited for; capacity,
    pending_capacity and dir_capacity double from step to step, so the handle's snapshot scratch and raw scratch are both
    regrown three times while the step before is still queued.  Every step's directory, arena, pending list and summary --
    of the snapshots and of the raw capture -- equal the ro_snapshots_host / ro_raw_host chain byte for byte; run twice, each
    time on a fresh handle (a handle that has grown does not grow again)."""
    torch = torch_cuda
    steps, chunk, ring_rows, cols, snap = 4, 50, 96, 33, 20
    stride, total = cols + 3, 4 * 50
    shape = (256, 0, 48000)
    hop = 256
    caps = [(12 << k, 6 << k) for k in range(steps)]           # (capacity, pending_capacity); dir_capacity is their sum
    snap_arena, raw_arena = cols * 400, 2 * rawlib.L_of(shape, snap) * 12
    rng = np.random.default_rng(5)
    # the samples lag ten rows behind the rows until the last step, so that raw runs near the head wait for a step
    arrived = [((k + 1) * chunk - (10 if k < steps - 1 else 0)) * hop for k in range(steps)]
    image = np.stack([snapshotslib.row_values(r, cols) for r in range(total)])
    # ---- the host twins' chain
    snap_cases, snap_host, raw_cases, raw_host = [], [], [], []
    for k, (cap, pcap) in enumerate(caps):
        fire = np.sort(rng.integers(k * chunk, (k + 1) * chunk, 9))
        spans = [(max(int(f) - int(rng.integers(0, 16)), 1), int(rng.integers(1, 26))) for f in fire]
        spans = [(a, min(n, total - a)) for a, n in spans]
        case = snapshotslib.Case(ro, {0: spans}, snap, ring_rows, cols, (k + 1) * chunk, snap_arena, pcap=pcap, capacity=cap,
                                 stride=stride)
        if snap_host:
            case.pending = padded(snap_host[-1].pending, pcap).reshape(1, pcap)
            case.pending_count = snap_host[-1].pending_count.copy()
        snap_cases.append(case)
        snap_host.append(snapshotslib.host_call(ro, case))
        r = snap_host[-1]
        dcap = cap + pcap
        raw = rawlib.Case(ro, shape, padded(r.dir, dcap), [(0, arrived[k], rawlib.F32)], raw_arena, pcap=pcap, dcap=dcap)
        raw.snap_summary[0] = r.summary
        if raw_host:
            raw.pending = padded(raw_host[-1].pending, pcap)
            raw.pending_count = raw_host[-1].pending_count.copy()
        raw_cases.append(raw)
        raw_host.append(rawlib.host_call(ro, raw))
    assert sum(int(r.summary["captured"]) for r in snap_host) > 20 and sum(int(r.summary["captured"]) for r in raw_host) > 10
    assert any(int(r.summary["pending"]) > 0 for r in snap_host[:-1]) and any(int(r.summary["pending"]) > 0 for r in raw_host[:-1])
    assert all(int(r.summary["pending_dropped"]) == 0 and int(r.summary["unlisted"]) == 0 for r in snap_host)
    d_image = GS.up(torch, image)
    d_samples = GS.up(torch, rawlib.EMU.samples_of(0, total * hop, rawlib.F32))
    s = stream_of(torch)
    for run in range(2):
        max_pcap = caps[-1][1]
        d_ring = torch.full((ring_rows * stride,), float(snapshotslib.PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_pending = torch.zeros(max_pcap * 40, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(8, dtype=torch.uint8, device="cuda")
        d_raw_pending = torch.zeros(max_pcap * 72, dtype=torch.uint8, device="cuda")
        d_raw_count = torch.zeros(8, dtype=torch.uint8, device="cuda")
        outs = [[GS.up(torch, o) for o in snapshotslib.outputs_for(c)] for c in snap_cases]
        raw_outs = [[GS.up(torch, o) for o in rawlib.outputs_for(c)] for c in raw_cases]
        d_events = [GS.up(torch, c.events) for c in snap_cases]
        d_summary = [GS.up(torch, c.summary) for c in snap_cases]
        lists = []
        with GS.handle(ro) as st:
            torch.cuda.synchronize()
            for k, (cap, pcap) in enumerate(caps):             # ---- nothing below waits for the device
                st.ring_put_resident(d_image[k * chunk * cols * 4:], k * chunk, chunk, ring, stream=s)
                st.snapshots_resident(1, snap, ring, (k + 1) * chunk, d_pending, d_count, pcap, outs[k][0], outs[k][1], snap_arena,
                                      outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k], stream=s)
                st.raw_resident(outs[k][0], cap + pcap, outs[k][4], [(d_samples, 0, arrived[k], ro.RO_IQ_F32)],
                                d_raw_pending, d_raw_count, pcap, raw_outs[k][0], raw_outs[k][1], raw_arena, raw_outs[k][4],
                                stream=s)
                # (the lists exist once: their state behind this step, copied on the same stream without a wait)
                lists.append([t.clone() for t in (d_pending, d_count, d_raw_pending, d_raw_count)])
            torch.cuda.synchronize()
        for k, (cap, pcap) in enumerate(caps):
            pend, count, raw_pend, raw_count = [t.cpu().numpy() for t in lists[k]]
            got = [o.cpu().numpy() for o in outs[k]]
            got[2][:pcap * 40], got[3][:8] = pend[:pcap * 40], count
            r = snapshotslib.Result(ro, snap_cases[k], *got)
            assert r.summary.tobytes() == snap_host[k].summary.tobytes(), (run, k, r.summary, snap_host[k].summary)
            assert r.dir.tobytes() == snap_host[k].dir.tobytes() and r.same_bytes(snap_host[k]), (run, k)
            assert not pend[pcap * 40:].any(), "pending entries beyond pending_capacity were written"
            got = [o.cpu().numpy() for o in raw_outs[k]]
            got[2][:pcap * 72], got[3][:8] = raw_pend[:pcap * 72], raw_count
            r = rawlib.Result(ro, raw_cases[k], *got)
            assert r.summary.tobytes() == raw_host[k].summary.tobytes(), (run, k, r.summary, raw_host[k].summary)
            assert r.dir.tobytes() == raw_host[k].dir.tobytes() and r.same_bytes(raw_host[k]), (run, k)
            assert not raw_pend[pcap * 72:].any(), "raw pending entries beyond pending_capacity were written"
