"""GPU checks of the raw I/Q capture on the device (csrc/ro_raw.hip): the samples behind every captured snapshot, cut out of
the sample buffers into an arena with a directory -- against ro_raw_host byte for byte (summary, directory, arena, pending
list and count), with guard entries behind every output and the sample buffers and the snapshot directory checked
unwritten.  The inputs are synthetic (tests/rawlib.py): stream sample s is (s, -s - 0.5), so a wrong sample names itself,
and a sample read from a span that does not own it is 7777.  Only the last test runs a transform.  Nothing here has a
tolerance."""
import numpy as np
import pytest

from rawlib import (CAPTURED, EMPTY, EMU, F32, F64, GUARD, I16, LOST, TABLE, Case, L_of, Result, S, apply_refusal, case_from_emu,
                    expected_run, f_of, header_constant, host_call, outputs_for, refusals)
from snapshotslib import PAD
from snapshotslib import Case as SnapCase
from snapshotslib import Result as SnapResult
from snapshotslib import outputs_for as snap_outputs_for
from util import add_chirp, noise_iq

pytestmark = pytest.mark.gpu

B = header_constant("RO_RAW_BLOCK")
TILE = header_constant("RO_RAW_TILE")


class Handles:
    """one handle per shape: the raw call takes hop, z and the rates from it"""

    def __init__(self, ro):
        self.ro, self.by_shape = ro, {}

    def __call__(self, shape):
        if shape not in self.by_shape:
            self.by_shape[shape] = self.ro.Stft(bins=shape[0], overlap=shape[1], sample_rate=shape[2])
        return self.by_shape[shape]

    def close(self):
        for st in self.by_shape.values():
            st.close()


@pytest.fixture()
def handles(ro, torch_cuda):
    h = Handles(ro)
    yield h
    h.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def device_spans(ro, case, d_samples):
    return [ro.capi.IqSpan(d.data_ptr(), first, len(a), fmt, 0) for d, (a, first, fmt) in zip(d_samples, case.spans)]


def launch(torch, st, case, spans, d_dir, d_snap_summary, d_outs):
    """one ro_stft_raw_resident on the current stream; nothing is waited for"""
    st.raw_resident(d_dir if case.dcap else None, case.dcap, d_snap_summary, spans, d_outs[2] if case.pcap else None, d_outs[3],
                    case.pcap, d_outs[0], d_outs[1] if case.arena_floats else None, case.arena_floats, d_outs[4],
                    stream=stream_of(torch))


def device_call(ro, torch, handles, case):
    d_samples = [up(torch, a) for a, _, _ in case.spans]
    d_outs = [up(torch, o) for o in outputs_for(case)]
    d_dir = up(torch, case.directory) if len(case.directory) else None
    d_snap_summary = up(torch, case.snap_summary)
    launch(torch, handles(case.shape), case, device_spans(ro, case, d_samples), d_dir, d_snap_summary, d_outs)
    torch.cuda.synchronize()
    for d, (a, _, _) in zip(d_samples, case.spans):
        assert d.cpu().numpy().tobytes() == a.tobytes(), "the samples were written"
    assert d_dir is None or d_dir.cpu().numpy().tobytes() == case.directory.tobytes(), "the snapshot directory was written"
    assert d_snap_summary.cpu().numpy().tobytes() == case.snap_summary.tobytes()
    return Result(ro, case, *[o.cpu().numpy() for o in d_outs])


def device_vs_host(ro, torch, handles, twice=False):
    def call(case):
        got, want = device_call(ro, torch, handles, case), host_call(ro, case)
        assert got.summary.tobytes() == want.summary.tobytes(), (got.summary, want.summary)
        assert got.dir.tobytes() == want.dir.tobytes(), (got.dir, want.dir)
        assert got.same_bytes(want)
        if twice:
            assert device_call(ro, torch, handles, case).same_bytes(got), "two runs differ"
        return got
    return call


# ---- 1. the decision table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_fn", TABLE, ids=lambda f: f.__name__)
def test_decision_table_on_the_device(ro, torch_cuda, handles, case_fn):
    case_fn(ro, device_vs_host(ro, torch_cuda, handles))


def test_random_emulator_cases_on_the_device(ro, torch_cuda, handles):
    rng = np.random.default_rng(78)
    call = device_vs_host(ro, torch_cuda, handles)
    captured = 0
    for _ in range(16):
        captured += int(call(case_from_emu(ro, EMU.random_case(rng))).summary["captured"])
    assert captured > 0


# ---- 2. sizes around the copy's block ---------------------------------------------------------------------------------------
def shape_with_length(bins, overlap, L):
    """((bins, overlap, sample_rate), rows) whose raw length is exactly L, or None: L is about rows x hop x (1 + something),
    never below the hop for a snapshot with rows, so L == 1 exists for a hop of 1 only"""
    hop = bins - overlap
    for rate in range(hop, 64 * hop + 1):
        r = EMU.int_rate(bins, overlap, rate)
        for rows in {max(L * r // rate, 1), L * r // rate + 1}:
            if L_of((bins, overlap, rate), rows) == L:
                return (bins, overlap, rate), rows
    return None


@pytest.mark.parametrize("overlap", [1, 0, 192, 255])
def test_runs_around_the_copy_kernels_block(ro, torch_cuda, handles, overlap):
    """L in {1, B - 1, B, B + 1, 3 B + 5} for bins = 256 with overlap 1 (an odd hop: f alternates even and odd), 0 and 192 --
    L == 1 needs a hop of 1 (the raw length of a snapshot with rows is never below the hop), so overlap 255 is here for it,
    and the other three shapes take the four lengths a hop of theirs can give; one to four spans in each of the formats,
    the span boundaries inside a block: at its first pair, behind its first pair, at its last pair and in the middle of a wave;
    two snapshots per call, one with an even and one with an odd start; run twice"""
    torch = torch_cuda
    call = device_vs_host(ro, torch, handles, twice=True)
    lengths = [1, B - 1, B, B + 1, 3 * B + 5]
    found = {L: shape_with_length(256, overlap, L) for L in lengths}
    assert all(found[L] for L in lengths[1:]) and (found[1] is not None) == (overlap == 255), found
    for L in lengths:
        if not found[L]:
            continue
        shape, rows = found[L]
        starts = (6, 7)
        f = [f_of(shape, s) for s in starts]
        base, end = f[0] - 3, f[1] + L + 10
        for cuts, formats in (((), (F32,)), ((), (I16,)), ((), (F64,)),
                              ((B,), (F32, F64)), ((1, 2 * B - 1), (I16, F32, F64)), ((B + 1, B + 100), (F64, I16, F32)),
                              ((B - 1, B, L - 1), (F32, I16, F64, F32))):
            # span i + 1 begins `cuts[i]` pairs into the first run and owns the samples from there; every span reaches 5
            # samples into the next one, which holds those samples too: they come from the later span
            firsts = [base] + sorted({f[0] + c for c in cuts if 0 < c < L})
            ends = [a + 5 for a in firsts[1:]] + [end]
            layout = [(a, b - a, fmt) for a, b, fmt in zip(firsts, ends, formats)]
            case = Case(ro, shape, [(starts[0], rows), (starts[1], rows)], layout, 4 * L + 6)
            r = call(case)
            assert r.dir["status"].tolist() == [CAPTURED] * 2 and r.dir["samples"].tolist() == [L, L], (L, layout, r.dir)
            assert r.dir["first_sample"].tolist() == f
            for i in range(2):
                assert r.run(i).tobytes() == expected_run(case.layout, f[i], L).tobytes(), (overlap, L, layout, i)


# ---- 3. crossing the plan kernel's tile -------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", ["everything", "runs out in the second tile"])
def test_300_entries_and_30_pending_cross_the_plan_kernels_tile(ro, torch_cuda, handles, room):
    """300 directory entries and 30 pending candidates: raw_plan_kernel walks two tiles and carries the directory index, the
    packed pairs and blocks and the pending index into the second; with the small arena the room runs out inside it"""
    torch, rng = torch_cuda, np.random.default_rng(300)
    hop = S[0] - S[1]
    layout = [(100 * hop + 1, 60 * hop, F32), (150 * hop, 45 * hop, I16)]         # rows 100 ... 194, more or less

    def some(n):
        start = rng.integers(92, 198, n)
        return [(int(a), int(b), int(st)) for a, b, st in zip(start, rng.integers(0, 12, n),
                                                               rng.choice([CAPTURED] * 8 + [EMPTY, LOST], n))]
    items, pend = some(300), [(a, b) for a, b, _ in some(30)]
    case = Case(ro, S, items, layout, 10 ** 6, pending=pend, pcap=40)
    want = host_call(ro, case)
    # the first tile: the pending list and the directory's first TILE - 30 entries
    tile1 = set(case.pending[:30]["event"]["peak"].tolist()) | set(case.directory[:TILE - 30]["event"]["peak"].tolist())
    if room != "everything":
        # the room for the captured runs of the first tile's candidates and a few more: it runs out in the second tile
        floats = sum(2 * int(e["samples"]) for e in want.dir if int(e["event"]["peak"]) in tile1)
        case = Case(ro, S, case.directory, layout, floats + 900, pending=case.pending[:30], pcap=40)
        want = host_call(ro, case)
        assert int(want.summary["pending_dropped"]) > 0 and int(want.summary["arena_floats"]) > floats
    s = want.summary
    print(s)
    # (said of the host twin's result first: one of each status, and runs captured behind the first tile's packed pairs)
    assert min(int(s[k]) for k in ("captured", "empty", "lost", "pending")) > 0
    assert (int(s["pending_dropped"]) > 0) == (room != "everything")
    assert [e for e in want.dir if e["status"] == CAPTURED and int(e["event"]["peak"]) not in tile1]
    r = device_vs_host(ro, torch, handles, twice=True)(case)
    assert all((int(r.summary[k]) > 0) == (int(s[k]) > 0) for k in s.dtype.names)
    for i in list(range(0, r.dir.size, 7)) + [r.dir.size - 1]:
        if r.dir[i]["status"] == CAPTURED:
            assert r.run(i).tobytes() == expected_run(layout, int(r.dir[i]["first_sample"]), int(r.dir[i]["samples"])).tobytes(), i


# ---- 4. chained calls on one stream, nothing waited for in between -----------------------------------------------------------
def test_four_chunks_back_to_back_without_a_host_synchronisation(ro, torch_cuda, handles):
    """no overlap between the rows, so a raw run ends up to fft rate / R behind its snapshot's last row: a snapshot that ends
    with its chunk has to wait for the next chunk's samples"""
    torch = torch_cuda
    shape, chunk, chunks, pcap, dcap, arena = (256, 0, 4000), 50, 4, 8, 12, 2 * 8000 * 5
    hop = shape[0]
    rng = np.random.default_rng(5)
    # the buffer of chunk k holds the samples of its rows and the last 100 of the chunk in front; a call gets the last two
    buffers = [(max(k * chunk * hop - 100, 0), chunk * hop + min(k * chunk * hop, 100), (F32, I16, F64, F32)[k]) for k in range(chunks)]
    end = buffers[-1][0] + buffers[-1][1]
    per_chunk = []
    for k in range(chunks):
        ends = np.sort(rng.integers(k * chunk + 2, (k + 1) * chunk + 1, 7))
        rows = rng.integers(1, 30, 7)
        ends[-1], rows[-1] = (k + 1) * chunk, 28           # ends with the chunk: its raw run ends behind the buffer
        per_chunk.append([(int(e) - int(n), int(n)) for e, n in zip(ends, rows) if f_of(shape, int(e) - int(n)) + L_of(shape, int(n)) <= end])
    cases, host = [], []
    for k in range(chunks):
        case = Case(ro, shape, per_chunk[k], buffers[max(k - 1, 0):k + 1], arena, pcap=pcap, dcap=dcap)
        case.spans = [(EMU.samples_of(*b), b[0], b[2]) for b in case.layout]     # (nothing shadowed: the chunks hold the stream)
        if host:
            case.carry(host[-1])
        cases.append(case)
        host.append(host_call(ro, case))
    # (what the case is meant to hold, said of the host twin's results: the device has to equal them below)
    assert sum(int(r.summary["captured"]) for r in host) > 20 and int(host[-1].summary["pending"]) == 0
    assert all(int(r.summary["pending_dropped"]) == 0 for r in host) and any(int(r.summary["pending"]) > 0 for r in host[:-1])
    st = handles(shape)
    d_buffers = [up(torch, EMU.samples_of(*b)) for b in buffers]
    outs = [[up(torch, o) for o in outputs_for(cases[0])] for _ in range(chunks)]
    d_dirs = [up(torch, np.concatenate([c.directory, np.zeros(dcap - len(c.directory), ro.capi.SNAPSHOT_DTYPE)])) for c in cases]
    d_sums = [up(torch, c.snap_summary) for c in cases]
    d_pending, d_count = outs[0][2], outs[0][3]                          # one list for the whole stream
    torch.cuda.synchronize()
    for k in range(chunks):                                              # ---- nothing below waits for the device
        spans = [ro.capi.IqSpan(d_buffers[j].data_ptr(), buffers[j][0], buffers[j][1], buffers[j][2], 0)
                 for j in range(max(k - 1, 0), k + 1)]
        st.raw_resident(d_dirs[k], dcap, d_sums[k], spans, d_pending, d_count, pcap, outs[k][0], outs[k][1], arena, outs[k][4],
                        stream=stream_of(torch))
    torch.cuda.synchronize()
    results = []
    for k in range(chunks):
        raw = [o.cpu().numpy() for o in outs[k]]
        raw[2], raw[3] = host[k].raw[2], host[k].raw[3]                  # (the list exists once: checked behind the last call)
        results.append(Result(ro, cases[k], *raw))
        assert results[k].same_bytes(host[k]), k
    assert d_pending.cpu().numpy().tobytes() == host[-1].raw[2].tobytes()
    assert d_count.cpu().numpy().tobytes() == host[-1].raw[3].tobytes()
    for d, b in zip(d_buffers, buffers):
        assert d.cpu().numpy().tobytes() == EMU.samples_of(*b).tobytes(), "the samples were written"
    # every candidate is resolved exactly once, with the stream's samples; at least one was carried
    peaks = [int(e["event"]["peak"]) for r in results for e in r.dir]
    assert sorted(peaks) == sorted(int(p) for c in cases for p in c.directory["event"]["peak"])
    carried = [(k, e) for k, r in enumerate(results) for e in r.dir
               if int(e["event"]["peak"]) not in cases[k].directory["event"]["peak"].tolist()]
    assert carried and all(e["status"] == CAPTURED for r in results for e in r.dir)
    for k, r in enumerate(results):
        for i, e in enumerate(r.dir):
            assert r.run(i).tobytes() == expected_run(cases[k].layout, int(e["first_sample"]), int(e["samples"])).tobytes(), (k, i)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_handle(ro, torch_cuda, handles):
    torch = torch_cuda
    case = Case(ro, S, [(20, 4)], [(300, 200, F32)], 200)
    d_samples = up(torch, case.spans[0][0])
    d_outs = [up(torch, o) for o in outputs_for(case)]
    d_dir, d_sum = up(torch, case.directory), up(torch, case.snap_summary)
    base = (ro.capi.IqSpan * 4)(ro.capi.IqSpan(d_samples.data_ptr(), 300, 200, F32, 0))
    ptr = lambda t: t.data_ptr()
    lib = ro.library()

    def call(st, **kw):
        a = dict(dir=ptr(d_dir), dcap=1, snap_summary=ptr(d_sum), spans=base, span_count=1, pending=ptr(d_outs[2]),
                 count=ptr(d_outs[3]), pcap=case.pcap, raw_dir=ptr(d_outs[0]), arena=ptr(d_outs[1]), arena_floats=200,
                 out=ptr(d_outs[4]))
        a.update(apply_refusal(ro, base, kw))
        return lib.ro_stft_raw_resident(st._h, a["dir"], a["dcap"], a["snap_summary"], a["spans"], a["span_count"], a["pending"],
                                        a["count"], a["pcap"], a["raw_dir"], a["arena"], a["arena_floats"], a["out"],
                                        stream_of(torch))
    st = handles(S)
    extra = [(dict(arena=ptr(d_outs[1]) + 4), "d_arena is not aligned"),
             (dict(spans=[dict(d_iq=d_samples.data_ptr() + 4)]), "spans[0]: d_iq is not aligned")]
    for kw, word in refusals(ro, "d_") + extra:
        assert call(st, **kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_stft_raw_resident:"), (kw, text)
    # a handle whose integer fft rate is 0: the reference divides by zero there
    with ro.Stft(bins=256, overlap=0, sample_rate=200) as slow:
        assert call(slow) == -2 and "fft sample rate" in lib.ro_last_error().decode()
    torch.cuda.synchronize()
    for o, before in zip(d_outs, outputs_for(case)):
        assert o.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"
    assert call(st) == 0
    torch.cuda.synchronize()
    assert d_outs[4].cpu().numpy()[:64].view(ro.capi.RAW_SUMMARY_DTYPE)["captured"][0] == 1


# ---- 6. from samples to raw --------------------------------------------------------------------------------------------------
def test_samples_to_raw_in_three_chunks(ro, torch_cuda):
    """the shape of test_gpu_snapshots.py::test_samples_to_snapshots_in_three_chunks -- 1024 bins, 75 % overlap, 600 rows, two
    windows, two detectors, three chunks of 200 rows -- with the samples uploaded as three overlapping chunk buffers and
    raw_resident, given the last two of them, behind each snapshots_resident: run_resident_windows -> ring_put_resident ->
    events_resident -> snapshots_resident -> raw_resident per chunk, nothing waited for.  Every event whose raw run ends by
    the last sample is in exactly one raw directory, CAPTURED, with iq[f : f + L] of the un-chunked array."""
    torch = torch_cuda
    bins, overlap, nrows, chunk = 1024, 768, 600, 200
    hop = bins - overlap
    shape = (bins, overlap, 48000)
    samples = bins + hop * (nrows - 1)
    iq = noise_iq(np.random.default_rng(31), samples, sigma=0.05)
    for f, spans in ((6000.0, ((189, 191), (203, 206), (450, 452))), (-9000.0, ((100, 101), (393, 395), (520, 524)))):
        for a, b in spans:
            add_chirp(iq, a * hop + 384, ((b - a) * hop + 256) / 48000.0, f, 0.0, 5.0)
    windows = [(300, 40), (628, 25)]
    cols = 65
    primary = ro.Bands(low_noise=100, noise_width=64, low_detect=630, detect_width=20, avg_bins=5)
    second = ro.Bands(low_noise=700, noise_width=64, low_detect=310, detect_width=20, avg_bins=5)
    dets = [(12, 4), (5, 3)]
    snap, ring_rows, cap, pcap = 40, 256, 24, 8
    stride = cols + 3
    arena_floats = cols * snap * 12
    dcap = 2 * (cap + pcap)
    raw_arena = 2 * L_of(shape, snap) * 8
    s = stream_of(torch)
    chunk_samples = (chunk - 1) * hop + bins
    d_iq = [torch.from_numpy(iq[k * chunk * hop:k * chunk * hop + chunk_samples].copy()).cuda() for k in range(3)]
    proto = SnapCase(ro, {0: [], 1: []}, snap, ring_rows, cols, 0, arena_floats, pcap=pcap, capacity=cap, stride=stride)
    raw_proto = Case(ro, shape, np.zeros(dcap, ro.capi.SNAPSHOT_DTYPE), [(0, 1, F32)], raw_arena, pcap=pcap)
    with ro.Stft(bins=bins, overlap=overlap, bands=primary, extra_bands=[second]) as st:
        d_rows = torch.zeros((chunk, bins), dtype=torch.float32, device="cuda")
        d_image = torch.zeros((chunk, cols), dtype=torch.float32, device="cuda")
        d_recs = torch.zeros((chunk * 12,), dtype=torch.uint8, device="cuda")
        d_extra = torch.zeros((chunk * 12,), dtype=torch.uint8, device="cuda")
        d_ring = torch.full((ring_rows * stride,), float(PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_state = torch.zeros((2 * 32,), dtype=torch.uint8, device="cuda")
        outs = [[up(torch, o) for o in snap_outputs_for(proto)] for _ in range(3)]
        raw_outs = [[up(torch, o) for o in outputs_for(raw_proto)] for _ in range(3)]
        d_events = [torch.full((2 * cap * 40,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_summary = [torch.zeros((2 * 24,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_pending, d_count = outs[0][2], outs[0][3]
        d_raw_pending, d_raw_count = raw_outs[0][2], raw_outs[0][3]
        torch.cuda.synchronize()
        for k in range(3):                                   # ---- nothing below waits for the device
            first = k * chunk
            st.run_resident_windows(d_iq[k], ro.RO_IQ_F32, chunk_samples, 0, chunk, d_rows, windows, d_image, d_records=d_recs,
                                    d_extra=d_extra, stream=s)
            st.ring_put_resident(d_image, first, chunk, ring, stream=s)
            st.events_resident(chunk, dets, d_state, d_records=d_recs, d_extra=d_extra, first_row=first, d_events=d_events[k],
                               capacity=cap, d_summary=d_summary[k], stream=s)
            st.snapshots_resident(3, snap, ring, first + chunk, d_pending, d_count, pcap, outs[k][0], outs[k][1], arena_floats,
                                  outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k], stream=s)
            spans = [(d_iq[j], j * chunk * hop, chunk_samples, ro.RO_IQ_F32) for j in range(max(k - 1, 0), k + 1)]
            st.raw_resident(outs[k][0], dcap, outs[k][4], spans, d_raw_pending, d_raw_count, pcap, raw_outs[k][0], raw_outs[k][1],
                            raw_arena, raw_outs[k][4], stream=s)
        torch.cuda.synchronize()
    for k in range(3):
        assert d_iq[k].cpu().numpy().tobytes() == iq[k * chunk * hop:k * chunk * hop + chunk_samples].tobytes(), "samples written"
    # the snapshots' directories, as the snapshots test reads them
    snaps = []
    for k in range(3):
        raw = [o.cpu().numpy() for o in outs[k]]
        if k:
            raw[2], raw[3] = snap_outputs_for(proto)[2], snap_outputs_for(proto)[3]
            raw[2][:], raw[3][:] = outs[0][2].cpu().numpy(), outs[0][3].cpu().numpy()
        snaps.append(SnapResult(ro, proto, *raw))
    # the raw directories: each call's against the host twin's chain over the un-chunked array, and by the closed form
    flat = iq.astype(np.float32)
    pending, count = np.zeros(pcap, ro.capi.SNAPSHOT_DTYPE), np.zeros(1, np.int64)
    seen, straddles, carried = [], [], []
    for k in range(3):
        raw = [o.cpu().numpy() for o in raw_outs[k]]
        directory = np.zeros(dcap, ro.capi.SNAPSHOT_DTYPE)
        directory[:len(snaps[k].dir)] = snaps[k].dir
        sm = np.zeros(1, ro.capi.SNAP_SUMMARY_DTYPE)
        sm[0] = snaps[k].summary
        before = int(count[0])
        base = max(k - 1, 0) * chunk * hop
        want_dir, want_arena, want_sm = ro.raw_host(*shape, directory, sm, [(flat[base:k * chunk * hop + chunk_samples], base, F32)],
                                                    pending, count, raw_arena)
        got_sm = raw[4][:64].view(ro.capi.RAW_SUMMARY_DTYPE)[0]
        n, used = int(got_sm["resolved"]), int(got_sm["arena_floats"])
        got_dir, got_arena = raw[0][:n * 72].view(ro.capi.RAW_CAPTURE_DTYPE), raw[1][:used * 4].view(np.float32)
        assert got_sm.tobytes() == want_sm.tobytes() and got_dir.tobytes() == want_dir.tobytes(), (k, got_sm, want_sm)
        assert got_arena.tobytes() == want_arena.tobytes()
        assert np.all(raw[0][n * 72:] == GUARD) and np.all(raw[1][used * 4:] == GUARD) and np.all(raw[4][64:] == GUARD)
        assert int(got_sm["lost"]) == 0 and int(got_sm["empty"]) == 0 and int(got_sm["pending_dropped"]) == 0
        assert n == int(snaps[k].summary["captured"]) + before - int(got_sm["pending"])
        boundary = k * chunk * hop                           # where the second span takes over
        for e in got_dir:
            assert e["status"] == CAPTURED
            start, f, L = int(e["event"]["start_row"]), int(e["first_sample"]), int(e["samples"])
            length = min(int(e["event"]["length"]), snap)
            assert f == (start * hop + 1 if start >= 1 else 0) and L == int(length / 187.0 * 48000) and f + L <= samples
            assert got_arena[int(e["offset"]):int(e["offset"]) + 2 * L].tobytes() == flat[f:f + L].tobytes(), (k, e)
            seen.append(e["event"])
            if k and f < boundary < f + L:
                straddles.append((k, f, L))
            if int(e["event"]["fire_row"]) // chunk < k:
                carried.append((k, f, L, int(e["event"]["fire_row"])))
    # the pending list exists once, in the first call's buffers: what the host twin's chain leaves
    assert raw_outs[0][2].cpu().numpy()[:pcap * 72].tobytes() == pending.tobytes()
    assert raw_outs[0][3].cpu().numpy()[:8].tobytes() == count.tobytes()
    # exactly once: every captured snapshot of the three snapshot directories has its raw run, except those whose run ends
    # behind the last sample, which still wait
    snapped = [e["event"] for r in snaps for e in r.dir if e["status"] == CAPTURED]
    waiting = [p["event"] for p in pending[:int(count[0])]]
    key = lambda ev: (int(ev["fire_row"]), int(ev["peak"]), int(ev["start_row"]))
    assert sorted([key(e) for e in seen] + [key(e) for e in waiting]) == sorted(key(e) for e in snapped)
    assert len(seen) >= 6 and all(f_of(shape, int(e["start_row"])) + L_of(shape, min(int(e["length"]), snap)) > samples for e in waiting)
    print("straddle two buffers: %s\ncarried: %s" % (straddles, carried))
    assert straddles and carried
