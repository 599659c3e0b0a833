"""GPU checks of the compressed preview files on the device (csrc/ro_png_deflate.hip): every level image of a level directory
as a complete PNG whose deflate blocks are Huffman coded where that is shorter.  The yardstick is the twin,
ro_levels_png_deflate_host, which tests/test_png_deflate_cpu.py holds to pngdeflatelib's restatement of the stream: every output
of the device call equals the twin's byte for byte -- directory, summary, files, the pad behind each file, the guards, the
untouched tail -- and the sources come back unwritten.  Every case runs twice with equal bytes; one case per test is
additionally walked with zlib and Pillow straight from the device's bytes.  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import periodiclib as P
import pngdeflatelib as D
import pnglib as G
import unitslib as U
from levelslib import LBLOCK
from levelslib import outputs_for as level_outputs_for
from pnglib import GUARD, NGUARD, SHAPES, WRITTEN
from snapshotslib import Case as SnapCase
from snapshotslib import outputs_for as snap_outputs_for
from test_gpu_levels import chain_input

pytestmark = pytest.mark.gpu


@pytest.fixture()
def st(ro, torch_cuda):
    with ro.Stft(bins=256, overlap=0) as handle:
        yield handle


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def device_call(ro, torch, st, case):
    d_dir = up(torch, case.level_dir) if len(case.level_dir) else None
    d_summary, d_levels = up(torch, case.summary), up(torch, case.levels) if case.levels.size else None
    d_outs = [up(torch, o) for o in G.outputs_for(case)]
    st.levels_png_deflate_resident(d_dir if case.dcap else None, case.dcap, d_summary, d_levels, case.levels.size, d_outs[0],
                                   d_outs[1] if case.png_bytes else None, case.png_bytes, d_outs[2], stream=stream_of(torch))
    torch.cuda.synchronize()
    assert d_dir is None or d_dir.cpu().numpy().tobytes() == case.level_dir.tobytes(), "the level directory was written"
    assert d_summary.cpu().numpy().tobytes() == case.summary.tobytes()
    assert d_levels is None or d_levels.cpu().numpy().tobytes() == case.levels.tobytes(), "the levels were written"
    return D.Result(ro, case, *[o.cpu().numpy() for o in d_outs])


def device_checked(ro, torch, st, walked):
    def call(case):
        got = device_call(ro, torch, st, case)
        want = D.host_call(ro, case)
        assert got.summary.tobytes() == want.summary.tobytes(), (got.summary, want.summary)
        assert got.dir.tobytes() == want.dir.tobytes(), (got.dir, want.dir)
        for d in got.written():
            assert got.file(d).tobytes() == want.file(d).tobytes(), "file %d differs from the twin's" % d
        assert got.same_bytes(want), "an output differs from the twin's"
        assert device_call(ro, torch, st, case).same_bytes(got), "two runs differ"
        if not walked and got.written():
            D.check_files(case, got)
            walked.append(True)
        return got
    return call


@pytest.mark.parametrize("case_fn", D.TABLE, ids=lambda f: f.__name__)
def test_decision_table_on_the_device(ro, torch_cuda, st, case_fn):
    walked = []
    case_fn(ro, device_checked(ro, torch_cuda, st, walked))
    assert walked


@pytest.mark.parametrize("content", D.CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shape_table_on_the_device(ro, torch_cuda, st, shape, content):
    walked = []
    case = D.shape_case(ro, *shape, content)
    r = device_checked(ro, torch_cuda, st, walked)(case)
    assert G.statuses(r) == [WRITTEN, WRITTEN] and walked
    need = int(r.summary["needed_bytes"])
    short = device_checked(ro, torch_cuda, st, walked)(case.with_room(need - 1))
    assert G.statuses(short) == [WRITTEN, G.NO_ROOM] and short.dir["bytes"].tolist() == r.dir["bytes"].tolist()
    sizing = device_checked(ro, torch_cuda, st, walked)(case.with_room(0))
    assert int(sizing.summary["needed_bytes"]) == need and G.statuses(sizing) == [G.NO_ROOM, G.NO_ROOM]


def test_all_shapes_in_one_call(ro, torch_cuda, st):
    """the shape table as one directory, every content in turn: blocks of several files share the launches, a workgroup takes
    several, and the files are packed by their actual sizes.  The sizing call first, then exactly that room"""
    shapes = SHAPES + SHAPES[1:] + SHAPES[1:]
    d, levels = G.images(ro, [D.pixels_of(c, w, h, 7) for (w, h), c in zip(shapes, D.CONTENTS * 4)])
    walked = []
    call = device_checked(ro, torch_cuda, st, walked)
    full, rooms = D.sized(call, G.Case(ro, d, levels, 0))
    assert G.statuses(full) == [WRITTEN] * len(shapes)
    assert sum(rooms) < sum(G.room_of(w, h) for w, h in shapes) * 3 // 4
    D.check_files(G.Case(ro, d, levels, sum(rooms)), full, walk_them=False)


def test_overlapping_images_beyond_the_block_bound_on_the_device(ro, torch_cuda, st):
    d, levels = G.images(ro, [D.pixels_of("noise", 300, 250)])
    r = device_checked(ro, torch_cuda, st, [])(G.Case(ro, np.repeat(d, 9), levels, 9 * G.room_of(300, 250)))
    assert G.statuses(r) == [WRITTEN] * 6 + [G.INVALID] * 3


def test_refusals_with_a_handle(ro, torch_cuda, st):
    torch = torch_cuda
    lib = ro.library()
    d, levels = G.images(ro, [G.small(1, 6, 10)])
    room = G.room_of(6, 10)
    case = G.Case(ro, d, np.concatenate([levels, np.zeros(room, np.uint8)]), room)
    d_dir, d_sum, d_levels = up(torch, d), up(torch, case.summary), up(torch, case.levels)
    d_outs = [up(torch, o) for o in G.outputs_for(case)]
    ptr = lambda t: t.data_ptr()

    def call(**kw):
        a = dict(level_dir=ptr(d_dir), dcap=1, summary=ptr(d_sum), levels=ptr(d_levels), levels_bytes=LBLOCK, png_dir=ptr(d_outs[0]),
                 png=ptr(d_outs[1]), png_bytes=room, out=ptr(d_outs[2]))
        a.update(kw)
        if a["png"] == "levels":
            a["png"] = ptr(d_levels) + LBLOCK - 16                    # its first 16 bytes are the levels' last
        elif a["png"] == "levels end":
            a["png"] = ptr(d_levels) - room + 16                      # its last 16 bytes are the levels' first
        return lib.ro_stft_levels_png_deflate_resident(st._h, a["level_dir"], a["dcap"], a["summary"], a["levels"], a["levels_bytes"],
                                                       a["png_dir"], a["png"], a["png_bytes"], a["out"], stream_of(torch))
    assert ptr(d_levels) % 16 == 0 and room % 16 == 0
    for kw, word in G.refusals("d_") + [(dict(png=ptr(d_outs[1]) + 8), "d_png is not aligned")]:
        assert call(**kw) == -1, kw
        text = lib.ro_last_error().decode()
        assert word in text and text.startswith("ro_stft_levels_png_deflate_resident:"), (kw, text)
    torch.cuda.synchronize()
    for o, before in zip(d_outs, G.outputs_for(case)):
        assert o.cpu().numpy().tobytes() == before.tobytes(), "a refused call launched something"
    assert call(png=None, png_bytes=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert d_outs[2].cpu().numpy()[:64].view(ro.capi.UNIT_SUMMARY_DTYPE)["written"][0] == 1


# ---- the chain, nothing waited for in between ----------------------------------------------------------------------------------
def test_samples_to_compressed_png_files_in_three_chunks(ro, torch_cuda):
    """test_gpu_png.test_samples_to_png_files_in_three_chunks's event-snapshot leg with the compressed call behind
    snapshot_levels_resident, per chunk on one stream, nothing waited for.  Every chunk's files are the twin's over the levels
    the device left, and walk against those levels"""
    torch = torch_cuda
    bins, overlap = 256, 192
    hop = bins - overlap
    chunks = [(0, 61), (61, 90), (151, 49)]
    iq, windows, cols, primary, det, snap = chain_input(ro)
    stride, ring_rows, cap, pcap = cols + 3, 128, 8, 4
    slot_windows = [(30, 21)]
    arena_floats = cols * snap * 6
    dcap = cap + pcap
    levels_room, png_room = 8 * LBLOCK, 16384
    s = stream_of(torch)
    d_iq = [torch.from_numpy(iq[a * hop:a * hop + (n - 1) * hop + bins].copy()).cuda() for a, n in chunks]
    proto = SnapCase(ro, {0: []}, snap, ring_rows, cols, 0, arena_floats, pcap=pcap, capacity=cap, stride=stride)
    level_case = U.Case(ro, "image", np.zeros(dcap, ro.capi.SNAPSHOT_DTYPE), 0, levels_room, cols, slot_windows + [(0, 0)] * 7)
    png_outs = lambda n: [G.guarded(n * 32, NGUARD * 32), G.guarded(png_room, NGUARD * 64), G.guarded(64, NGUARD * 64)]
    with ro.Stft(bins=bins, overlap=overlap, bands=primary) as st:
        d_rows = torch.zeros((90, bins), dtype=torch.float32, device="cuda")
        d_image = [torch.zeros((n, cols), dtype=torch.float32, device="cuda") for _, n in chunks]
        d_recs = torch.zeros((90 * 12,), dtype=torch.uint8, device="cuda")
        d_ring = torch.full((ring_rows * stride,), float(P.PAD), dtype=torch.float32, device="cuda")
        ring = ro.capi.RowRing(d_ring.data_ptr(), stride, ring_rows, cols, 0)
        d_state = torch.zeros((32,), dtype=torch.uint8, device="cuda")
        outs = [[up(torch, o) for o in snap_outputs_for(proto)] for _ in chunks]
        d_events = [torch.full((cap * 40,), GUARD, dtype=torch.uint8, device="cuda") for _ in chunks]
        d_summary = [torch.zeros((24,), dtype=torch.uint8, device="cuda") for _ in chunks]
        d_pending, d_count = outs[0][2], outs[0][3]
        d_levels = [[up(torch, o) for o in level_outputs_for(level_case)] for _ in chunks]
        d_png = [[up(torch, o) for o in png_outs(dcap)] for _ in chunks]
        torch.cuda.synchronize()
        for k, (first, n) in enumerate(chunks):              # ---- nothing below waits for the device
            st.run_resident_windows(d_iq[k], ro.RO_IQ_F32, (n - 1) * hop + bins, 0, n, d_rows, windows, d_image[k], d_records=d_recs,
                                    stream=s)
            st.ring_put_resident(d_image[k], first, n, ring, stream=s)
            st.events_resident(n, [det], d_state, d_records=d_recs, first_row=first, d_events=d_events[k], capacity=cap,
                               d_summary=d_summary[k], stream=s)
            st.snapshots_resident(1, snap, ring, first + n, d_pending, d_count, pcap, outs[k][0], outs[k][1], arena_floats,
                                  outs[k][4], d_events=d_events[k], capacity=cap, d_summary=d_summary[k], stream=s)
            st.snapshot_levels_resident(outs[k][0], dcap, outs[k][4], outs[k][1], arena_floats, cols, slot_windows, d_levels[k][0],
                                        d_levels[k][1], d_levels[k][2], levels_room, d_levels[k][3], stream=s)
            st.levels_png_deflate_resident(d_levels[k][0], dcap, d_levels[k][3], d_levels[k][2], levels_room, d_png[k][0],
                                           d_png[k][1], png_room, d_png[k][2], stream=s)
        torch.cuda.synchronize()
    event_files = 0
    for k in range(len(chunks)):
        got_levels = [o.cpu().numpy() for o in d_levels[k]]
        case = G.Case(ro, got_levels[0][:dcap * 32].view(ro.capi.FITS_UNIT_DTYPE).copy(), got_levels[2][:levels_room], png_room, dcap=dcap)
        case.summary = got_levels[3][:64].view(ro.capi.UNIT_SUMMARY_DTYPE).copy()
        got = D.Result(ro, case, *[o.cpu().numpy() for o in d_png[k]])
        assert got.same_bytes(D.host_call(ro, case)), "chunk %d: the event files differ from the twin's" % k
        D.check_files(case, got)
        assert int(got.summary["no_room"]) == 0 and int(got.summary["invalid"]) == 0
        event_files += len(got.written())
    print("files written: %d of event snapshots" % event_files)
    assert event_files >= 1


# ---- addressing ------------------------------------------------------------------------------------------------------------------
def test_compressed_files_beyond_4_gib(ro, torch_cuda, st):
    """four entries over one image of 32767 x 43700 six-bit levels, 21851 blocks each, whose compressed files together pass 2^32
    bytes, and a small image behind them: the sizing call gives the room; the four files are equal on the device; the first
    one's IDAT CRC and Adler-32 are zlib's over the download, its first and last block are the restatement's and inflate; the
    small file is the twin's.  About 7.5 GiB of device memory: the levels hold the image once, and as much again unused, which
    is what lets four entries' blocks be measured"""
    torch = torch_cuda
    w, h = 32767, 43700
    pixels, image_room = w * h, -(-w * h // LBLOCK) * LBLOCK
    small = D.pixels_of("noise", 615, 37, 5)
    d = np.zeros(5, ro.capi.FITS_UNIT_DTYPE)
    for i in range(4):
        d[i] = (0, pixels, h, w, WRITTEN)
    d[4] = (2 * image_room, small.size, 37, 615, WRITTEN)
    levels_bytes = 2 * image_room + LBLOCK * -(-small.size // LBLOCK) + 400 * LBLOCK        # (and a few blocks' worth more)
    assert h * (w + 1) < 1 << 31 and levels_bytes // 65535 * 2 + 1 + 5 >= 4 * 21851 + 1
    d_levels = torch.empty(levels_bytes, dtype=torch.uint8, device="cuda")
    step = 1 << 26
    for at in range(0, pixels, step):                       # a pattern whose period no scanline shares, built on the device
        i = torch.arange(at, min(at + step, pixels), dtype=torch.int64, device="cuda")
        d_levels[at:at + len(i)] = (((i * 40503 + (i >> 9)) >> 3) & 63).to(torch.uint8)
        del i
    d_levels[2 * image_room:2 * image_room + small.size] = torch.from_numpy(small.reshape(-1)).cuda()
    sm = np.zeros(1, ro.capi.UNIT_SUMMARY_DTYPE)
    sm["entries"] = 5
    d_dir, d_sum = up(torch, d), up(torch, sm)
    d_png_dir, d_png_sum = torch.zeros(5 * 32, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    st.levels_png_deflate_resident(d_dir, 5, d_sum, d_levels, levels_bytes, d_png_dir, None, 0, d_png_sum, stream=stream_of(torch))
    torch.cuda.synchronize()
    sizing = d_png_sum.cpu().numpy().view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
    png_bytes = int(sizing["needed_bytes"])
    sized_dir = d_png_dir.cpu().numpy().view(ro.capi.FITS_UNIT_DTYPE).copy()
    assert sized_dir["status"].tolist() == [G.NO_ROOM] * 5 and int(sizing["written"]) == 0
    big = int(sized_dir["bytes"][0])
    big_room = D.room_of_bytes(big)
    assert sized_dir["bytes"].tolist()[:4] == [big] * 4 and big < G.file_bytes(w, h) * 4 // 5
    assert png_bytes == 4 * big_room + D.room_of_bytes(int(sized_dir["bytes"][4])) and 4 * big_room > 1 << 32
    d_png = torch.full((png_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    st.levels_png_deflate_resident(d_dir, 5, d_sum, d_levels, levels_bytes, d_png_dir, d_png, png_bytes, d_png_sum, stream=stream_of(torch))
    torch.cuda.synchronize()
    png_dir = d_png_dir.cpu().numpy().view(ro.capi.FITS_UNIT_DTYPE)
    out = d_png_sum.cpu().numpy().view(ro.capi.UNIT_SUMMARY_DTYPE)[0]
    assert png_dir["status"].tolist() == [WRITTEN] * 5 and png_dir["offset"].tolist() == [k * big_room for k in range(5)]
    assert png_dir["bytes"].tolist() == sized_dir["bytes"].tolist() and int(out["units_bytes"]) == png_bytes == int(out["needed_bytes"])
    assert bool((d_png[png_bytes:] == GUARD).all()), "bytes past the files were touched"
    for k in (1, 2, 3):
        assert torch.equal(d_png[:big_room], d_png[k * big_room:(k + 1) * big_room]), "file %d differs from file 0" % k
    # the small file behind 2^32 is the twin's
    scase = G.Case(ro, *G.images(ro, [small]), G.room_of(615, 37))
    want = D.host_call(ro, scase)
    assert d_png[4 * big_room:png_bytes].cpu().numpy().tobytes() == want.png.tobytes()
    # the first file against zlib over the downloaded levels
    data = d_png[:big_room].cpu().numpy()
    assert not data[big:].any()
    px = d_levels[:pixels].cpu().numpy().reshape(h, w)
    raw = np.zeros((h, w + 1), np.uint8)
    raw[:, 1:] = px
    raw = raw.reshape(-1)
    idat = big - 57
    assert data[:33].tobytes() == G.SIGNATURE + G.chunk(b"IHDR", np.array([w, h], ">u4").tobytes() + bytes([8, 0, 0, 0, 0]))
    assert data[33:43].tobytes() == np.array([idat], ">u4").tobytes() + b"IDAT\x78\x01"
    adler = zlib.adler32(raw)
    crc = zlib.crc32(data[37:41 + idat])
    assert data[big - 20:big].tobytes() == np.array([adler, crc], ">u4").tobytes() + G.IEND
    first, _ = D.huffman_block(raw[:G.STORED].tobytes(), False)
    last_raw = raw[len(raw) // G.STORED * G.STORED:].tobytes()
    last, _ = D.huffman_block(last_raw, True)
    assert data[43:43 + len(first)].tobytes() == first and data[big - 20 - len(last):big - 20].tobytes() == last
    inflate = zlib.decompressobj(-15)
    assert inflate.decompress(first, G.STORED) == raw[:G.STORED].tobytes()
    assert zlib.decompress(last, -15) == last_raw
