"""Addresses beyond 2^32 bytes and stream rows beyond 2^31: the case table and the layout arithmetic the CPU and the GPU
test walk (test infrastructure; tests/test_wide_offsets_cpu.py holds the table to its promises without a GPU,
tests/test_gpu_wide_offsets.py runs every case on the device).

Every device entry point takes 64-bit sample counts, rows, strides and offsets, and the kernels turn them into addresses
in many separately written places.  One `int` in one of them computes, instead of the true byte offset o of an element of
size e (index i = o / e), one of
    o mod 2^32,   o sign-extended from 32 bits,   (i mod 2^32) e,   (i sign-extended from 32 bits) e.
The GPU test owns ONE allocation, the arena of ARENA_BYTES = 2^34 + 2^28 bytes, and hands the library BASE = arena + 2^33
as its large pointer.  Every true offset of every case lies in [0, 2^33 + 2^28) from BASE, and then all four wrong
addresses lie inside the arena: a slip reads the arena's NaN fill or writes where the test looks afterwards -- a wrong
value, not a memory fault.  `wrong_addresses` computes the four, `extents` lists what a case reads or writes at BASE, and
the CPU test asserts the claim for every extent of every case.

The two thresholds, in bytes from BASE, and the quantity that passes an int32 / uint32 boundary there:
    2^32 bytes   RO_IQ_F32 sample 2^29, RO_IQ_I16 sample 2^30, RO_IQ_F64 sample 2^28, float index 2^30
    2^33 bytes   RO_IQ_F32 sample 2^30 (float index 2^31), RO_IQ_I16 sample 2^31, RO_IQ_F64 sample 2^29, float index 2^31

Three kinds of case, never combined: samples at BASE with a small output elsewhere (SAMPLE_CASES: three rows, the first
across the threshold, the others above it); small samples elsewhere with three output rows at BASE, 2^30 + 4 floats apart
(STRIDED_CASES: byte offsets 0, 2^32 + 16, 2^33 + 32); and small samples with one dense output of more than 2^32 bytes at
BASE (DENSE_CASES).

The last part is for the stream calls, whose rows and samples are counted from the stream's start: `translating` wraps a
`call` of tests/snapshotslib.py or tests/rawlib.py so that every case is also run K stream rows later and compared with
itself, on whatever voices the call holds (the host twin and the emulator on the CPU, the device and the host twin on
the GPU)."""
import copy
from collections import namedtuple

F32, F64 = 0, 1                       # RO_PRECISION_F32, RO_PRECISION_F64 (include/ro_stft.h)
IQ_F32, IQ_I16, IQ_F64 = 0, 1, 2      # RO_IQ_F32, RO_IQ_I16, RO_IQ_F64
SAMPLE_BYTES = {IQ_F32: 8, IQ_I16: 4, IQ_F64: 16}
FORMAT_NAMES = {IQ_F32: "f32", IQ_I16: "i16", IQ_F64: "f64"}

ARENA_BYTES = (1 << 34) + (1 << 28)   # 16.25 GiB
BASE = 1 << 33                        # byte offset of BASE inside the arena
ROOM = ARENA_BYTES - BASE             # bytes from BASE to the arena's end: 8.25 GiB
THRESHOLDS = (1 << 32, 1 << 33)
FILL_WORD = 0x7fc00000                # a quiet NaN as float32; two of them are a NaN as float64

STRIDE_FLOATS = (1 << 30) + 4         # rows at byte offsets 0, 2^32 + 16, 2^33 + 32
STRIDE_SPECTRA = (1 << 29) + 4        # in float2: spectra at byte offsets 0, 2^32 + 32, 2^33 + 64
ROWS = 3

# ---- the four wrong addresses -----------------------------------------------------------------------------------------


def sign_extend_32(v):
    return ((v & 0xffffffff) ^ 0x80000000) - 0x80000000


def wrong_addresses(offset, elem):
    """arena byte offsets of the four 32-bit slips for the element of `elem` bytes that holds byte `offset` from BASE:
    (byte offset mod 2^32, byte offset sign-extended, element index mod 2^32, element index sign-extended)"""
    index, within = divmod(offset, elem)
    return (BASE + (offset & 0xffffffff), BASE + sign_extend_32(offset),
            BASE + (index & 0xffffffff) * elem + within, BASE + sign_extend_32(index) * elem + within)


Extent = namedtuple("Extent", "what lo hi elems")        # bytes [lo, hi) from BASE; elems: the sizes an index of it may count


def probe_points(ext, elem):
    """every byte offset of the extent at which one of the four maps changes its branch, the byte in front of each, and the
    two ends: the maps are linear in between, so these carry the extremes"""
    pts = {ext.lo, ext.hi - 1}
    for period in (1 << 31, (1 << 31) * elem):
        m = (ext.lo // period + 1) * period
        while m < ext.hi:
            pts.update((m - 1, m))
            m += period
    return sorted(pts)


def landings(ext):
    """[(true offset, elem, (four arena offsets))] over the probe points of an extent"""
    return [(o, e, wrong_addresses(o, e)) for e in ext.elems for o in probe_points(ext, e)]


def inside_arena(address):
    return 0 <= address < ARENA_BYTES


# ---- the kernels the launchers can select (launch_transform, launch_stft, launch_f64reg, run_band in csrc/) ----------------
# path: "rows" (ro_stft_run_resident), "spectra" (ro_stft_spectra_resident), "band" (ro_stft_band_resident), "windows"
# (ro_stft_band_windows_resident); bins: the smallest size that selects the kernel; formats: what the handle accepts
Kernel = namedtuple("Kernel", "name path bins precision formats windows")
BOTH, ALL = (IQ_F32, IQ_I16), (IQ_F32, IQ_I16, IQ_F64)

KERNELS = (
    Kernel("stft_kernel<Plan256>", "rows", 256, F32, BOTH, ()),                       # the small single-pass plans
    Kernel("stft32k_kernel", "rows", 32768, F32, BOTH, ()),
    Kernel("one-kernel large form dec 2", "rows", 65536, F32, BOTH, ()),              # stft_kernel MODE 3
    Kernel("four-step pair", "rows", 262144, F32, BOTH, ()),                          # ro_fourstep.hip
    Kernel("chirp-z M 512", "rows", 258, F32, BOTH, ()),                              # ro_czt.cpp
    Kernel("f64reg 256 (16 rows per workgroup)", "rows", 256, F64, ALL, ()),          # ro_f64reg.hip
    Kernel("f64reg 4096", "rows", 4096, F64, ALL, ()),
    Kernel("f64reg 65536 (D x M)", "rows", 65536, F64, ALL, ()),
    Kernel("f64 through scratch 131072", "rows", 131072, F64, BOTH, ()),              # launch_transform_f64
    Kernel("spectra 256", "spectra", 256, F32, BOTH, ()),
    Kernel("spectra 65536 (fold, 32768, interleave)", "spectra", 65536, F32, BOTH, ()),
    # spectra of FP64 handles: f64r_kernel's SPEC instantiations, whose spec_store has one branch per plan shape
    Kernel("f64reg spectra 256 (16 rows per workgroup)", "spectra", 256, F64, ALL, ()),
    Kernel("f64reg spectra 4096 (D = 1)", "spectra", 4096, F64, ALL, ()),
    Kernel("f64reg spectra 65536 (D x M)", "spectra", 65536, F64, ALL, ()),
    Kernel("band 16384", "band", 16384, F32, BOTH, ((9000, 300),)),                   # ro_band.hip
    Kernel("band windows 16384", "windows", 16384, F32, BOTH, ((100, 40), (9000, 260))),
    Kernel("f64 band 131072", "band", 131072, F64, ALL, ((70000, 300),)),             # ro_band_f64.hip
    Kernel("f64 band windows 131072", "windows", 131072, F64, ALL, ((40000, 100), (90000, 120))),
)
ENTRY_OF_PATH = {"rows": "ro_stft_run_resident", "spectra": "ro_stft_spectra_resident", "band": "ro_stft_band_resident",
                 "windows": "ro_stft_band_windows_resident"}
# what each sample-reading entry point accepts on some handle (validate_resident, check_band_handle): doubles on the FP64
# handles of the register kernel's sizes (rows and spectra) and on the FP64 band kernels
ACCEPTS = {"ro_stft_run_resident": ALL, "ro_stft_spectra_resident": ALL, "ro_stft_band_resident": ALL,
           "ro_stft_band_windows_resident": ALL}


def kernel(name):
    return next(k for k in KERNELS if k.name == name)


def hop(k):
    """three quarters of a row (193 of 258): no power of two divides the thresholds' sample indices into whole hops, so a
    row can start below one and end above it"""
    return 193 if k.bins == 258 else 3 * k.bins // 4


def overlap(k):
    return k.bins - hop(k)


def cols(k):
    return sum(n for _, n in k.windows)


def width(k):
    """floats (spectra: complex pairs) of one output row"""
    return cols(k) if k.windows else k.bins


def bands_of(bins):
    """(low_noise, noise_width, low_detect, detect_width, avg_bins) and the tile (first_col, cols) of the transform cases:
    a noise band in the row's first quarter, a detect band and a tile beyond its middle"""
    return (bins // 16, bins // 8 if bins <= 4096 else 410, bins // 2 + bins // 8, bins // 16 if bins <= 4096 else 136, 3), \
        (bins // 2 + bins // 8 - 20, 45)


# ---- 1. samples at BASE -----------------------------------------------------------------------------------------------
SampleCase = namedtuple("SampleCase", "kernel fmt threshold")
SAMPLE_CASES = tuple(SampleCase(k, f, t) for k in KERNELS for f in k.formats for t in THRESHOLDS)


def threshold_sample(c):
    return c.threshold // SAMPLE_BYTES[c.fmt]


def first_row(c):
    """the last row that starts below the threshold"""
    return (threshold_sample(c) - 1) // hop(c.kernel)


def first_sample(c):
    return first_row(c) * hop(c.kernel)


def samples(c):
    """what ro_row_count turns into exactly first_row + ROWS rows"""
    return (first_row(c) + ROWS - 1) * hop(c.kernel) + c.kernel.bins


def tail_samples(c):
    """the samples the three rows read, and all that is written into the arena"""
    return samples(c) - first_sample(c)


def sample_id(c):
    return "%s %s 2^%d" % (c.kernel.name, FORMAT_NAMES[c.fmt], c.threshold.bit_length() - 1)


def sample_extents(c):
    b = SAMPLE_BYTES[c.fmt]
    return [Extent("samples", first_sample(c) * b, samples(c) * b, (b, b // 2))]      # (counted in samples or in numbers)


# ---- 2. three output rows at BASE, 2^30 + 4 floats apart ---------------------------------------------------------------
# entry: the call under test; kernel: the transform behind it (None: rows that are already there); role: what lies at BASE --
# "out" the call's output rows, "image" its window image, "in" the rows it reads, "ring" the ring it fills and reads
StridedCase = namedtuple("StridedCase", "name entry kernel role row_floats stride_floats")
READER_BINS = 1024                                        # the readers' rows and the window cuts
READER_WINDOWS = ((100, 40), (600, 25))
RING_COLS = 65


def _strided():
    out = []
    for k in KERNELS:
        comp = 2 if k.path == "spectra" else 1
        out.append(StridedCase("%s: %s" % (ENTRY_OF_PATH[k.path][8:], k.name), ENTRY_OF_PATH[k.path], k, "out", width(k) * comp,
                               STRIDE_SPECTRA * 2 if comp == 2 else STRIDE_FLOATS))
    image = sum(n for _, n in READER_WINDOWS)
    out.append(StridedCase("run_resident_windows: image", "ro_stft_run_resident_windows", None, "image", image, STRIDE_FLOATS))
    out.append(StridedCase("cut_windows_resident: image", "ro_stft_cut_windows_resident", None, "image", image, STRIDE_FLOATS))
    for entry in ("ro_stft_scan_resident", "ro_stft_scan_sets_resident", "ro_stft_ln_tile_resident",
                  "ro_stft_cut_windows_resident"):
        out.append(StridedCase("%s: rows" % entry[8:], entry, None, "in", READER_BINS, STRIDE_FLOATS))
    out.append(StridedCase("ring_put_resident, snapshots_resident: ring", "ro_stft_ring_put_resident", None, "ring", RING_COLS,
                           STRIDE_FLOATS))
    return tuple(out)


STRIDED_CASES = _strided()


def strided(name):
    return next(c for c in STRIDED_CASES if c.name == name)


def strided_extents(c):
    elems = (8, 4) if c.entry == "ro_stft_spectra_resident" else (4,)
    return [Extent("row %d" % r, r * c.stride_floats * 4, r * c.stride_floats * 4 + c.row_floats * 4, elems)
            for r in range(ROWS)]


# ---- 3. one dense output of more than 2^32 bytes ------------------------------------------------------------------------
# rows: 256 bins, overlap 255, 2^22 + 3 rows of 1 KiB and the whole-row tile behind them; band: 16384 bins, 1024 columns,
# 2^20 + 3 rows of 4 KiB -- the smallest row counts that pass 2^32 bytes with a row on either side of it
DenseCase = namedtuple("DenseCase", "name entry bins precision rows row_floats tile")
DENSE_CASES = (
    DenseCase("rows 256 float32", "ro_stft_run_resident", 256, F32, (1 << 22) + 3, 256, True),
    DenseCase("rows 256 FP64", "ro_stft_run_resident", 256, F64, (1 << 22) + 3, 256, True),
    DenseCase("band 16384 x 1024", "ro_stft_band_resident", 16384, F32, (1 << 20) + 3, 1024, False),
)
DENSE_BAND = (7680, 1024)                                 # (first_col, cols) of the dense band case


def dense(name):
    return next(c for c in DENSE_CASES if c.name == name)


def dense_extents(c):
    n = c.rows * c.row_floats * 4
    out = [Extent("rows", 0, n, (4,))]
    if c.tile:
        out.append(Extent("tile", n, 2 * n, (4,)))
    return out


def dense_probe_rows(c):
    """the rows compared with separate one-row calls: the first, either side of byte 2^32, the last"""
    at = (1 << 32) // (c.row_floats * 4)
    return [0, at - 1, at, c.rows - 1]


# ---- what every case crosses --------------------------------------------------------------------------------------------
Crossing = namedtuple("Crossing", "entry threshold quantity index fmt")     # `quantity` reaches `index` at `threshold` bytes


def crossings(c):
    """the thresholds a case crosses, and by which quantity"""
    if isinstance(c, SampleCase):
        entry, b = ENTRY_OF_PATH[c.kernel.path], SAMPLE_BYTES[c.fmt]
        assert first_sample(c) * b < c.threshold < (first_sample(c) + c.kernel.bins) * b      # a row across it
        assert (first_sample(c) + hop(c.kernel)) * b >= c.threshold                            # ... and the next above it
        return [Crossing(entry, c.threshold, "sample", c.threshold // b, c.fmt),
                Crossing(entry, c.threshold, "number", 2 * c.threshold // b, c.fmt)]
    exts = strided_extents(c) if isinstance(c, StridedCase) else dense_extents(c)
    lo, hi = min(e.lo for e in exts), max(e.hi for e in exts)
    entries = [c.entry] + (["ro_stft_snapshots_resident"] if getattr(c, "role", "") == "ring" else [])
    return [Crossing(e, t, "float", t // 4, None) for e in entries for t in THRESHOLDS if lo < t < hi]


def extents(c):
    if isinstance(c, SampleCase):
        return sample_extents(c)
    return strided_extents(c) if isinstance(c, StridedCase) else dense_extents(c)


def all_cases():
    return list(SAMPLE_CASES) + list(STRIDED_CASES) + list(DENSE_CASES)


# the entry points the issue lists: each crossed at both thresholds by some case
SAMPLE_ENTRIES = tuple(sorted(set(ENTRY_OF_PATH.values())))
OUTPUT_ENTRIES = SAMPLE_ENTRIES + ("ro_stft_run_resident_windows", "ro_stft_cut_windows_resident", "ro_stft_scan_resident",
                                   "ro_stft_scan_sets_resident", "ro_stft_ln_tile_resident", "ro_stft_ring_put_resident",
                                   "ro_stft_snapshots_resident")


# ---- 4. long streams: translation by K rows -----------------------------------------------------------------------------
def snapshot_shift(ring_rows):
    """K = 2^33 + k, the smallest such multiple of ring_rows: stream row r + K lives in row r's slot"""
    return -(-(1 << 33) // ring_rows) * ring_rows


RAW_SHIFT = 1 << 36                   # rows; first_sample rises by RAW_SHIFT x hop (2^44 at a hop of 256)
EVENTS_SHIFT = (1 << 33) + 5


def _rows_moved(a, fields, k):
    """a copy of a structured array with k added to the named int64 fields; "event.x" names a field of the nested event"""
    out = a.copy()
    for f in fields:
        view = out
        for part in f.split("."):
            view = view[part]
        view += k
    return out


EVENT_ROWS = ("start_row", "fire_row")
SNAPSHOT_ROWS = ("event.start_row", "event.fire_row", "first_row")


def _used(count, capacity):
    return min(max(int(count), 0), capacity)


def snapshot_translatable(case):
    """whether every candidate of a snapshotslib.Case starts at row 0 or later: max(start_row, 0) is the one rule of the
    snapshots that does not move with the stream, so a case with a negative start is left where it is"""
    for s in range(case.slots):
        if not (case.mask >> s) & 1:
            continue
        listed = _used(case.summary["events"][s], case.capacity) if case.summary is not None else 0
        starts = list(case.pending["start_row"][s, :_used(case.pending_count[s], case.pcap)]) + \
            list(case.events["start_row"][s, :listed])
        if any(int(x) < 0 for x in starts):
            return False
    return True


def shift_snapshot_case(case, k):
    """the same call k stream rows later: events, pending lists and head row raised, the ring's floats as they are (k is a
    multiple of ring_rows, so every row keeps its slot)"""
    assert k % case.ring.shape[0] == 0
    moved = copy.copy(case)
    moved.events = _rows_moved(case.events, EVENT_ROWS, k)
    moved.pending = _rows_moved(case.pending, EVENT_ROWS, k)
    moved.pending_count = case.pending_count.copy()
    moved.head_row = case.head_row + k
    return moved


def same_snapshots_after_shift(base, moved, k):
    """two snapshotslib.Result: the moved one is the base one with first_row and the event rows raised by k -- the same
    directory otherwise, the same arena bytes, pending lists, counts and summary"""
    assert moved.summary.tobytes() == base.summary.tobytes(), (moved.summary, base.summary)
    assert _rows_moved(moved.dir, SNAPSHOT_ROWS, -k).tobytes() == base.dir.tobytes(), (moved.dir, base.dir)
    assert moved.arena.tobytes() == base.arena.tobytes()
    assert _rows_moved(moved.pending, EVENT_ROWS, -k).tobytes() == base.pending.tobytes()
    assert moved.pending_count.tobytes() == base.pending_count.tobytes()


def raw_hop(case):
    bins, overlap = case.shape[0], case.shape[1]
    return bins - (0 if overlap < 0 else bins - 1 if overlap >= bins else overlap)


def raw_translatable(case):
    """whether every candidate of a rawlib.Case starts at row 1 or later: first_sample is 0 for every start below 1, the
    one rule of the raw capture that does not move with the stream"""
    listed = _used(case.snap_summary["resolved"][0], case.dcap)
    starts = list(case.pending["event"]["start_row"][:_used(case.pending_count[0], case.pcap)]) + \
        list(case.directory["event"]["start_row"][:listed])
    return all(int(x) >= 1 for x in starts)


def shift_raw_case(case, k):
    """the same call k stream rows later: the directory's and the pending list's rows raised by k, every span's
    first_sample by k x hop, the samples themselves as they are"""
    by = k * raw_hop(case)
    moved = copy.copy(case)
    moved.directory = _rows_moved(case.directory, SNAPSHOT_ROWS, k)
    moved.pending = _rows_moved(case.pending, SNAPSHOT_ROWS, k)
    moved.pending_count = case.pending_count.copy()
    moved.spans = [(a, first + by, fmt) for a, first, fmt in case.spans]
    moved.layout = [(first + by, count, fmt) for first, count, fmt in case.layout]
    return moved


def same_raw_after_shift(case, base, moved, k):
    """two rawlib.Result: run bytes, statuses, `samples` and offsets unchanged, first_sample raised by k x hop"""
    by = k * raw_hop(case)
    assert moved.summary.tobytes() == base.summary.tobytes(), (moved.summary, base.summary)
    back = _rows_moved(_rows_moved(moved.dir, ("event.start_row", "event.fire_row"), -k), ("first_sample",), -by)
    assert back.tobytes() == base.dir.tobytes(), (moved.dir, base.dir)
    assert moved.arena.tobytes() == base.arena.tobytes()
    assert _rows_moved(moved.pending, SNAPSHOT_ROWS, -k).tobytes() == base.pending.tobytes()
    assert moved.pending_count.tobytes() == base.pending_count.tobytes()


def translating(call, translatable, shift, same, k_of, counter):
    """`call` with the translation check around it: every translatable case is also run k rows later, through the very same
    voices, and compared with itself; the result handed on is the unmoved one, so a decision table walks on as it was"""
    def wrapped(case):
        base = call(case)
        if translatable(case):
            k = k_of(case)
            same(case, base, call(shift(case, k)), k)
            counter[0] += 1
        else:
            counter[1] += 1
        return base
    return wrapped


def translating_snapshots(call, counter):
    return translating(call, snapshot_translatable, shift_snapshot_case, lambda case, a, b, k: same_snapshots_after_shift(a, b, k),
                       lambda case: snapshot_shift(case.ring.shape[0]), counter)


def translating_raw(call, counter):
    return translating(call, raw_translatable, shift_raw_case, same_raw_after_shift, lambda case: RAW_SHIFT, counter)


# ---- cases of the long streams that both test files run -------------------------------------------------------------------
def ring_255_cases(ro):
    """a ring of 255 rows, not a power of two: `%` is a real division.  Head 600: rows 345 ... 599 are in the ring, row 510
    in slot 0; snapshots across the ring's end, at its first row, one row too old, and one still to come.  Returns the first
    call's case and what makes the second call's from the first one's result"""
    import snapshotslib
    C = snapshotslib.Case
    first = C(ro, {0: [(500, 20), (345, 7), (344, 7), (590, 20)], 3: [(505, 9), (598, 2)]}, 25, 255, 7, 600, 4000, pcap=3)
    return first, lambda r: C(ro, {0: [(640, 5)], 3: []}, 25, 255, 7, 650, 4000, pcap=3, mask=9).carry(r)


ODD_HOP_SHAPES = [(256, 1, 1000), (256, 0, 4000), (256, 253, 9)]                       # (bins, overlap, rate): hops 255, 256, 3


def odd_hop_case(ro, shape, call):
    """raw capture: snapshots of 5 rows at rows 6, 7, 9 and 11 over an int16 span and a double span that takes over inside
    the second run; the fourth run's samples have not arrived"""
    import rawlib
    hop = shape[0] - shape[1]
    f = [rawlib.f_of(shape, s) for s in (6, 7, 9)]
    L = rawlib.L_of(shape, 5)
    assert L > 0 and RAW_SHIFT * hop >= (1 << 36) and (hop != 256 or RAW_SHIFT * hop == 1 << 44)
    mid = f[1] + L // 2
    layout = [(f[0], mid - f[0] + 3, rawlib.I16), (mid, f[2] + L - mid, rawlib.F64)]
    case = rawlib.Case(ro, shape, [(6, 5), (7, 5), (9, 5), (11, 5)], layout, 6 * 2 * L)
    r = call(case)
    assert rawlib.statuses(r) == [rawlib.CAPTURED] * 3 and r.pending_count[0] == 1
    for i, s in enumerate((6, 7, 9)):
        rawlib.captured_ok(case, r, i, s, 5)
