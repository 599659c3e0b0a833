"""tests/chunk_seams.py's case table against the library's constants and its CPU-side C ABI, without a GPU: every case
crosses the seams it was written for, with rows on both sides, and is a call the ABI accepts.  A change of one of
csrc/ro_host.h's RO_*_SCRATCH_MB defaults that leaves a case inside one chunk fails here."""
import os

import pytest

import chunk_seams as S


def test_the_header_states_the_three_scratch_defaults():
    found = S.header_defaults()
    for name in ("RO_SPEC_SCRATCH_MB", "RO_FOUR_SCRATCH_MB", "RO_F64_SCRATCH_MB"):
        assert found.get(name, 0) > 0, (name, found)


def test_every_family_and_path_is_in_the_table():
    assert {c.family for c in S.CASES} == {"f64", "spectra", "czt", "four", "band"}
    band = {(c.path, c.precision, S.chunk_rows(c) == S.GRID_ROWS) for c in S.CASES if c.family == "band"}
    # all four band families at the 65535-row cap; at the 256 MiB seam all but the single-window FP64 band, which
    # tests/test_gpu_band_f64.py::test_chunk_boundary crosses
    assert {(p, q, True) for p in ("band", "windows") for q in (S.F32, S.F64)} <= band
    assert {("band", S.F32, False), ("windows", S.F32, False), ("windows", S.F64, False)} <= band
    assert len({c.name for c in S.CASES}) == len(S.CASES)
    assert set(S.BANDS) == {c.name for c in S.CASES if c.records}
    assert any(c.pad for c in S.CASES if c.path == "rows") and all(
        any(c.pad for c in S.CASES if c.path == p) for p in ("spectra", "band", "windows"))


@pytest.mark.parametrize("name", S.names())
def test_case_crosses_its_seams(name):
    c = S.by_name(name)
    chunk = S.chunk_rows(c)
    seams = S.seams(c)
    assert c.rows > chunk, "%s: %d rows are one chunk of %d" % (name, c.rows, chunk)
    assert len(seams) >= c.min_seams, "%s: %d rows in chunks of %d cross %d seams, written for %d" % (
        name, c.rows, chunk, len(seams), c.min_seams)
    assert all(s < c.rows - 1 for s in seams), (name, seams)
    assert seams[0] == chunk - 1                           # a full first chunk ...
    assert (c.rows - 1 - seams[-1]) <= chunk               # ... and a last one that is short or full, never empty
    assert 1 <= c.hop <= 4096 and S.samples(c) <= 2200000
    # the shards tile the rows, none is empty, and no cut lies on a seam
    sh = S.shards(c)
    assert sh[0][0] == 0 and all(n >= 1 for _, n in sh) and sh[-1][0] + sh[-1][1] == c.rows
    assert all(sh[i][0] + sh[i][1] == sh[i + 1][0] for i in range(2))
    assert not {first - 1 for first, _ in sh[1:]} & set(seams)
    assert sh[1][1] > sh[0][1] and sh[1][1] > sh[2][1]     # small, large, small
    assert set(S.oracle_rows(c)) >= {c.rows - 1} | {r for s in seams for r in (s, s + 1)}


@pytest.mark.parametrize("name", S.names())
def test_case_is_a_call_the_abi_accepts(ro, name):
    c = S.by_name(name)
    lib = ro.library()
    assert ro.bins_supported(c.bins)
    assert c.precision in (ro.RO_PRECISION_F32, ro.RO_PRECISION_F64) and (S.F32, S.F64) == (ro.RO_PRECISION_F32, ro.RO_PRECISION_F64)
    assert (S.IQ_F32, S.IQ_I16) == (ro.RO_IQ_F32, ro.RO_IQ_I16)
    assert ro.row_count(S.samples(c), c.bins, S.overlap(c)) == c.rows
    assert ro.row_count(S.samples(c) - 1, c.bins, S.overlap(c)) == c.rows - 1
    assert ro.clamp_overlap(c.bins, S.overlap(c)) == S.overlap(c)
    if c.family == "czt":
        assert c.bins & (c.bins - 1) and c.precision == S.F32
    else:
        assert c.bins & (c.bins - 1) == 0
    if c.family == "band":
        assert lib.ro_stft_band_supported_precision(c.bins, S.cols(c), c.precision) == 1
        assert ro.band_windows_supported(c.bins, c.windows, c.precision)
        assert (len(c.windows) == 1) == (c.path == "band")
        m, a, slabs = S.band_plan(c.bins, S.cols(c), c.precision)
        assert m >= S.cols(c) and m * a * slabs == c.bins
    if c.records:
        b = ro.Bands(*S.BANDS[name])
        sets = [b] + [ro.Bands(*e) for e in S.EXTRA.get(name, ())]
        if c.family == "band":
            # every set's noise band and its detect band with the average's margin inside one of the case's windows
            for got in (ro.bands_windows(s_, c.bins) for s_ in sets):
                for w in got:
                    assert any(f <= w.first_col and w.first_col + w.cols <= f + n for f, n in c.windows), (name, w)
        else:
            ro.bands_hull(b, c.bins, *S.TILES[name])       # raises when what the recorders read leaves the row


def test_the_table_follows_the_header(tmp_path):
    """the FP64 cases no longer cross their two seams when RO_F64_SCRATCH_MB doubles: the functions read the header"""
    text = open(S.HOST_HEADER).read()
    now = S.scratch_mib("RO_F64_SCRATCH_MB")
    doubled = text.replace("#define RO_F64_SCRATCH_MB %d" % now, "#define RO_F64_SCRATCH_MB %d" % (2 * now))
    assert doubled != text
    copy = os.path.join(str(tmp_path), "ro_host.h")
    with open(copy, "w") as f:
        f.write(doubled)
    assert S.scratch_mib("RO_F64_SCRATCH_MB", copy) == 2 * now
    for c in S.CASES:
        if c.family == "f64":
            assert S.chunk_rows(c, copy) == 2 * S.chunk_rows(c)
            assert len(S.seams(c, copy)) < c.min_seams
        else:
            assert S.chunk_rows(c, copy) == S.chunk_rows(c)
