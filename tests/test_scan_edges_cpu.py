"""The references and case tables of tests/scan_edges.py, checked against each other before either judges a kernel
(tests/test_gpu_scan_edges.py).  No GPU.  Everything is bit-exact."""
import numpy as np
import pytest

import scan_edges as se


def oracle_tone_rows(oracle, bins, overlap, tones):
    key = ("rows", bins, overlap, tuple(tones))
    if key not in se._rows_cache:
        se._rows_cache[key] = oracle.stft(se.tone_signal(bins, overlap, tones), bins, overlap)
    return se._rows_cache[key]


def agree(oracle, name, rows, bands, sortable=True):
    bins = rows.shape[1]
    ref = se.scan_reference(rows, bands, bins)
    if not sortable:
        return ref
    padded = se.oracle_padded(oracle, rows, bands)
    assert se.same_bits(ref, padded), (name, se.describe(ref, padded))
    if se.window_inside(bands, bins):
        plain = se.oracle_plain(oracle, rows, bands)
        assert se.same_bits(ref, plain), (name, se.describe(ref, plain))
    return ref


def test_references_agree_where_the_window_leaves_the_row(oracle):
    clipped = 0
    for name, rows, bands in se.hbm_window_cases():
        ref = agree(oracle, name, rows, bands)
        leaves = se.window_leaves(rows, bands, rows.shape[1])
        clipped += int(leaves.sum())
        if rows.shape[1] == se.A_SMALL_BINS and bands[3] == 256:
            assert list(ref["peak"]) == [0, 1, 127, 254, 255, 255]            # equal maxima: the last one wins
    assert clipped > 60
    # every one of the 256-bin cases has a clipped row on each side except avg_bins = 1, and the 16384-bin rows do
    for name, rows, bands in se.hbm_window_cases():
        start = bands[2] + se.scan_reference(rows, bands, rows.shape[1])["peak"].astype(int) - bands[4] // 2
        if bands[4] > 2:
            assert (start < 0).any() or (start + bands[4] > rows.shape[1]).any(), name


def test_references_agree_on_float32_edge_values(oracle):
    for name, fx, rows, bands in se.float_edge_cases():
        assert se.window_inside(bands, se.B_BINS)
        ref = agree(oracle, name, rows, bands, sortable=fx in se.B_ORACLE_SORTS)
        band = rows[:, bands[2]:bands[2] + bands[3]]
        if fx == "inf":
            for r in range(se.B_ROWS):
                assert ref["peak"][r] == np.flatnonzero(np.isposinf(band[r])).max()
            assert np.isposinf(ref["average"]).all() and np.isfinite(ref["noise"]).all()
        if fx == "flt_max":
            assert np.isposinf(ref["noise"]).all() and np.isfinite(ref["average"]).all()
            assert (band[np.arange(se.B_ROWS), ref["peak"]] == se.FLT_MAX).all()
        if fx == "denormal":
            assert (ref["noise"] > 0).all() and (ref["average"] > 0).all()


@pytest.mark.parametrize("bins,overlap", se.C_SHAPES)
def test_references_agree_on_the_transform_cases(oracle, bins, overlap):
    """on the oracle's rows of the same signals; the tones are where the table says and are their bands' maxima"""
    clipped = 0
    for name, bands, tones in se.epilogue_cases(bins):
        rows = oracle_tone_rows(oracle, bins, overlap, tones)
        assert rows.shape == (se.C_ROWS, bins)
        ref = agree(oracle, name, rows, bands)
        assert se.peaks_on_tones(rows, bands, tones), (name, ref["peak"])
        clipped += int(se.window_leaves(rows, bands, bins).all())
    assert clipped == 4                                   # left, right, and the whole row twice


def test_clipped_cases_tell_a_wrapped_window_from_a_clipped_one(oracle):
    """scan_reference with the guard replaced by wrapping disagrees with oracle_padded on every row whose window leaves
    the row, and agrees on the others: the cases can tell the two behaviours apart"""
    todo = [(name, rows, bands) for name, rows, bands in se.hbm_window_cases()]
    for bins, overlap in se.C_SHAPES:
        todo += [(name, oracle_tone_rows(oracle, bins, overlap, tones), bands)
                 for name, bands, tones in se.epilogue_cases(bins)]
    told = 0
    for name, rows, bands in todo:
        bins = rows.shape[1]
        leaves = se.window_leaves(rows, bands, bins)
        wrapped = se.scan_reference(rows, bands, bins, wrap=True)
        padded = se.oracle_padded(oracle, rows, bands)
        differs = wrapped["average"].view(np.uint32) != padded["average"].view(np.uint32)
        assert np.array_equal(differs, leaves), (name, differs, leaves)
        told += int(leaves.sum())
    assert told > 100


def test_tables_contain_the_limits_they_claim():
    a = se.hbm_window_cases()
    widths_a = {b[1] for _, _, b in a} | {b[3] for _, _, b in a}
    assert {1024, 1025, 4096, 4097, 8192, 8193, 16384, 256, 1} <= widths_a
    assert {b[4] for _, _, b in a} >= {1, 2, 3, 27, 64, 65, 129, 255, 101}
    assert {(b[2], b[3]) for _, _, b in a} >= {(0, 256), (0, 1), (255, 1)}
    assert {b[3] for _, _, _, b in se.float_edge_cases()} == {5, 64, 409, 1024, 1025, 4097}
    assert {fx for _, fx, _, _ in se.float_edge_cases()} == set(se.B_FIXTURES)
    N = 32768
    c = se.epilogue_cases(N)
    noise_w = {b[1] for _, b, _ in c}
    detect_w = {b[3] for _, b, _ in c}
    assert {1, 2, 3, 4, 5, 511, 512, 513, 1024, 1025, 32768} <= noise_w
    assert {1, 63, 64, 65, 511, 512, 513, 1025, 32768} <= detect_w
    assert {64, 65, 129, 1, 2, 27, 63} <= {b[4] for _, b, _ in c}

    def holds(low, width, col):
        return low <= col < low + width

    for n in (N, 4096):
        c = se.epilogue_cases(n)
        assert any(holds(b[0], b[1], n // 2 - 1) and holds(b[0], b[1], n // 2) and b[1] < n for _, b, _ in c)
        assert any(holds(b[2], b[3], n // 2 - 1) and holds(b[2], b[3], n // 2) and b[3] == 2 for _, b, _ in c)
        assert any(b[0] == 0 and b[1] == 409 for _, b, _ in c) and any(b[0] + b[1] == n and b[1] == 409 for _, b, _ in c)
        assert any(b[2] == 0 and b[3] == 410 for _, b, _ in c) and any(b[2] + b[3] == n and b[3] == 410 for _, b, _ in c)
        assert all(0 <= b[0] and b[0] + b[1] <= n and 0 <= b[2] and b[2] + b[3] <= n for _, b, _ in c)
    assert se.json_like(N) == (22528, 409, 23415, 410, 27)
    assert (16384 - 100, 200) in se.D_TILES and (0, 32768) in se.D_TILES and (0, 1) in se.D_TILES and (32767, 1) in se.D_TILES
    assert {t[1] for t in se.D_TILES} >= {1, 63, 64, 65, 127, 128, 129, 200, 615, 32768}
    assert all(0 <= f and f + w <= se.D_BINS for f, w in se.D_TILES)


def test_float_fixtures_are_what_they_claim():
    for w in se.B_WIDTHS:
        sl = slice(se.B_LOW, se.B_LOW + w)
        den = se.float_edge_rows("denormal", w)[:, sl]
        u = den.view(np.uint32)
        assert ((u >= 1) & (u <= 0x7fffff)).all()                               # positive, exponent field 0, not zero
        assert all(len(np.unique(u[r])) == w for r in range(se.B_ROWS))        # pairwise distinct
        mixed = se.float_edge_rows("mixed", w)[:, sl]
        assert (mixed != 0).all() and not np.isnan(mixed).any()
        if w >= 64:
            m = mixed.view(np.uint32)
            assert ((m & 0x7f800000) == 0).any() and ((m & 0x7f800000) != 0).any() and (mixed < 0).any() and (mixed > 0).any()
        low = se.float_edge_rows("low_byte", w)[:, sl].view(np.uint32)
        assert ((low & ~np.uint32(0xff)) == 0x3f800000).all()                   # keys differ in bits 0 ... 7 only
        assert all(len(np.unique(low[r])) == min(w, 256) for r in range(se.B_ROWS))
        b8 = se.float_edge_rows("bit8", w)[:, sl].view(np.uint32)
        assert ((b8 & ~np.uint32(0x1ff)) == 0x3f800000).all()                   # nothing differs above bit 8
        assert all((b8[r] & 0x100).any() and not (b8[r] & 0x100).all() for r in range(se.B_ROWS))   # ... and bit 8 does
        for fx in se.B_FIXTURES:
            rows = se.float_edge_rows(fx, w)
            assert not np.isnan(rows).any() and not (np.signbit(rows) & (rows == 0)).any()         # no NaN, no -0.0
