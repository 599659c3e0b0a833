#!/usr/bin/env python3
"""The window-list gather of the band-only transform (ro_stft_band_windows_resident; csrc/ro_band_windows.hip and
csrc/ro_band_windows_f64.hip) emulated on the CPU in complex128 and checked against numpy's FFT BEFORE anything runs on a GPU.

The loads and the levels are emu_band.py's and emu_band_f64.py's (imported: the window-list kernels keep those index
maps).  What is walked here is their gather:

  image column    window w = [first_col_w, +cols_w) occupies image columns [off_w, off_w + cols_w), off_w the sum of the
                  earlier windows' cols; image column j shows bin k(j) = (its row column + N/2) mod N
  kcell[j]        band_pos(k(j) mod M) A: the logical LDS cell of residue t = 0 (host table, one int32 per image column);
                  the kernel reads cell kcell[j] + t (float32) or phys(kcell[j] + t) (FP64)
  tables          t1[j A + t] = W_N^(t k(j) mod N), t2[slab cols + j] = W_N^(slab A k(j) mod N)
  partial sums    A lanes per column folded by the xor tree A/2, ..., 1; the slabs added in slab order

Nothing in X[k] = sum_a W_N^(a k) Z_a[k mod M] needs the k(j) consecutive or their residues mod M distinct: two image
columns of one residue read the same cell.  The cases marked "colliding" are such lists.

For the FP64 image the worst LDS cycles per 16-lane group of the gather's 16-byte read are printed (emu_band_f64.py's
rule: distinct cells on one 16-byte slot; reads of the same cell are one broadcast), lane groups that straddle two
windows included, next to the figure of one consecutive band of the same width.  Recorded, not gated.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_band as f32            # noqa: E402
import emu_band_f64 as f64        # noqa: E402

# (bins, windows, note)
F32_CASES = (
    (16384, ((3000, 300), (9000, 400)), "M = 1024"),
    (16384, ((1000, 100), (1000 + 5 * 256, 100)), "colliding residues"),
    (16384, ((0, 200), (8100, 200), (16284, 100)), "row edges, across N/2"),
    (16384, tuple((700 + 1900 * i, 100 + 7 * i) for i in range(8)), "eight windows"),
    (32768, ((22528, 409), (23278, 615)), "radio-observer.json"),
)
F64_CASES = (
    (131072, ((1000, 100), (1000 + 5 * 256, 100)), "colliding residues"),
    (131072, ((5000, 150), (70000, 203)), "M = 512"),
    (131072, ((0, 409), (65300, 515), (130972, 100)), "row edges, across N/2"),
    (131072, tuple((900 + 15000 * i, 21 + 13 * i) for i in range(8)), "eight windows"),
    (131072, ((40000, 37), (40000 + 3 * 1024 + 19, 900)), "colliding residues at M = 1024"),
)


def columns(windows):
    """row column of every image column, in image order"""
    return np.concatenate([np.arange(first, first + n) for first, n in windows])


def check_windows(bins, windows):
    assert 1 <= len(windows) <= 8
    end = 0
    for first, n in windows:
        assert n >= 1 and first >= end and first + n <= bins, windows
        end = first + n
    assert sum(n for _, n in windows) <= 1024


def gather(cell, bins, m, a, slabs, windows, threads, phys, conflicts):
    """the band image row (magnitudes) from the slabs' LDS images; conflicts (a list or None) collects the LDS cycles of
    every step's read"""
    cols_of = columns(windows)
    cols = cols_of.size
    k_all = (cols_of + bins // 2) % bins
    kcell = f32.band_pos(m, k_all % m) * a                                                      # the host's table
    assert kcell.min() >= 0 and kcell.max() + a <= m * a
    t1 = f32.root((np.arange(a)[None, :] * k_all[:, None]) % bins, bins).reshape(-1)               # [cols][a]
    t2 = f32.root(((np.arange(slabs) * a)[:, None] * k_all[None, :]) % bins, bins).reshape(-1)     # [slabs][cols]
    part = np.full((slabs, cols), np.nan + 0j)
    tid = np.arange(threads)
    t, g = tid % a, tid // a
    step = threads // a
    for j0 in range(0, cols, step):
        j = j0 + g
        live = j < cols
        jj = np.where(live, j, cols - 1)
        logical = kcell[jj] + t
        assert logical.min() >= 0 and logical.max() < m * a and (jj * a + t).max() < t1.size
        if conflicts is not None:
            conflicts.append(f64.read_conflict(phys(logical)))
        p = cell[:, phys(logical)] * t1[jj * a + t][None, :]
        mm = a // 2
        while mm >= 1:
            assert ((tid ^ mm) // a == g).all() and ((tid ^ mm) // 64 == tid // 64).all()
            p = p + p[:, tid ^ mm]
            mm //= 2
        sel = live & (t == 0)
        sl = np.arange(slabs)[:, None]
        assert (sl * cols + j[sel][None, :]).max() < t2.size
        part[:, j[sel]] = p[:, sel] * t2[sl * cols + j[sel][None, :]]
    assert not np.isnan(part).any()
    acc = np.zeros(cols, dtype=np.complex128)
    for s in range(slabs):
        acc = acc + part[s]
    return np.abs(acc)


def signal(bins, seed):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(bins) + 1j * rng.standard_normal(bins)) * rng.random(bins)
    return y, np.roll(np.abs(np.fft.fft(y)), bins // 2)


def describe(windows):
    return " ".join("[%d,+%d)" % w for w in windows)


def shared_residues(bins, m, windows):
    k = (columns(windows) + bins // 2) % bins
    return k.size - np.unique(k % m).size


def run_f32(bins, windows, note):
    check_windows(bins, windows)
    total = sum(n for _, n in windows)
    m, a, slabs = f32.plan(bins, total)
    y, want = signal(bins, bins + total)
    cell = f32.transforms(y, bins, m, a, slabs)
    got = gather(cell, bins, m, a, slabs, windows, a * m // 16, lambda c: c, None)
    err = np.abs(got - want[columns(windows)]).max() / want.max()
    print("f32  bins %7d  M %4d  A %2d  slabs %3d  %d windows, %4d columns, %3d share a residue (%s): "
          "max err / row max %.2e   %s" % (bins, m, a, slabs, len(windows), total, shared_residues(bins, m, windows), note,
                                          err, describe(windows)))
    return err


def run_f64(bins, windows, note):
    check_windows(bins, windows)
    total = sum(n for _, n in windows)
    m, a, slabs = f64.plan(bins, total)
    y, want = signal(bins, bins + total + 1)
    cell = f64.transforms(y, bins, m, a, slabs, {True: [], False: []})
    conflicts, one_band = [], []
    got = gather(cell, bins, m, a, slabs, windows, f64.T, lambda c: f64.phys(a, c), conflicts)
    err = np.abs(got - want[columns(windows)]).max() / want.max()
    gather(cell, bins, m, a, slabs, ((windows[0][0], total),), f64.T, lambda c: f64.phys(a, c), one_band)
    print("f64  bins %7d  M %4d  A %2d  slabs %3d  %d windows, %4d columns, %3d share a residue (%s): "
          "max err / row max %.2e, gather worst LDS cycles per 16-lane group %d (one band of %d columns: %d)   %s"
          % (bins, m, a, slabs, len(windows), total, shared_residues(bins, m, windows), note, err, max(conflicts), total,
             max(one_band), describe(windows)))
    return err


def main():
    worst = 0.0
    for case in F32_CASES:
        worst = max(worst, run_f32(*case))
    for case in F64_CASES:
        worst = max(worst, run_f64(*case))
    if not worst < 1e-12:
        print("FAILED: max err / row max %.2e" % worst)
        return 1
    print("all band window maps ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
