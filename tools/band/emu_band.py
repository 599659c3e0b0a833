#!/usr/bin/env python3
"""Index algebra of the band-only transform (csrc/ro_band.hip) emulated on the CPU and checked against numpy's FFT
BEFORE anything runs on a GPU.

Columns c in [first_col, first_col + cols) of the fft-shifted row are bins k(c) = (c + N/2) mod N.  With M the smallest of
{256, 512, 1024} >= cols, L = N / M, and the windowed samples indexed n = a + L b:
    Z_a[r] = sum_b y[a + L b] exp(-2 pi i b r / M)
    X[k]   = sum_a exp(-2 pi i a k / N) Z_a[k mod M]
The maps walked here are the kernel's own:
  slab -> a       workgroup `slab` of a row owns a = slab A + t, t < A (A = 16, or 8 at M = 1024)
  LDS cell        sample a + L b sits in cell b A + t; the load's work item w = tid + T i IS that cell
  the levels      radix 4 in place, decimation in frequency, spans M, M/4, ..., then radix 2 if M = 512; work item
                  w -> (t = w mod A, u = w div A), butterfly u of span S at base (u div Q) S + u mod Q, Q = S / 4
  residue -> cell result r of a transform ends in cell band_pos(r) A + t (digit reversal, mixed radix 4 ... 4 [2])
  tables          tw[q j M / S], t1[j A + t] = W_N^(t k mod N), t2[slab cols + j] = W_N^(slab A k mod N)
  partial sums    A lanes per column folded by the xor tree A/2, ..., 1; the slabs added in slab order
"""
import sys

import numpy as np

SHAPES = ((16384, 256), (16384, 1024), (32768, 400), (65536, 600), (524288, 218))       # M = 256, 1024, 512, 1024, 256


def plan(bins, cols):
    assert 16384 <= bins <= 1048576 and bins & (bins - 1) == 0 and 1 <= cols <= 1024
    m = 256 if cols <= 256 else 512 if cols <= 512 else 1024
    a = 8 if m == 1024 else 16
    return m, a, bins // (m * a)


def band_pos(m, r):
    r = np.asarray(r).copy()
    pos = np.zeros_like(r)
    s = m
    while s > 1:
        radix = 4 if s >= 4 else 2
        pos += (r % radix) * (s // radix)
        r //= radix
        s //= radix
    return pos


def root(e, n):
    """exp(-2 pi i e / n) from the exactly reduced integer phase"""
    e = np.asarray(e, dtype=np.int64)
    assert e.min() >= 0 and e.max() < n
    return np.exp(-2j * np.pi * e.astype(np.float64) / n)


def transforms(y, bins, m, a, slabs):
    """the LDS images of every slab after the levels: [slabs][m * a]"""
    L = bins // m
    T = a * m // 16
    tid = np.arange(T)
    tw = root(np.arange(m), m)
    cell = np.full((slabs, m * a), np.nan + 0j)
    # ---- loads
    for i in range(16):
        w = tid + T * i
        assert w.max() < a * m
        n = (np.arange(slabs) * a)[:, None] + (w % a)[None, :] + L * (w // a)[None, :]
        assert n.max() < bins
        cell[:, w] = y[n]
    assert not np.isnan(cell).any()
    # ---- levels
    s = m
    while s >= 4:
        q = s // 4
        written = np.zeros(m * a, dtype=int)
        nxt = cell.copy()
        for i in range(4):
            w = tid + T * i
            t, u = w % a, w // a
            assert u.max() < m // 4
            j = u % q
            base = (u // q) * s + j
            idx = [(base + p * q) * a + t for p in range(4)]
            assert max(ix.max() for ix in idx) < m * a
            x0, x1, x2, x3 = (cell[:, ix] for ix in idx)
            s02, d02, s13, d13 = x0 + x2, x0 - x2, x1 + x3, x1 - x3
            md = -1j * d13
            ys = [s02 + s13, d02 + md, s02 - s13, d02 - md]
            if q > 1:
                step = m // s
                for p in (1, 2, 3):
                    assert (p * j * step).max() < m
                    ys[p] = ys[p] * tw[p * j * step][None, :]
            for p in range(4):
                nxt[:, idx[p]] = ys[p]
                written[idx[p]] += 1
        assert (written == 1).all(), "a level must touch every cell exactly once"
        cell = nxt
        s //= 4
    if s == 2:
        nxt = cell.copy()
        written = np.zeros(m * a, dtype=int)
        for i in range(8):
            w = tid + T * i
            t, u = w % a, w // a
            i0 = 2 * u * a + t
            assert (i0 + a).max() < m * a
            x0, x1 = cell[:, i0], cell[:, i0 + a]
            nxt[:, i0], nxt[:, i0 + a] = x0 + x1, x0 - x1
            written[i0] += 1
            written[i0 + a] += 1
        assert (written == 1).all()
        cell = nxt
    return cell


def band(cell, bins, m, a, slabs, first_col, cols):
    T = a * m // 16
    j_all = np.arange(cols)
    k_all = (first_col + j_all + bins // 2) % bins
    assert len(np.unique(k_all % m)) == cols, "the band's residues k mod M must be distinct"
    t1 = root((np.arange(a)[None, :] * k_all[:, None]) % bins, bins).reshape(-1)                 # [cols][a]
    t2 = root(((np.arange(slabs) * a)[:, None] * k_all[None, :]) % bins, bins).reshape(-1)       # [slabs][cols]
    part = np.full((slabs, cols), np.nan + 0j)
    tid = np.arange(T)
    t, g = tid % a, tid // a
    for j0 in range(0, cols, T // a):
        j = j0 + g
        live = j < cols
        jj = np.where(live, j, cols - 1)
        k = (first_col + jj + bins // 2) & (bins - 1)
        c = band_pos(m, k & (m - 1)) * a + t
        assert c.max() < m * a and (jj * a + t).max() < t1.size
        p = cell[:, c] * t1[jj * a + t][None, :]
        mm = a // 2
        while mm >= 1:                                  # the xor tree: partner lane tid ^ mm is in the same column group
            assert ((tid ^ mm) // a == g).all()
            p = p + p[:, tid ^ mm]
            mm //= 2
        sel = live & (t == 0)
        sl = np.arange(slabs)[:, None]
        assert (sl * cols + j[sel][None, :]).max() < t2.size
        part[:, j[sel]] = p[:, sel] * t2[sl * cols + j[sel][None, :]]
    assert not np.isnan(part).any()
    acc = np.zeros(cols, dtype=np.complex128)
    for s in range(slabs):                              # slab order
        acc = acc + part[s]
    return np.abs(acc)


def run(bins, cols, seed):
    m, a, slabs = plan(bins, cols)
    assert m * a * slabs == bins
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(bins) + 1j * rng.standard_normal(bins)) * rng.random(bins)
    want = np.roll(np.abs(np.fft.fft(y)), bins // 2)
    cell = transforms(y, bins, m, a, slabs)
    worst = 0.0
    for first_col in (bins // 2 - cols // 3, 0, bins - cols):      # straddling N/2, starting at 0, ending at N
        got = band(cell, bins, m, a, slabs, first_col, cols)
        err = np.abs(got - want[first_col:first_col + cols]).max() / want.max()
        assert err < 1e-12, (bins, cols, first_col, err)
        worst = max(worst, err)
    print("bins %7d  cols %4d  M %4d  A %2d  slabs %3d: max err / row max %.2e" % (bins, cols, m, a, slabs, worst))


def main():
    for bins, cols in SHAPES:
        run(bins, cols, seed=bins + cols)
    print("all band maps ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
