#!/usr/bin/env python3
"""Index algebra of the FP64 band-only transform (csrc/ro_band_f64.hip) emulated on the CPU in complex128 and checked
against numpy's FFT BEFORE anything runs on a GPU.  The decomposition is ro_band.h's (emu_band.py restates the float32
kernel); what differs here is the plan and the LDS image:

  plan            M the smallest of {256, 512, 1024} >= cols, A M = 4096 double2 cells = 64 KiB: A = 16, 8, 4;
                  slabs = bins / 4096; T = 512 threads, 8 cells per thread
  slab -> a       workgroup `slab` of a row owns a = slab A + t, t < A
  LDS cell        sample a + L b is LOGICAL cell c = b A + t and sits at physical cell phys(c): the 16-cell (256-byte)
                  bank row is c's low four bits; A = 16: phys = c; A = 8: bit 3 of c (= b0) ^= b2 ^ b7;
                  A = 4: bits 3:2 of c (= b1 b0) ^= (b2 ^ b9, b2 ^ b3 ^ b8)
  the levels      radix 4 in place, decimation in frequency, spans M, M/4, ..., then radix 2 if M = 512; work item
                  w = tid + T i -> (t = w mod A, u = w div A), butterfly u of span S at base (u div Q) S + u mod Q
  residue -> cell result r of a transform ends in logical cell band_pos(r) A + t
  tables          tw[q j M / S], t1[j A + t] = W_N^(t k mod N), t2[slab cols + j] = W_N^(slab A k mod N)
  partial sums    A lanes per column folded by the xor tree A/2, ..., 1; the slabs added in slab order

Bank conflicts are counted the way the hardware serves a 16-byte LDS read (ds_read_b128): a wave's 64 lanes in four
groups of 16, {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32; a group takes as many LDS cycles as the largest
number of DISTINCT cells that share a 16-byte slot (cell mod 16) -- 1 is conflict-free.  Reported per shape: the worst
count over every read of every level, "load" (the stores of the samples, 8 lanes x 16 bytes over 32 banks) excluded,
then the gather of the wanted columns; and the same for the unswizzled image, to show what the swizzle buys.
"""
import sys

import numpy as np

SHAPES = ((131072, 256), (131072, 300), (131072, 1024), (524288, 218), (1048576, 1024))
T = 512
CELLS = 4096
B128_GROUPS = [np.array(g) for g in (
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)))]


def plan(bins, cols):
    assert 131072 <= bins <= 1048576 and bins & (bins - 1) == 0 and 1 <= cols <= 1024
    m = 256 if cols <= 256 else 512 if cols <= 512 else 1024
    a = CELLS // m
    return m, a, bins // CELLS


def phys(a, c, swizzle=True):
    """physical cell of logical cell c = b a + t"""
    c = np.asarray(c)
    if not swizzle or a == 16:
        return c
    if a == 8:
        b = c >> 3
        return c ^ (((b >> 2 ^ b >> 7) & 1) << 3)
    b = c >> 2
    x = ((b >> 2 ^ b >> 3 ^ b >> 8) & 1) | (((b >> 2 ^ b >> 9) & 1) << 1)
    return c ^ (x << 2)


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


def read_conflict(cells):
    """worst LDS cycles per 16-lane group of a 16-byte read by work items 0 .. T-1 (cells[tid])"""
    worst = 0
    for wave in range(0, T, 64):
        for g in B128_GROUPS:
            c = np.unique(cells[wave + g])                  # identical addresses broadcast
            worst = max(worst, int(np.bincount(c % 16, minlength=16).max()))
    return worst


def write_conflict(cells):
    """the same for a 16-byte store: eight groups of eight consecutive lanes, 32 banks = 8 slots"""
    worst = 0
    for l0 in range(0, T, 8):
        c = np.unique(cells[l0:l0 + 8])
        worst = max(worst, int(np.bincount(c % 8, minlength=8).max()))
    return worst


def transforms(y, bins, m, a, slabs, conf):
    """the LDS images (physical order) of every slab after the levels: [slabs][4096]; conf[swz] collects
    (level name, read cycles, write cycles) for the swizzled (True) and the plain (False) image"""
    L = bins // m
    tid = np.arange(T)
    tw = root(np.arange(m), m)
    cell = np.full((slabs, CELLS), np.nan + 0j)

    def note(name, reads, writes):
        for swz in (True, False):
            conf[swz].append((name, max(read_conflict(phys(a, c, swz)) for c in reads) if reads else 1,
                              max(write_conflict(phys(a, c, swz)) for c in writes)))

    # ---- loads: work item w IS the logical cell
    seen = np.zeros(CELLS, dtype=int)
    for i in range(CELLS // T):
        w = tid + T * i
        assert w.max() < CELLS
        n = (np.arange(slabs) * a)[:, None] + (w % a)[None, :] + L * (w // a)[None, :]
        assert n.min() >= 0 and n.max() < bins
        p = phys(a, w)
        assert p.min() >= 0 and p.max() < CELLS
        cell[:, p] = y[n]
        seen[p] += 1
        note("load", [], [w])
    assert (seen == 1).all(), "phys() must be a permutation of the cells"
    # ---- levels
    s = m
    while s >= 4:
        q = s // 4
        written = np.zeros(CELLS, dtype=int)
        nxt = cell.copy()
        for i in range(CELLS // 4 // T):
            w = tid + T * i
            t, u = w % a, w // a
            assert u.max() < m // 4
            j = u % q
            base = (u // q) * s + j
            logical = [(base + p * q) * a + t for p in range(4)]
            assert max(ix.max() for ix in logical) < CELLS
            note("S%d" % s, logical, logical)
            idx = [phys(a, ix) for ix in logical]
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
        written = np.zeros(CELLS, dtype=int)
        for i in range(CELLS // 2 // T):
            w = tid + T * i
            t, u = w % a, w // a
            l0 = 2 * u * a + t
            assert (l0 + a).max() < CELLS
            note("S2", [l0, l0 + a], [l0, l0 + a])
            i0, i1 = phys(a, l0), phys(a, l0 + a)
            x0, x1 = cell[:, i0], cell[:, i1]
            nxt[:, i0], nxt[:, i1] = x0 + x1, x0 - x1
            written[i0] += 1
            written[i1] += 1
        assert (written == 1).all()
        cell = nxt
    return cell


def band(cell, bins, m, a, slabs, first_col, cols, conf):
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
        logical = band_pos(m, k & (m - 1)) * a + t
        assert logical.min() >= 0 and logical.max() < CELLS and (jj * a + t).max() < t1.size
        for swz in (True, False):
            conf[swz].append(("gather", read_conflict(phys(a, logical, swz)), 1))
        p = cell[:, phys(a, logical)] * t1[jj * a + t][None, :]
        mm = a // 2
        while mm >= 1:                                  # the xor tree: partner lane tid ^ mm is in the same column group
            assert ((tid ^ mm) // a == g).all() and ((tid ^ mm) // 64 == tid // 64).all()
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


def worst_by_level(conf):
    out = {}
    for name, r, w in conf:
        pr, pw = out.get(name, (1, 1))
        out[name] = (max(pr, r), max(pw, w))
    return out


def fmt_levels(by):
    return " ".join("%s:%d/%d" % (name, r, w) for name, (r, w) in by.items())


def run(bins, cols, seed):
    m, a, slabs = plan(bins, cols)
    assert m * a * slabs == bins and m * a == CELLS
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(bins) + 1j * rng.standard_normal(bins)) * rng.random(bins)
    want = np.roll(np.abs(np.fft.fft(y)), bins // 2)
    conf = {True: [], False: []}
    cell = transforms(y, bins, m, a, slabs, conf)
    worst = 0.0
    for first_col in (bins // 2 - cols // 3, 0, bins - cols):      # straddling N/2, starting at 0, ending at N
        got = band(cell, bins, m, a, slabs, first_col, cols, conf)
        err = np.abs(got - want[first_col:first_col + cols]).max() / want.max()
        assert err < 1e-12, (bins, cols, first_col, err)
        worst = max(worst, err)
    swz, plain = worst_by_level(conf[True]), worst_by_level(conf[False])
    levels = max(r for name, (r, w) in swz.items() if name not in ("load", "gather"))
    print("bins %7d  cols %4d  M %4d  A %2d  slabs %3d: max err / row max %.2e, worst LDS conflict per level %d"
          " (read/write cycles per group, %s; unswizzled %s)"
          % (bins, cols, m, a, slabs, worst, levels, fmt_levels(swz), fmt_levels(plain)))


def main():
    for bins, cols in SHAPES:
        run(bins, cols, seed=bins + cols)
    print("all f64 band maps ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
