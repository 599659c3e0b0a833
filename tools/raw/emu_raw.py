#!/usr/bin/env python3
"""The raw I/Q capture of include/ro_stft.h (ro_raw_host, ro_stft_raw_resident) restated in numpy, twice:

  raw        the rules candidate by candidate, literally: the candidates are the pending list followed by the snapshot
             directory's CAPTURED entries; still pending / EMPTY / LOST / capturable in that order; `offset` the exclusive
             prefix sum of the capturable sizes, fitting or not; CAPTURED where offset + 2 L <= arena_floats; a sample comes
             from the last span that holds it
  raw_plan   the kernels of csrc/ro_raw.hip: one workgroup walks the candidates TILE at a time and carries the directory
             index, the packed pairs, the packed blocks and the pending index (the sums in 16-bit limbs, as the kernel makes
             them); the pending list is compacted in place; the copy kernel finds each block's entry by binary search in
             the plan's table of first blocks and takes each sample from the span that owns it
Neither looks at the library.  tests/test_raw_cpu.py holds ro_raw_host to `raw`; main() holds the two against each other
on random cases with a tile of a few candidates and a block of a few pairs, so that most cases cross their seams.

Run it: python tools/raw/emu_raw.py [cases]     (exit status 0 and a line "ok ..." when everything agrees)
"""
import sys

import numpy as np

EVENT_DTYPE = np.dtype([("fire_row", np.int64), ("start_row", np.int64), ("length", np.int64), ("noise", np.float32),
                        ("peak", np.int32), ("magnitude", np.float32), ("reserved", np.int32)])
SNAPSHOT_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_row", np.int64), ("offset", np.int64), ("rows", np.int32),
                           ("slot", np.int32), ("status", np.int32), ("reserved", np.int32)])
SNAP_SUMMARY_DTYPE = np.dtype([("resolved", np.int64), ("captured", np.int64), ("empty", np.int64), ("lost", np.int64),
                               ("pending", np.int64), ("pending_dropped", np.int64), ("unlisted", np.int64),
                               ("arena_floats", np.int64)])
RAW_CAPTURE_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_sample", np.int64), ("samples", np.int64), ("offset", np.int64),
                              ("slot", np.int32), ("status", np.int32)])
RAW_SUMMARY_DTYPE = np.dtype([("resolved", np.int64), ("captured", np.int64), ("empty", np.int64), ("lost", np.int64),
                              ("pending", np.int64), ("pending_dropped", np.int64), ("arena_floats", np.int64),
                              ("reserved", np.int64)])
CAPTURED, EMPTY, LOST = 0, 1, 2
PENDING, CAPTURABLE = -1, -2                             # (not statuses: what a candidate is before the arena is asked)
F32, I16, F64 = 0, 1, 2
SAMPLE_DTYPE = {F32: np.float32, I16: np.int16, F64: np.float64}
SHADOW = 7777                                            # what a span holds where a later span owns the sample


def clamp_overlap(bins, overlap):
    return 0 if overlap < 0 else (bins - 1 if overlap >= bins else overlap)


def int_rate(bins, overlap, sample_rate):
    """(int)fft_sample_rate: a float32 quotient, truncated"""
    return int(np.float32(sample_rate) / np.float32(bins - clamp_overlap(bins, overlap)))


def raw_length(length, rate_r, sample_rate):
    """fftSamplesToRaw of the recorder: one division, one multiplication in double, truncated toward zero"""
    return int((float(length) / float(rate_r)) * float(sample_rate))


def first_sample(start, bins, overlap):
    hop = bins - clamp_overlap(bins, overlap)
    z = 1 if clamp_overlap(bins, overlap) == 0 else 0
    return (start - z) * hop + 1 if start >= 1 else 0


def samples_of(first, count, fmt):
    """stream samples [first, first + count) in a wire format, [count, 2]: sample s is (s, -s - 0.5), as int16
    (s % 30011 - 15000, -(s % 29989)), so that a wrong sample names itself"""
    s = np.arange(first, first + count, dtype=np.int64)
    if fmt == I16:
        return np.stack([s % 30011 - 15000, -(s % 29989)], axis=1).astype(np.int16)
    return np.stack([s.astype(np.float64), -s.astype(np.float64) - 0.5], axis=1).astype(SAMPLE_DTYPE[fmt])


def spans_of(layout, shadow=True):
    """[(first_sample, samples, format), ...] -> [(array, first_sample, format), ...]; where a later span owns a sample, the
    earlier ones hold SHADOW instead: whoever reads the wrong span names itself"""
    out = []
    for i, (first, count, fmt) in enumerate(layout):
        a = samples_of(first, count, fmt)
        if shadow and i + 1 < len(layout) and layout[i + 1][0] < first + count:
            a[layout[i + 1][0] - first:] = SHADOW
        out.append((a, first, fmt))
    return out


def as_float_pairs(array, fmt):
    """samples in a wire format as the float32 pairs the reference stores: F32 bit for bit, the others (float) of each"""
    if fmt == F32:
        return array.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return array.astype(np.float32)


def run_of(spans, floats, f, L):
    """the float32 pairs of stream samples [f, f + L), each from the LAST span that holds it"""
    s = np.arange(f, f + L, dtype=np.int64)
    owner = np.full(L, -1, np.int64)
    for i, (a, first, _) in enumerate(spans):
        owner[(s >= first) & (s < first + len(a))] = i            # (a later span overrides an earlier one)
    assert (owner >= 0).all(), "no span holds a sample of [%d, %d)" % (f, f + L)
    out = np.zeros((L, 2), np.float32)
    for i, (_, first, _) in enumerate(spans):
        mine = owner == i
        out[mine] = floats[i][s[mine] - first]
    return out.reshape(-1)


def candidates(directory, resolved, pending, pending_count):
    pcap, dcap = pending.shape[0], directory.shape[0]
    have = min(max(int(pending_count[0]), 0), pcap)
    listed = min(max(int(resolved), 0), dcap)
    return [pending[i].copy() for i in range(have)] + [directory[i].copy() for i in range(listed)
                                                       if directory[i]["status"] == CAPTURED]


def classify(c, bins, overlap, sample_rate, base, head):
    """(kind, f, L) of one candidate"""
    start = int(c["event"]["start_row"])
    length = int(c["rows"]) + (int(c["first_row"]) - start)
    L = raw_length(length, int_rate(bins, overlap, sample_rate), sample_rate)
    f = first_sample(start, bins, overlap)
    if f + L > head:
        return PENDING, f, L
    if L <= 0:
        return EMPTY, f, L
    if f < base:
        return LOST, f, L
    return CAPTURABLE, f, L


def entry(c, f, samples, offset, status):
    out = np.zeros(1, RAW_CAPTURE_DTYPE)
    out[0] = (c["event"], f, samples, offset, c["slot"], status)
    return out[0]


def raw(bins, overlap, sample_rate, directory, resolved, spans, pending, pending_count, arena_floats):
    """directory: SNAPSHOT_DTYPE [dir_capacity], `resolved` as the snapshots' summary holds it; spans: [(array [n, 2],
    first_sample, format), ...]; pending [pending_capacity] and pending_count [1] are updated in place.  Returns (raw
    directory, arena, summary): the resolved entries, arena_floats floats (NaN where nothing was written), a
    RAW_SUMMARY_DTYPE scalar."""
    assert int_rate(bins, overlap, sample_rate) != 0
    base, head = spans[0][1], spans[-1][1] + len(spans[-1][0])
    floats = [as_float_pairs(a, fmt) for a, _, fmt in spans]
    out = []
    arena = np.full(arena_floats, np.nan, np.float32)
    sm = np.zeros(1, RAW_SUMMARY_DTYPE)[0]
    offset, still = 0, []
    for c in candidates(directory, resolved, pending, pending_count):
        kind, f, L = classify(c, bins, overlap, sample_rate, base, head)
        if kind == PENDING:
            still.append(c)
        elif kind in (EMPTY, LOST):
            out.append(entry(c, f, 0, 0, kind))
            sm["empty" if kind == EMPTY else "lost"] += 1
        else:
            if offset + 2 * L <= arena_floats:
                arena[offset:offset + 2 * L] = run_of(spans, floats, f, L)
                out.append(entry(c, f, L, offset, CAPTURED))
                sm["captured"] += 1
                sm["arena_floats"] = offset + 2 * L
            else:
                still.append(c)
            offset += 2 * L
    kept = still[:pending.shape[0]]
    for i, c in enumerate(kept):
        pending[i] = c
    pending_count[0] = len(kept)
    sm["pending"] = len(kept)
    sm["pending_dropped"] = len(still) - len(kept)
    sm["resolved"] = len(out)
    d = np.zeros(len(out), RAW_CAPTURE_DTYPE)
    for i, e in enumerate(out):
        d[i] = e
    return d, arena, sm


def limb_cumsum(x):
    """an inclusive sum of 64-bit counts the way the kernel makes it: four ladders of 16 bits each, put together"""
    x = np.asarray(x, np.uint64)
    total = np.zeros(len(x), np.uint64)
    for limb in range(4):
        part = (x >> np.uint64(16 * limb)) & np.uint64(0xffff)
        total += np.cumsum(part).astype(np.uint64) << np.uint64(16 * limb)
    return total.astype(np.int64)


def raw_plan(bins, overlap, sample_rate, directory, resolved, spans, pending, pending_count, arena_floats, tile=256, block=512,
             waves=7):
    """the same outputs the way the kernels get them"""
    base, head = spans[0][1], spans[-1][1] + len(spans[-1][0])
    floats = [as_float_pairs(a, fmt) for a, _, fmt in spans]
    pcap, dcap = pending.shape[0], directory.shape[0]
    have = min(max(int(pending_count[0]), 0), pcap)
    listed = min(max(int(resolved), 0), dcap)
    n = have + listed
    arena_pairs = arena_floats >> 1
    raw_dir = np.zeros(pcap + dcap, RAW_CAPTURE_DTYPE)
    first_block = np.zeros(pcap + dcap, np.int64)
    sm = np.zeros(1, RAW_SUMMARY_DTYPE)[0]
    pair_base = block_base = used_pairs = used_blocks = dir_base = pend_base = 0
    # ---- raw_plan_kernel
    for t0 in range(0, n, tile):
        idx = range(t0, min(t0 + tile, n))
        lanes = [pending[c].copy() if c < have else directory[c - have].copy() for c in idx]      # loaded before any store
        live = [c < have or lanes[i]["status"] == CAPTURED for i, c in enumerate(idx)]
        kinds = [classify(c, bins, overlap, sample_rate, base, head) if live[i] else (None, 0, 0) for i, c in enumerate(lanes)]
        pairs = np.array([L if k == CAPTURABLE else 0 for k, _, L in kinds], np.int64)
        blocks = (pairs + block - 1) // block
        first_p = pair_base + limb_cumsum(pairs) - pairs
        first_b = block_base + limb_cumsum(blocks) - blocks
        capturable = np.array([k == CAPTURABLE for k, _, _ in kinds])
        fits = capturable & (first_p + pairs <= arena_pairs)
        resolved_here = fits | np.array([k in (EMPTY, LOST) for k, _, _ in kinds])
        pend = np.array([k == PENDING for k, _, _ in kinds]) | (capturable & ~fits)
        res_rank = np.cumsum(resolved_here) - resolved_here
        pend_rank = np.cumsum(pend) - pend
        for i, c in enumerate(lanes):
            kind, f, L = kinds[i]
            if resolved_here[i]:
                d = dir_base + int(res_rank[i])
                status = CAPTURED if fits[i] else kind
                raw_dir[d] = entry(c, f, L if fits[i] else 0, 2 * int(first_p[i]) if fits[i] else 0, status)
                first_block[d] = first_b[i]
                sm[("captured", "empty", "lost")[status]] += 1
            if pend[i] and pend_base + int(pend_rank[i]) < pcap:
                assert pend_base + int(pend_rank[i]) <= idx[i]               # in place: at or in front of where it was read
                pending[pend_base + int(pend_rank[i])] = c
        if fits.any():
            last = int(np.flatnonzero(fits)[-1])
            used_pairs = max(used_pairs, int(first_p[last] + pairs[last]))
            used_blocks = max(used_blocks, int(first_b[last] + blocks[last]))
        pair_base += int(pairs.sum())
        block_base += int(blocks.sum())
        dir_base += int(resolved_here.sum())
        pend_base += int(pend.sum())
    kept = min(pend_base, pcap)
    pending_count[0] = kept
    sm["pending"], sm["pending_dropped"] = kept, pend_base - kept
    sm["resolved"], sm["arena_floats"] = dir_base, 2 * used_pairs
    # ---- raw_copy_kernel: wave w takes blocks w, w + waves, ...
    arena = np.full(arena_floats, np.nan, np.float32)
    own_lo = [first for _, first, _ in spans]
    own_hi = own_lo[1:] + [head]
    for w in range(waves):
        for b in range(w, used_blocks, waves):
            lo, hi = 0, dir_base
            while lo < hi:
                mid = (lo + hi) >> 1
                if first_block[mid] <= b:
                    lo = mid + 1
                else:
                    hi = mid
            assert lo > 0
            en = raw_dir[lo - 1]
            p0 = (b - int(first_block[lo - 1])) * block
            L, offset = int(en["samples"]), int(en["offset"])
            assert en["status"] == CAPTURED and p0 < L and offset + 2 * L <= arena_floats, (b, lo - 1, en)
            count = min(block, L - p0)
            s0 = int(en["first_sample"]) + p0
            got = np.zeros((count, 2), np.float32)
            for i in range(len(spans)):
                if s0 + count <= own_lo[i] or s0 >= own_hi[i]:
                    continue
                s = np.arange(s0, s0 + count)
                at = np.clip(s - spans[i][1], 0, len(spans[i][0]) - 1)
                mine = (s >= own_lo[i]) & (s < own_hi[i])
                got[mine] = floats[i][at][mine]
            arena[offset + 2 * p0:offset + 2 * (p0 + count)] = got.reshape(-1)
    return raw_dir[:dir_base].copy(), arena, sm


def random_case(rng):
    """arguments of one call: snapshots around the spans, so that every outcome turns up"""
    bins = int(rng.choice([256, 512]))                   # (sizes a handle takes: the device runs these cases too)
    overlap = int(rng.choice([0, 1, bins // 2, bins - 8, bins - 1]))
    hop = bins - overlap
    sample_rate = int(rng.choice([hop, 2 * hop + 1, 5 * hop, 48 * hop + 7]))
    count = int(rng.integers(1, 5))
    base = int(rng.integers(0, 40 * hop))
    starts = base + np.concatenate([[0], np.sort(rng.choice(np.arange(1, 30 * hop + count), count - 1, replace=False))])
    layout = []
    for i in range(count):
        lowest_end = (int(starts[i + 1]) if i + 1 < count else int(starts[i]) + 1)
        lowest_end = max(lowest_end, layout[-1][0] + layout[-1][1] + 1 if layout else 0)
        end = lowest_end + int(rng.integers(0, 6 * hop))
        layout.append((int(starts[i]), end - int(starts[i]), int(rng.integers(0, 3))))
    spans = spans_of(layout)
    head = layout[-1][0] + layout[-1][1]
    dcap, pcap = int(rng.integers(0, 41)), int(rng.integers(0, 9))

    def some(n, all_captured=False):
        d = np.zeros(n, SNAPSHOT_DTYPE)
        start = rng.integers(base // hop - 6, head // hop + 4, n)
        start = np.where(rng.random(n) < 0.1, rng.integers(-5, 2, n), start)        # some at and below row 0: f = 0
        length = rng.integers(0, 14, n)
        d["event"]["start_row"] = start
        d["event"]["length"] = length + rng.integers(0, 3, n)
        d["event"]["fire_row"] = start + length
        d["event"]["peak"] = rng.integers(0, 400, n)
        d["event"]["noise"] = rng.random(n)
        d["event"]["magnitude"] = rng.random(n)
        d["first_row"] = np.maximum(start, 0)
        d["rows"] = np.maximum(length - (d["first_row"] - start), 0)
        d["offset"] = rng.integers(0, 1000, n)
        d["slot"] = rng.integers(0, 8, n)
        d["status"] = CAPTURED if all_captured else rng.choice([CAPTURED, CAPTURED, CAPTURED, EMPTY, LOST], n)
        return d
    directory = some(dcap)
    resolved = int(rng.integers(-1, dcap + 4))
    pending = some(pcap, all_captured=True)
    pending_count = np.array([rng.integers(-1, pcap + 2)], np.int64)
    L_typ = raw_length(7, int_rate(bins, overlap, sample_rate), sample_rate)
    arena_floats = int(rng.choice([0, 1, 2 * L_typ, 9 * L_typ + 3, 200 * L_typ]))
    return dict(bins=bins, overlap=overlap, sample_rate=sample_rate, directory=directory, resolved=resolved, spans=spans,
                pending=pending, pending_count=pending_count, arena_floats=arena_floats)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main(cases=200):
    rng = np.random.default_rng(21)
    seen = np.zeros(5, np.int64)
    for case in range(cases):
        args = random_case(rng)
        a = dict(args, pending=args["pending"].copy(), pending_count=args["pending_count"].copy())
        b = dict(args, pending=args["pending"].copy(), pending_count=args["pending_count"].copy())
        d1, arena1, s1 = raw(**a)
        d2, arena2, s2 = raw_plan(tile=int(rng.choice([3, 5, 64])), block=int(rng.choice([1, 7, 64])),
                                  waves=int(rng.choice([1, 7])), **b)
        kept = int(a["pending_count"][0])
        ok = (same(d1, d2) and same(arena1, arena2) and s1 == s2 and same(a["pending_count"], b["pending_count"]) and
              same(a["pending"][:kept], b["pending"][:kept]) and same(a["pending"][kept:], args["pending"][kept:]) and
              same(b["pending"][kept:], args["pending"][kept:]))
        if not ok:
            print("case %d: the plan and the rules disagree\n%s\n%s\n%s\n%s" % (case, s1, s2, d1, d2))
            return 1
        seen += (int(s1["captured"]), int(s1["empty"]), int(s1["lost"]), int(s1["pending"]), int(s1["pending_dropped"]))
    if not seen.all():
        print("the cases leave an outcome out: captured, empty, lost, pending, dropped = %s" % seen.tolist())
        return 1
    print("ok: %d cases; captured %d, empty %d, lost %d, pending %d, dropped %d" % ((cases,) + tuple(seen.tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 200))
