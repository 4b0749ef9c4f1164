"""Shared by the k-mer index tests (tests/test_index_host.py, tests/test_index_gpu.py, tests/test_index_scale_gpu.py; the block set
also by tests/test_votes_scale_gpu.py): the read sets at which the device build of
hinge_amd/csrc/index_kernels.h can go wrong, and the comparison with the numpy model seed_common.Index (written from the rule:
numpy's stable argsort and bincount where the kernels have a radix sort, a scan and fixed-trip searches).  T = the sort's tile
(hinge_index_tile(); IDX_TILE of index_kernels.h)."""
import re
import os

import numpy as np

import seed_common as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_from_source():
    """IDX_TILE as index_kernels.h states it (the GPU test asks the library instead)."""
    src = open(os.path.join(ROOT, "hinge_amd", "csrc", "index_kernels.h")).read()
    rows = int(re.search(r"constexpr int IDX_ROWS = (\d+);", src).group(1))
    assert re.search(r"constexpr int IDX_TILE = 64 \* IDX_ROWS;", src)
    return 64 * rows


def scan_chunk_from_source():
    """IDX_SCAN_CHUNK (C) as index_kernels.h states it: the elements one wavefront scans; the scan recurses once per factor of C."""
    src = open(os.path.join(ROOT, "hinge_amd", "csrc", "index_kernels.h")).read()
    per_lane = int(re.search(r"constexpr int IDX_SCAN_PER_LANE = (\d+);", src).group(1))
    assert re.search(r"constexpr int IDX_SCAN_CHUNK = 64 \* IDX_SCAN_PER_LANE;", src)
    return 64 * per_lane


def scan_levels(length, C):
    """Launch levels of the scan over `length` elements: 1 up to C, 2 up to C * C, 3 beyond."""
    levels = 1
    while length > C:
        length = -(-length // C)
        levels += 1
    return levels


def block_set(seed=7):
    """About one block's worth of overlapping reads: 1030 reads of 3 000 .. 5 399 bases cut from a random genome of 1 450 000
    bases (about 3x), every second one stored reverse-complemented; about 4.33 M entries, so the scan of its n + 1 flags has three
    levels and read_top of the vote kernels is 1024."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 4, size=1_450_000, dtype=np.uint8)
    lens = rng.integers(3000, 5400, size=1030)
    starts = rng.integers(0, len(G) - 5400, size=1030)
    reads = []
    for i in range(1030):
        r = G[int(starts[i]):int(starts[i]) + int(lens[i])].copy()
        reads.append(sm.revcomp(r) if i % 2 else r)
    return reads


def sized(reads, k, n):
    """The same reads cut at the end so that entries(., k) == n exactly: whole trailing reads dropped, then the last one shortened
    (it keeps at least k bases: at least one entry)."""
    out, have = [], 0
    for r in reads:
        e = max(len(r) - k + 1, 0)
        if have + e >= n and e > 0:
            out.append(r[:n - have + k - 1].copy())
            have = n
            break
        out.append(r)
        have += e
    assert have == n and entries(out, k) == n and len(out[-1]) >= k, (have, n)
    return out


def sorted_codes(reads, k):
    """Every entry's code before the filter, sorted."""
    cs = [sm.kmer_codes(r, k) for r in reads]
    return np.sort(np.concatenate(cs)) if cs else np.zeros(0, np.int64)


def entries(reads, k):
    return sum(max(len(r) - k + 1, 0) for r in reads)


def rand_reads(rng, lens, letters=4):
    return [rng.integers(0, letters, size=int(n), dtype=np.uint8) for n in lens]


def one_read_of(rng, n_entries, k):
    return rand_reads(rng, [n_entries + k - 1])


def straddle(T, k=8):
    """Reads whose sorted entries have a run of exactly two equal codes at positions T - 1 and T: with max_occ 1 the run that is
    dropped lies across the first tile boundary of the filter's input."""
    for seed in range(2000):
        rng = np.random.default_rng(1000 + seed)
        reads = rand_reads(rng, [T // 2 + 301, 13, T // 2 + 297, 5])
        c = sorted_codes(reads, k)
        if len(c) > T + 1 and c[T - 1] == c[T] and c[T - 2] != c[T - 1] and c[T + 1] != c[T]:
            return reads
    raise AssertionError("no seed gives a run of two across the boundary")


def homopolymer_sets(k):
    """(reads with 256 entries of the all-zero code, reads with 257): one homopolymer read each, between two-letter reads that
    cannot hold k zeros in a row."""
    rng = np.random.default_rng(7)
    out = []
    for copies in (256, 257):
        side = [np.where(np.arange(n) % (k - 1) == 0, 1, rng.integers(0, 2, size=n)).astype(np.uint8) for n in (300, 211)]
        out.append([side[0], np.zeros(copies + k - 1, np.uint8), side[1]])
        assert int((sorted_codes(out[-1], k) == 0).sum()) == copies
    return out


def check(got, reads, k, max_occ, label=""):
    """got = (codes, gpos, off, dropped) of a build over `reads` (the range's own reads) against the model."""
    codes, gpos, off, dropped = got
    want = sm.Index(reads, k, max_occ)
    assert len(codes) == len(want.codes) and dropped == want.dropped_codes, (label, len(codes), len(want.codes), dropped, want.dropped_codes)
    assert np.array_equal(np.asarray(codes, np.int64), want.codes), label
    assert np.array_equal(np.asarray(gpos, np.int64), want.gpos), label
    assert np.array_equal(np.asarray(off, np.int64), want.off), label
    return want


def both(ctx, reads, k, max_occ, first=0, n_seqs=None, label=""):
    """Device build == host build == model, for the range of the context's DB (GPU tests: ctx = capi.Context); returns the device
    build, its stats and the model's index."""
    n_seqs = len(reads) - first if n_seqs is None else n_seqs
    dev = ctx.index_build(first, n_seqs, k, max_occ, where=1)
    st = ctx.index_last_stats()
    assert st["device_builds"] == 1 and st["host_builds"] == 0, (label, st)
    host = ctx.index_build(first, n_seqs, k, max_occ, where=0)
    sh = ctx.index_last_stats()
    assert sh["device_builds"] == 0 and sh["host_builds"] == 1, (label, sh)
    for a, b in zip(dev[:3], host[:3]):
        assert a.dtype == b.dtype and np.array_equal(a, b), label
    assert dev[3] == host[3], label
    want = check(dev, reads[first:first + n_seqs], k, max_occ, label)
    assert st["entries"] == sh["entries"] == want.all_entries and st["kept"] == sh["kept"] == len(want.codes) and st["dropped_codes"] == want.dropped_codes
    assert st["passes"] == (2 * k + 7) // 8
    return dev, st, want


def gpos_ascends_within_codes(codes, gpos):
    codes, gpos = np.asarray(codes, np.int64), np.asarray(gpos, np.int64)
    same = codes[1:] == codes[:-1]
    return bool(np.all(codes[1:] >= codes[:-1]) and np.all(gpos[1:][same] > gpos[:-1][same]))
