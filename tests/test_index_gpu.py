"""The k-mer index built on the GPU (hinge_index_build, index_kernels.h): Context.index_build(where=1) value for
value - codes, gpos, off, the count, dropped_codes - against where=0 (the host build of seed_index.h) and against the numpy model
seed_common.Index, at the smallest shapes at which each part can go wrong (tests/index_common.py; tests/test_index_host.py runs
the same kernels on the CPU under sanitizers)."""
import os

import numpy as np
import pytest

import index_common as ic
from hinge_amd import formats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.lib.hinge_index_tile()
    assert t == ic.tile_from_source() and t % 64 == 0
    return t


@pytest.fixture(scope="module")
def random_set(ctx, tmp_path_factory):
    """About 200 000 entries of four letters in reads whose lengths are no multiples of 4, one DB for the tests that share it
    (each of them makes it the context's DB again: _use)."""
    rng = np.random.default_rng(31)
    lens = [int(v) | 1 for v in rng.integers(3000, 7000, size=40)] + [4098, 6, 2049, 15]
    reads = ic.rand_reads(rng, lens)
    assert sum(n % 4 != 0 for n in lens) >= 40
    wd = str(tmp_path_factory.mktemp("index_random"))
    _set_db(ctx, wd, reads)
    return reads, wd


def _set_db(ctx, wd, reads):
    from hinge_amd import capi
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))


def _use(ctx, random_set):
    from hinge_amd import capi
    reads, wd = random_set
    capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))
    return reads


def _both(ctx, reads, k, max_occ, first=0, n_seqs=None, label=""):
    """Device build == host build == model, for the range (index_common.both); returns the device build and its stats."""
    return ic.both(ctx, reads, k, max_occ, first, n_seqs, label)[:2]


def test_entry_counts_around_the_tile(ctx, T, tmp_path):
    rng = np.random.default_rng(32)
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 7):
        reads = ic.rand_reads(rng, [3, 7, 1]) if n == 0 else ic.one_read_of(rng, n, 9)
        _set_db(ctx, os.path.join(str(tmp_path), "n%d" % n), reads)
        _, st = _both(ctx, reads, 9, 4, label="n%d" % n)
        assert st["entries"] == n


def test_random_set_every_k(ctx, random_set):
    """k = 8 (two passes), 12 (three), 15 (a partial top digit), 16 (all 32 bits: codes with the top bit set)."""
    reads = _use(ctx, random_set)
    for k, max_occ in ((8, 64), (12, 16), (15, 16), (16, 16)):
        dev, st = _both(ctx, reads, k, max_occ, label="k%d" % k)
        assert 190000 < st["entries"] < 260000
        if k == 16:
            assert (dev[0] >= np.uint32(2 ** 31)).any() and (dev[0] < np.uint32(2 ** 31)).any()
        if k == 8:
            assert st["dropped_codes"] == 0 and ic.gpos_ascends_within_codes(dev[0], dev[1])


def test_stability(ctx, T, tmp_path):
    """Two-letter reads and a homopolymer of 5 000 bases (one code with thousands of entries across several tiles) at max_occ 256;
    the homopolymer's code at exactly 256 entries (kept) and 257 (dropped); gpos ascends inside every code."""
    rng = np.random.default_rng(33)
    reads = ic.rand_reads(rng, [2500, 11, 1750, 3001, 1], letters=2) + [np.zeros(5000, np.uint8)]
    _set_db(ctx, os.path.join(str(tmp_path), "two"), reads)
    for k in (8, 13):
        dev, st = _both(ctx, reads, k, 256, label="two_letter_k%d" % k)
        assert st["entries"] > 3 * T and st["dropped_codes"] >= 1 and 0 not in dev[0].tolist() and ic.gpos_ascends_within_codes(dev[0], dev[1])
        assert k != 8 or np.unique(dev[0], return_counts=True)[1].max() > 16
    for copies, rd in zip((256, 257), ic.homopolymer_sets(10)):
        _set_db(ctx, os.path.join(str(tmp_path), "c%d" % copies), rd)
        dev, st = _both(ctx, rd, 10, 256, label="copies%d" % copies)
        assert int((dev[0] == 0).sum()) == (256 if copies == 256 else 0) and ic.gpos_ascends_within_codes(dev[0], dev[1])
        assert (dev[3] >= 1) == (copies == 257)


def test_max_occ_1_run_across_a_tile_boundary(ctx, T, tmp_path):
    reads = ic.straddle(T)
    _set_db(ctx, str(tmp_path), reads)
    dev, st = _both(ctx, reads, 8, 1, label="straddle")
    c = ic.sorted_codes(reads, 8)
    assert c[T - 1] == c[T] and int(c[T]) not in dev[0].tolist() and st["dropped_codes"] >= 1


def test_offsets_and_ranges(ctx, tmp_path):
    """Reads shorter than k between longer ones; first > 0; a single-read range; a range of short reads: gpos is relative to the range."""
    rng = np.random.default_rng(34)
    reads = ic.rand_reads(rng, [5, 3333, 14, 1, 4021, 15, 7, 1290, 3])
    _set_db(ctx, str(tmp_path), reads)
    for first, n in ((0, 9), (1, 4), (4, 1), (5, 2), (2, 7), (0, 1), (3, 0)):
        dev, st = _both(ctx, reads, 15, 16, first, n, label="range%d_%d" % (first, n))
        assert dev[2][0] == 0 and len(dev[2]) == n + 1
        if (first, n) == (4, 1):
            assert dev[1].max() == 4021 - 15 and dev[1].min() == 0
        if (first, n) == (1, 4):
            assert dev[2].tolist() == [0, 3333, 3347, 3348, 7369]


def test_determinism(ctx, random_set):
    reads = _use(ctx, random_set)
    a = ctx.index_build(0, len(reads), 15, 16, where=1)
    b = ctx.index_build(0, len(reads), 15, 16, where=1)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_budget_and_switch(ctx, random_set, monkeypatch):
    reads = _use(ctx, random_set)
    n = len(reads)
    monkeypatch.delenv("HINGE_INDEX_SCRATCH_BYTES", raising=False)
    monkeypatch.delenv("HINGE_INDEX_SCRATCH_MB", raising=False)
    monkeypatch.delenv("HINGE_INDEX_DEVICE", raising=False)
    dev = ctx.index_build(0, n, 15, 16)                                    # the defaults: where = -1, the device
    st = ctx.index_last_stats()
    assert st["device_builds"] == 1 and st["host_builds"] == 0 and 16 * st["entries"] < st["scratch_bytes"] < 20 * st["entries"]
    monkeypatch.setenv("HINGE_INDEX_SCRATCH_BYTES", str(st["scratch_bytes"] - 1))
    low = ctx.index_build(0, n, 15, 16, where=1)
    sl = ctx.index_last_stats()
    assert sl["device_builds"] == 0 and sl["host_builds"] == 1
    monkeypatch.setenv("HINGE_INDEX_SCRATCH_BYTES", str(st["scratch_bytes"]))
    ctx.index_build(0, n, 15, 16, where=1)
    assert ctx.index_last_stats()["device_builds"] == 1
    monkeypatch.delenv("HINGE_INDEX_SCRATCH_BYTES")
    monkeypatch.setenv("HINGE_INDEX_DEVICE", "0")
    off = ctx.index_build(0, n, 15, 16)
    so = ctx.index_last_stats()
    assert so["device_builds"] == 0 and so["host_builds"] == 1
    for got in (low, off):
        assert all(np.array_equal(x, y) for x, y in zip(dev[:3], got[:3])) and dev[3] == got[3]


def test_errors(ctx, random_set):
    from hinge_amd import capi
    reads = _use(ctx, random_set)
    n = len(reads)
    for k, max_occ in ((7, 16), (17, 16), (15, 0), (15, 257)):
        with pytest.raises(capi.HingeError) as e:
            ctx.index_build(0, n, k, max_occ, where=1)
        assert e.value.code == capi.HINGE_E_ARG
    for first, cnt in ((0, n + 1), (n, 1), (-1, 2), (2, -1)):
        with pytest.raises(capi.HingeError) as e:
            ctx.index_build(first, cnt, 15, 16, where=1)
        assert e.value.code == capi.HINGE_E_RANGE
