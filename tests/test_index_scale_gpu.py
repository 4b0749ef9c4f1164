"""The k-mer index built on the GPU at a real block's size (index_kernels.h, index_capi.inc): device build == host
build == numpy model (index_common.both) where tests/test_index_gpu.py stops short - the scan of the n + 1 flags at three levels
and at the two seams in front of it (n + 1 == C * C: a second level of exactly one full chunk; C * C + 1: a second level of C + 1
elements and a third of 2, the one place where the sums array is carved at depth 2), the table scan at one chunk, one chunk less
an entry and one chunk plus 256 slots (8 and 9 tiles), every pass count on 4.3 M entries, and indexes that keep nothing.
C = IDX_SCAN_CHUNK, T = IDX_TILE.  The set is index_common.block_set(): 1030 reads, about 4.33 M entries."""
import os

import numpy as np
import pytest

import index_common as ic
import overlap_common as oc
import seed_common as sm
from test_index_gpu import _set_db

pytestmark = pytest.mark.gpu

DEFAULT_BUDGET = 2048 << 20                                              # HINGE_INDEX_SCRATCH_MB's default, in bytes


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


@pytest.fixture(scope="module")
def C():
    return ic.scan_chunk_from_source()


@pytest.fixture(scope="module")
def block():
    return ic.block_set()


@pytest.fixture(scope="module")
def block_db(ctx, block, tmp_path_factory):
    """The whole block set as a DB, written once (each test that uses it makes it the context's DB again: _use)."""
    wd = str(tmp_path_factory.mktemp("index_block"))
    _set_db(ctx, wd, block)
    return wd


def _use(ctx, wd):
    from hinge_amd import capi
    capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for name in ("HINGE_INDEX_SCRATCH_BYTES", "HINGE_INDEX_SCRATCH_MB", "HINGE_INDEX_DEVICE"):
        monkeypatch.delenv(name, raising=False)


def _mixed(want):
    """The conditions on the model alone: the scanned flags are a real mix, and some codes are dropped."""
    assert 0.1 < len(want.codes) / want.all_entries < 0.9 and want.dropped_codes > 0, (len(want.codes), want.all_entries, want.dropped_codes)


@pytest.mark.parametrize("which", ("below", "at"))
def test_flag_scan_at_the_seam_of_the_third_level(ctx, block, C, tmp_path, which):
    """n + 1 == C * C: two levels, the second exactly one full chunk; n + 1 == C * C + 1: three, the third of 2 elements."""
    n = C * C - 1 if which == "below" else C * C
    reads = ic.sized(block, 12, n)
    _set_db(ctx, str(tmp_path), reads)
    dev, st, want = ic.both(ctx, reads, 12, 3, label=which)
    assert want.all_entries == n and ic.scan_levels(n + 1, C) == (2 if which == "below" else 3)
    assert -(-(n + 1) // C) == (C if which == "below" else C + 1)
    _mixed(want)
    assert 0 < st["scratch_bytes"] < DEFAULT_BUDGET


def test_flag_scan_at_three_levels(ctx, block, block_db, C):
    _use(ctx, block_db)
    dev, st, want = ic.both(ctx, block, 12, 3, label="block_k12")
    assert want.all_entries + 1 > C * C + C and ic.scan_levels(want.all_entries + 1, C) == 3
    _mixed(want)
    assert 0 < st["scratch_bytes"] < DEFAULT_BUDGET


def test_table_scan_around_one_chunk(ctx, C, tmp_path):
    """table_len = 256 x tiles: 8 tiles are exactly one chunk of the scan, 9 tiles one chunk and 256 slots of the second."""
    T = ctx.lib.hinge_index_tile()
    assert T == ic.tile_from_source() and 256 * 8 == C
    rng = np.random.default_rng(41)
    for n in (8 * T - 1, 8 * T, 8 * T + 1):
        reads = ic.one_read_of(rng, n, 9)
        _set_db(ctx, os.path.join(str(tmp_path), "n%d" % n), reads)
        dev, st, want = ic.both(ctx, reads, 9, 1, label="n%d" % n)
        assert st["entries"] == n and -(-n // T) == (8 if n <= 8 * T else 9) and ic.scan_levels(256 * -(-n // T), C) == (1 if n <= 8 * T else 2)
        assert 0 < len(want.codes) < n and want.dropped_codes > 0         # (4^9 codes in 16 384 entries: some hundred twice, dropped at max_occ 1)


def test_four_passes_at_depth_k16(ctx, block, block_db):
    """All 32 bits of the code, four full digits, codes on both sides of 2^31, on 4.3 M entries."""
    _use(ctx, block_db)
    dev, st, want = ic.both(ctx, block, 16, 16, label="block_k16")
    assert st["passes"] == 4 and (dev[0] >= np.uint32(2 ** 31)).any() and (dev[0] < np.uint32(2 ** 31)).any()
    assert st["kept"] > (1 << 22) and 0 < st["scratch_bytes"] < DEFAULT_BUDGET


def test_two_passes_at_depth_k8(ctx, block, block_db):
    """k = 8, max_occ 256 on the block set: 65 536 codes of 23 .. 129 entries each, so every one is kept and the scanned flags
    are all 1; gpos ascends inside every code (the sort is stable across 2 115 tiles)."""
    _use(ctx, block_db)
    dev, st, want = ic.both(ctx, block, 8, 256, label="block_k8_all")
    assert st["passes"] == 2 and st["kept"] == st["entries"] > (1 << 22) and st["dropped_codes"] == 0 and ic.gpos_ascends_within_codes(dev[0], dev[1])


def test_keeps_nothing_at_depth_k8(ctx, block, block_db):
    """k = 8 at a max_occ below the rarest code's count: all 65 536 codes are over-full, kept == 0 (the flags are all 0, the
    compaction is skipped) and dropped_codes is the number of distinct codes."""
    _use(ctx, block_db)
    per_code = np.bincount(ic.sorted_codes(block, 8), minlength=1 << 16)
    assert per_code.min() > 16
    dev, st, want = ic.both(ctx, block, 8, 16, label="block_k8_none")
    assert st["entries"] > (1 << 22) and st["kept"] == 0 and len(dev[0]) == 0 and st["dropped_codes"] == dev[3] == int((per_code > 0).sum()) == 1 << 16


def test_an_index_that_keeps_nothing(ctx, tmp_path):
    """One homopolymer read and two reads shorter than k: entries > 0, one code, over-full.  The vote kernels then search an index
    of no entries (n_entries = 0, search_top = 0): every status NONE, no rows."""
    reads = [np.zeros(300, np.uint8), np.asarray([0, 1, 2, 3, 0, 1, 2], np.uint8), np.asarray([3, 3, 1], np.uint8)]
    _set_db(ctx, str(tmp_path), reads)
    for k in (8, 15, 16):
        dev, st, want = ic.both(ctx, reads, k, 256, label="nothing_k%d" % k)
        assert st["entries"] == 300 - k + 1 > 256 and st["kept"] == 0 and len(dev[0]) == 0 and dev[3] == st["dropped_codes"] == 1
        assert dev[2].tolist() == [0, 300, 307, 310]
    pl, count, diag, rep, status, hits = ctx.overlap_run()
    assert len(pl) == 0 and len(count) == 0 and status.tolist() == [[oc.NONE, oc.NONE]] * 3 and hits.tolist() == [[0, 0]] * 3
    st = ctx.overlap_stats()
    assert st["entries"] == 0 and st["dropped_codes"] == 1 and st["blocks"] == 1 and st["jobs"] == 6
    pl, count, diag, rep, status, hits, rnd = ctx.overlap_run(max_stretches=2)
    assert len(pl) == 0 and status.tolist() == [[oc.NONE, oc.NONE]] * 3 and ctx.overlap_stats()["entries"] == 0
    pl, count, diag, n_placed, status = ctx.seed_run()
    assert len(pl) == 0 and n_placed.tolist() == [0, 0, 0] and status.tolist() == [[sm.NONE, sm.NONE]] * 3
    st = ctx.seed_stats()
    assert st["entries"] == 0 and st["dropped_codes"] == 1 and st["unplaced"] == 3 and st["jobs"] == 6
