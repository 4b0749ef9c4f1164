"""The numpy model of `hinge overlap --tile` (tests/overlap_tile_common.py) against the generator's ground truth
(hinge_amd.synth_draft) and against the un-tiled model (tests/overlap_common.py): no GPU.

LONG: reads of 30 .. 100 kb at 10 % errors per read, the defaults.  Un-tiled, every read is sampled at step 8 .. 26 (seed_stride:
at most `list` positions per read) and short overlaps between two long reads stay below min_hits from both sides; in tiles of 8 192
bases the step is 2 for every read.  Measured with these models: of the 3 152 ordered pairs sharing >= 2 000 genome bases the
un-tiled model finds 3 142 and the tiled one all; of the 3 200 sharing >= 1 000, 3 157 and 3 200."""
import numpy as np
import pytest

import overlap_common as oc
import overlap_tile_common as otc
import seed_common as sm
from hinge_amd import synth_draft as sd

NOISE = dict(p_sub=0.02, p_ins=0.05, p_del=0.03, min_ovl=1_000)
SHORT = sd.DraftSpec(genome_len=150_000, coverage=12, read_len=(2_000, 40_000), seed=1, **NOISE)
LONG = sd.DraftSpec(genome_len=500_000, coverage=15, read_len=(30_000, 100_000), seed=2, **NOISE)


@pytest.fixture(scope="module")
def long_set():
    d = sd.generate(LONG)
    indexes = {}
    tiled = otc.model_overlap_tiled(d.reads, indexes=indexes)
    plain = oc.model_overlap_jobs(d.reads, range(len(d.reads)), indexes=indexes)
    return d, tiled, plain


def test_long_reads_tiles_find_every_pair_the_whole_read_job_does_not(long_set):
    d, tiled, plain = long_set
    assert len(d.reads) == 115
    got_t, got_p = {tuple(r[:3]) for r in tiled[0]}, {tuple(r[:3]) for r in plain[0]}
    want2, want1 = oc.truth_pairs(d, 2_000), oc.truth_pairs(d, 1_000)
    print("pairs sharing >= 2000: %d, tiled %d, un-tiled %d; >= 1000: %d, tiled %d, un-tiled %d; tiles %d, the largest tile's hits %d" % (
        len(want2), len(want2 & got_t), len(want2 & got_p), len(want1), len(want1 & got_t), len(want1 & got_p), tiled[6]["tiles"], tiled[6]["max_tile_hits"]))
    assert len(want2) == 3152 and len(want1) == 3200
    assert want2 <= got_t and want1 <= got_t                            # all 3 152, and 3 200 of 3 200
    assert len(want2 & got_p) < len(want2) and len(want1 & got_p) < len(want1)      # the un-tiled model: strictly fewer
    # nothing from reads whose genome intervals are disjoint, in either form; no tile's list overflowed
    assert not [r for r in tiled[0] if oc.shared_bases(d, r[0], r[1]) <= 0]
    assert not [r for r in plain[0] if oc.shared_bases(d, r[0], r[1]) <= 0]
    assert tiled[6]["overflow"] == 0 and tiled[6]["truncated"] == 0 and tiled[6]["max_tile_hits"] < oc.LIST
    assert tiled[6]["multi_tile_jobs"] == tiled[6]["jobs"] == 2 * len(d.reads)


def test_one_tile_queries_equal_the_whole_read_job():
    """SHORT: every query of one tile (alen - k + 1 <= 8 192: its un-tiled step is the call's too) gets the un-tiled model's
    candidates, status and hits, value for value."""
    d = sd.generate(SHORT)
    one = [a for a in range(len(d.reads)) if otc.tile_count(len(d.reads[a]), oc.K, otc.TILE) == 1]
    assert len(one) >= 10 and len(one) < len(d.reads)
    indexes = {}
    rows, cnt, dg, rep, status, hits, st = otc.model_overlap_tiled(d.reads, picks=one, indexes=indexes)
    prow, pcnt, pdg, prep, pstatus, phits, pst = oc.model_overlap_jobs(d.reads, one, indexes=indexes)
    assert len(rows) > 100
    assert (rows, cnt, dg, rep) == (prow, pcnt, pdg, prep)
    assert all(status[a] == pstatus[a] and hits[a] == phits[a] for a in one)


def test_tile_counts_at_the_seams():
    k = oc.K
    for T in (64, 256, 8192):
        adv = T // 2
        for L, want in ((T - 1, 1), (T, 1), (T + 1, 2), (T + adv, 2), (T + adv + 1, 3), (T + 7 * adv, 8), (1, 1)):
            alen = L + k - 1
            assert otc.tile_count(alen, k, T) == want, (T, L)
            # every sampled position lies in a tile, the last tile is not empty of positions at step 1, and none starts beyond the read
            assert (want - 1) * adv <= L - 1 < (want - 1) * adv + T
        assert otc.tile_count(k - 1, k, T) == 1 and otc.tile_count(0, k, T) == 1


def test_phase_is_the_reads_not_the_tiles():
    """step 3, tile 64 (adv 32: no multiple of 3): a tile's positions are the read's multiples of 3, so tile 1 begins at 33, and
    the union of the tiles' hits is the read's hit list."""
    rng = np.random.default_rng(5)
    g = rng.integers(0, 4, size=400, dtype=np.uint8)
    reads = [g[:300].copy(), g.copy()]
    index = sm.Index(reads, oc.K, oc.MAX_OCC)
    b, dd, p = otc.query_hits(index, 0, 0, reads[0], 3)
    assert len(p) and np.all(p % 3 == 0)
    tiles = otc.job_tiles(index, 0, 0, reads[0], 64, 3, oc.WINDOW, 64, oc.MAX_PARTNERS, 1)
    assert len(tiles) == otc.tile_count(300, oc.K, 64)
    for t, (st, nh, over, cands) in enumerate(tiles):
        inside = (p >= 32 * t) & (p < 32 * t + 64)
        assert nh == int(inside.sum()) and not over
        for c in cands:
            assert c[3] % 3 == 0 and 32 * t <= c[3] < 32 * t + 64 and c[2] == 300               # one diagonal: both reads begin together
    assert [c[3] for c in tiles[1][3]] and min(p[p >= 32]) == 33
    st, nh, cands = otc.reduce_tiles(tiles)
    assert st == 0 and [c[0] for c in cands] == [1] and cands[0][1] == max(c[1] for t in tiles for c in t[3])
    assert nh == sum(t[1] for t in tiles) > len(p)                        # tiles overlap by half: their hits count twice
