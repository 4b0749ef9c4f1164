"""The numpy model of `hinge overlap` (tests/overlap_common.py) against the generator's ground truth (hinge_amd.synth_draft): no GPU.

Clean set (noise-free, linear): candidates -> symmetrised -> both lengths >= 1 000 equals the generator's records, pair for pair and
end point for end point (the overlaps end at read ends and the bases are identical, so the projection along a hit's diagonal IS
the overlap).  The clean set runs at --step 16 --list 8192: noise-free reads hit at EVERY sampled position of every read that
covers it, so at step 2 a 3 kb read at 12x has ~18 000 hits and the list (4 096) overflows; at step 16 the largest job keeps 2 646.
Noisy set (10 % errors per read, the defaults): recall of the pairs sharing >= 2 000 genome bases, and no candidate from pairs
whose genome intervals are disjoint.  Measured (tools/overlap_measure.py recall): 690 of 690 pairs, the smallest count 17."""
import numpy as np
import pytest

import overlap_common as oc
from hinge_amd import synth_draft as sd

CLEAN = sd.DraftSpec(genome_len=20_000, coverage=12, read_len=(2_000, 4_000), min_ovl=1_000)
NOISY = sd.DraftSpec(genome_len=20_000, coverage=12, read_len=(2_000, 4_000), min_ovl=1_000, p_sub=0.02, p_ins=0.05, p_del=0.03)
CLEAN_KW = dict(step=16, list_=8192)


@pytest.fixture(scope="module")
def clean():
    d = sd.generate(CLEAN)
    return d, oc.model_overlap(d.reads, **CLEAN_KW)


@pytest.fixture(scope="module")
def noisy():
    d = sd.generate(NOISY)
    return d, oc.model_overlap(d.reads)


def test_clean_set_equals_the_generator(clean):
    d, (rows, cnt, dg, rep, status, hits, st) = clean
    assert st["overflow"] == 0 and st["truncated"] == 0 and st["blocks"] == 1 and st["jobs"] == 2 * len(d.reads)
    sym, sdg, added = oc.symmetrise(rows, dg, d.rlen)
    got = {tuple(r[:3]): tuple(r[3:]) for r in oc.keep_pairs(sym, 1000)}
    want = oc.rec_rows(d)
    assert len(want) > 1000
    assert set(got) == set(want)
    assert all(got[x] == want[x] for x in want)
    # nothing at all - before any filter - for pairs whose genome intervals are disjoint
    assert not [r for r in sym if oc.shared_bases(d, r[0], r[1]) <= 0]


def test_noisy_set_recall_and_precision(noisy):
    d, (rows, cnt, dg, rep, status, hits, st) = noisy
    assert st["overflow"] == 0 and st["truncated"] == 0
    want = oc.truth_pairs(d, 2_000)
    got = {tuple(r[:3]) for r in rows}
    recall = len(want & got) / len(want)
    print("pairs sharing >= 2000 bases: %d, candidates of them: %d, recall %.4f" % (len(want), len(want & got), recall))
    assert len(want) > 500 and recall >= 0.95
    assert not [r for r in rows if oc.shared_bases(d, r[0], r[1]) <= 0]
    sym, sdg, added = oc.symmetrise(rows, dg, d.rlen)
    assert {(r[1], r[0], r[2]) for r in sym} == {tuple(r[:3]) for r in sym}


def test_projection_and_mirror_are_consistent():
    """A candidate's mirror, mirrored again, is the candidate; the projections of both cover the same bases of both reads."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        alen, blen, comp = int(rng.integers(20, 500)), int(rng.integers(20, 500)), int(rng.integers(0, 2))
        d = int(rng.integers(1, alen + blen))
        dg = oc.diag_of(alen, blen, comp, d)
        q = oc.project(alen, blen, dg, 15)
        md = oc.alen_blen_mirror(alen, blen, comp, dg)
        assert oc.alen_blen_mirror(blen, alen, comp, md) == dg
        m = oc.project(blen, alen, md, 15)
        assert (q is None) == (m is None)
        if q is None:
            continue
        ab, ae, bb, be = q
        assert 0 <= ab < ae <= alen and 0 <= bb < be <= blen and ae - ab == be - bb and (ab == 0 or bb == 0) and (ae == alen or be == blen)
        if comp:
            assert m == (blen - be, blen - bb, alen - ae, alen - ab)
        else:
            assert m == (bb, be, ab, ae)


def test_blocks_cut_at_block_bases():
    assert oc.blocks([5, 5, 5, 5], 10) == [(0, 2), (2, 4)]
    assert oc.blocks([5, 50, 5], 10) == [(0, 1), (1, 2), (2, 3)]
    assert oc.blocks([5, 5, 5], 100) == [(0, 3)] and oc.blocks([], 10) == []
