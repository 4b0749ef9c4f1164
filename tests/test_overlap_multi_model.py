"""The numpy model of `hinge overlap --max-stretches` (tests/overlap_multi_common.py) against the generator's ground truth
(hinge_amd.synth_draft) and on hand-made hit lists and records: no GPU.

Plasmid set (8 kb circular, noise-free, reads of 5 .. 6 kb: every pair of reads meets at both ends): at 2 stretches the records
equal the generator's 308, end point for end point; at 1 stretch 272 of them, one per (a, b, strand).
CLEAN and NOISY of test_overlap_model.py (linear, no repeat): rounds 1 and 2 add no candidate at all.
Repeat set (a 1 200-base copy 3 kb away, 10 % errors per read): every expected stretch is a candidate at 3 stretches."""
import numpy as np
import pytest

import overlap_common as oc
import overlap_multi_common as om
from hinge_amd import synth_draft as sd
from test_overlap_model import CLEAN, CLEAN_KW, NOISY

PLASMID = sd.DraftSpec(genome_len=8_000, circular=True, coverage=12, read_len=(5_000, 6_000), min_ovl=1_000, seed=5)
REPEAT = sd.DraftSpec(genome_len=20_000, coverage=12, read_len=(5_000, 7_000), min_ovl=1_000, p_sub=0.02, p_ins=0.05, p_del=0.03, repeat=(1_200, 6_000, 9_000), seed=7)
# a candidate is "on" an expected stretch if its diagonal lies within `window` of the stretch's: the copies are 3 000 bases apart,
# and the drift of a diagonal over a 7 kb read at 8 % indels is a random walk of sd sqrt(560) = 24
ON_TOL = oc.WINDOW


def rec_set(d):
    return sorted((int(q["aread"]), int(q["bread"]), int(q["flags"]) & 1, int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in d.rec)


def test_plasmid_set_both_stretches_of_every_pair():
    d = sd.generate(PLASMID)
    want = rec_set(d)
    keys = {r[:3] for r in want}
    assert len(d.reads) == 17 and len(want) == 308 and len(keys) == 272 and sum(1 for k in keys if sum(r[:3] == k for r in want) == 2) == 36
    two, per_round, merged, dropped = om.program_records(d.reads, max_stretches=2, **CLEAN_KW)
    assert sorted(two) == want and dropped == 0
    one, per_round1, merged1, dropped1 = om.program_records(d.reads, max_stretches=1, **CLEAN_KW)
    assert len(one) == 272 and set(one) <= set(want) and {r[:3] for r in one} == keys and dropped1 == 0
    assert per_round[0] == per_round1[0] and per_round[1] > 0


@pytest.mark.parametrize("spec,kw,round0", [(NOISY, {}, 1792), (CLEAN, CLEAN_KW, 1865)])
def test_no_second_stretch_without_a_repeat(spec, kw, round0):
    d = sd.generate(spec)
    rows, cnt, dg, rep, status, hits, st, rnd = om.model_overlap_multi(d.reads, max_stretches=3, **kw)
    assert [rnd.count(x) for x in range(3)] == [round0, 0, 0]
    base = oc.model_overlap(d.reads, **kw)
    assert (rows, cnt, dg, rep, status, hits) == base[:6]


def test_repeat_set_every_expected_stretch_is_a_candidate():
    d = sd.generate(REPEAT)
    assert len(d.reads) == 40
    want = om.expected_stretches(d)
    assert len(want) == 272
    rows, cnt, dg, rep, status, hits, st, rnd = om.model_overlap_multi(d.reads, max_stretches=3)
    assert [rnd.count(x) for x in range(3)] == [866, 290, 84]
    have = {}
    for r, g in zip(rows, dg):
        have.setdefault(tuple(r[:3]), []).append(g)
    missing = [w for w in want if not any(abs(g - (w[6] - w[4])) < ON_TOL for g in have.get(w[:3], []))]
    assert not missing, missing[:5]


# ---- the suppression bounds on hand-made hit lists ------------------------------------------------------------------------------
def _hits(groups):
    """groups: [(b, d, n)] -> n hits of partner b on diagonal d (p = 0, 1, ..)."""
    b, d, p = [], [], []
    for bb, dd, n in groups:
        b += [bb] * n; d += [dd] * n; p += list(range(len(p), len(p) + n))
    return b, d, p


def test_suppression_bounds_are_exclusive():
    """The pick: the first of five hits on d = 100, its window [100, 116) holding five more on 110 (cnt 10, or 12 with `hi` inside).
    One hit on `lo` (its window [lo, lo + 16) reaches the pick from lo = 85 on: cnt 6 < 10) and two on `hi`.  d[e] - window = 84
    and d[e] + window = 116 stay live and are the candidates of rounds 1 and 2; one diagonal inside either is dead."""
    W = 16
    for lo, hi, later in ((84, 116, [(7, 2, 116, 12), (7, 1, 84, 0)]), (85, 116, [(7, 2, 116, 12)]), (84, 115, [(7, 1, 84, 0)]), (85, 115, [])):
        b, d, p = _hits([(7, lo, 1), (7, 100, 5), (7, 110, 5), (7, hi, 2)])
        rounds = om.pick_rounds(b, d, p, W, 1, 4)
        c = 10 if hi == 116 else 12
        assert rounds[0] == [(7, c, d[1 + c // 2], 1 + c // 2)], (lo, hi, rounds)
        assert [x for r in rounds[1:] for x in r] == later, (lo, hi, rounds)


def test_a_dead_representative_is_still_the_representative():
    """Round 0 picks the first hit on d = 100 (cnt 12: 100 .. 115) and kills 85 .. 115: all but the hit on 84.  That one is live in
    round 1 with cnt 5 - its window [84, 100) counts the four dead hits on 93, none of the pick's window - and its representative,
    element 0 + 5 // 2, is one of the dead four.  Nothing is live in round 2."""
    b, d, p = _hits([(0, 84, 1), (0, 93, 4), (0, 100, 6), (0, 110, 6)])
    assert om.pick_rounds(b, d, p, 16, 3, 3) == [[(0, 12, 110, 11)], [(0, 5, 93, 2)], []]


def test_fewer_elements_than_rounds_and_the_min_hits_threshold():
    W = 16
    b, d, p = _hits([(1, 50, 1), (1, 500, 1)])
    assert om.pick_rounds(b, d, p, W, 1, 4) == [[(1, 1, 50, 0)], [(1, 1, 500, 1)], [], []]
    for second, n in ((3, 1), (2, 0)):                                     # a second pick of exactly min_hits, and of min_hits - 1
        b, d, p = _hits([(1, 50, 5), (1, 500, second), (2, 70, 3)])
        rounds = om.pick_rounds(b, d, p, W, 3, 3)
        assert [len(r) for r in rounds] == [2, n, 0]
        assert rounds[0] == [(1, 5, 50, 2), (2, 3, 70, 5 + second + 1)]
        if n:
            assert rounds[1] == [(1, 3, 500, 5 + 1)]


# ---- the program's merge and duplicate rules ------------------------------------------------------------------------------------
def test_merge_is_single_linkage_below_window():
    W = 256
    c = lambda dg, cnt, from_a: (0, 1, 0, dg, cnt, from_a)
    assert om.merge([c(1000, 10, 1), c(1000 + W - 1, 12, 0)], W) == ([(0, 1, 0, 1000)], 1)                  # a's side goes first
    assert om.merge([c(1000, 10, 0), c(1000 + W - 1, 12, 0)], W) == ([(0, 1, 0, 1000 + W - 1)], 1)          # then the largest count
    assert om.merge([c(1000, 10, 1), c(1000 + W - 1, 12, 1), c(1010, 30, 0)], W) == ([(0, 1, 0, 1000 + W - 1)], 2)
    assert om.merge([c(1000, 10, 1), c(1000 + W, 12, 0)], W) == ([(0, 1, 0, 1000), (0, 1, 0, 1000 + W)], 0)
    # a chain: every neighbour below W, the ends 2 (W - 1) apart; of a's side's equal counts the smaller diagonal
    assert om.merge([c(0, 9, 0), c(W - 1, 9, 1), c(2 * W - 2, 9, 1)], W) == ([(0, 1, 0, W - 1)], 2)
    assert om.merge([c(5, 9, 0), c(0, 9, 0)], W) == ([(0, 1, 0, 0)], 1)
    # other keys do not merge
    assert om.merge([(0, 1, 0, 7, 9, 1), (0, 1, 1, 7, 9, 1), (0, 2, 0, 7, 9, 1)], W)[1] == 0


def test_canonical_frame_mirrors_the_larger_read():
    rlen = [500, 300]
    rows = [(0, 1, 0), (1, 0, 0), (1, 0, 1)]
    got = om.canonical(rows, [40, -40, 10], [7, 8, 9], rlen)
    assert got == [(0, 1, 0, 40, 7, 1), (0, 1, 0, 40, 8, 0), (0, 1, 1, oc.alen_blen_mirror(300, 500, 1, 10), 9, 0)]


def test_duplicate_rule():
    W = 256
    main = (0, 1, 0, 100, 5100, 0, 5000)
    # the same alignment twice
    assert om.drop_duplicates([main, main], W) == ([main], 1)
    # a cut piece sharing one end (its begin diagonal is off by 300, its end diagonal the same)
    piece = (0, 1, 0, 3000, 5100, 2600, 5000)
    assert om.drop_duplicates([piece, main], W) == ([main], 1)
    # a cross alignment wholly inside both ranges, a copy distance (3 000) away on both ends: kept
    cross = (0, 1, 0, 1000, 2200, 3900, 5100)
    assert om.drop_duplicates([cross, main], W) == ([main, cross], 0)
    # disjoint A ranges on one diagonal: kept; another key: kept
    far = (0, 1, 0, 6000, 7000, 5900, 6900)
    other = (0, 2, 0, 100, 5100, 0, 5000)
    assert om.drop_duplicates([far, main, other], W) == ([main, far, other], 0)
