"""The numpy model of `hinge overlap --tile T --tile-stretches S` (tests/overlap_tile_multi_common.py) against the generator's ground
truth (hinge_amd.synth_draft) and on hand-made tile rows: no GPU.

LONGREP (66 reads of 30 .. 60 kb, 2 824 024 bases, 10 % errors per read, a 1 500-base copy 20 kb away): 334 expected stretches, 188 of
them cross alignments of the two copies.  Whole-read rounds (model_overlap_multi, 3 rounds: the step is 8 .. 15 for these reads) miss
26, tiles with one candidate per partner (model_overlap_tiled, tile 8 192) miss 176, all of them cross; tiles with rounds miss none.
The repeat-free long set of test_overlap_tile_model.py at 2 rounds: round 0 is model_overlap_tiled's 3 242 candidates, round 1 has
4 - remnants of one drifting overlap, 258 .. 298 diagonals from their pair's first pick."""
import pytest

import overlap_common as oc
import overlap_multi_common as omc
import overlap_tile_common as otc
import overlap_tile_multi_common as otm
from hinge_amd import synth_draft as sd
from test_overlap_tile_model import LONG

LONGREP = sd.DraftSpec(genome_len=300_000, coverage=10, read_len=(30_000, 60_000), min_ovl=1_000, p_sub=0.02, p_ins=0.05, p_del=0.03, repeat=(1_500, 120_000, 140_000), seed=11)


def test_long_reads_with_a_repeat_need_both():
    d = sd.generate(LONGREP)
    assert len(d.reads) == 66 and sum(len(r) for r in d.reads) == 2_824_024
    want = omc.expected_stretches(d)
    assert len(want) == 334 and sum(1 for w in want if w[3] == "cross") == 188
    indexes = {}
    whole = omc.model_overlap_multi(d.reads, max_stretches=3)
    assert [whole[7].count(x) for x in range(3)] == [1121, 131, 22]
    missed = otm.stretches_missed(d, whole[0], whole[2], expected=want)
    assert len(missed) == 26 and {w[3] for w in missed} == {"cross"}
    tiled = otc.model_overlap_tiled(d.reads, indexes=indexes)
    assert len(tiled[0]) == 1149
    missed = otm.stretches_missed(d, tiled[0], tiled[2], expected=want)
    assert len(missed) == 176 and {w[3] for w in missed} == {"cross"}
    both = otm.model_overlap_tiled_multi(d.reads, max_stretches=3, indexes=indexes)
    assert [both[7].count(x) for x in range(3)] == [1149, 157, 30]
    assert not otm.stretches_missed(d, both[0], both[2], expected=want)
    # round 0 is the one-candidate model's answer
    r0 = [x for x, r in enumerate(both[7]) if r == 0]
    assert [both[0][x] for x in r0] == tiled[0] and [both[1][x] for x in r0] == tiled[1] and [both[3][x] for x in r0] == tiled[3]


def test_no_repeat_costs_four_remnants():
    d = sd.generate(LONG)
    indexes = {}
    tiled = otc.model_overlap_tiled(d.reads, indexes=indexes)
    both = otm.model_overlap_tiled_multi(d.reads, max_stretches=2, indexes=indexes)
    assert [both[7].count(x) for x in range(2)] == [3242, 4]
    r0 = [x for x, r in enumerate(both[7]) if r == 0]
    assert [both[0][x] for x in r0] == tiled[0] and [both[1][x] for x in r0] == tiled[1] and [both[2][x] for x in r0] == tiled[2] and [both[3][x] for x in r0] == tiled[3]
    assert both[4] == tiled[4] and both[5] == tiled[5]
    first = {tuple(both[0][x][:3]): both[2][x] for x in r0}
    away = sorted(abs(both[2][x] - first[tuple(both[0][x][:3])]) for x, r in enumerate(both[7]) if r == 1)
    assert away == [258, 266, 277, 298]                                  # just past the window: one drifting overlap's other tiles


# ---- hand-made tile rows through the reduce rule ------------------------------------------------------------------------------------
def _tile(rounds, nh=100, over=False, st=0):
    """A tile row: rounds = [[(b, cnt, d, p)]]."""
    return (st if any(rounds) else oc.NONE, nh, over, rounds)


W = 256


def test_reduce_window_bounds():
    for off, n in ((W, 2), (W - 1, 1), (-W, 2), (-(W - 1), 1)):         # exactly `window` away stays live; window - 1 does not
        tiles = [_tile([[(5, 40, 1000, 10)], []]), _tile([[(5, 30, 1000 + off, 5000)], []])]
        st, nh, rounds = otm.reduce_tiles_multi(tiles, W, 8, 2)
        assert [len(r) for r in rounds] == [1, n - 1] and rounds[0] == [(5, 40, 1000, 10)] and nh == 200
        if n == 2:
            assert rounds[1] == [(5, 30, 1000 + off, 5000)]


def test_reduce_ties_go_to_the_lowest_tile_then_the_lowest_section():
    tiles = [_tile([[(3, 20, 5000, 1)], [(3, 50, 9000, 2)]]), _tile([[(3, 50, 100, 3)], [(3, 50, 3000, 4)]]), _tile([[(3, 50, 7000, 5)], []])]
    st, nh, rounds = otm.reduce_tiles_multi(tiles, W, 8, 4)
    # 50 four times: tile 0's (its section 1), then tile 1's section 0, then its section 1, then tile 2's; the 20 has no round left
    assert [r[0] for r in rounds] == [(3, 50, 9000, 2), (3, 50, 100, 3), (3, 50, 3000, 4), (3, 50, 7000, 5)]
    st, nh, rounds = otm.reduce_tiles_multi(tiles, W, 8, 5)
    assert rounds[4] == [(3, 20, 5000, 1)]


def test_reduce_a_partner_in_some_tiles_only():
    tiles = [_tile([[(2, 9, 500, 1)], []]), _tile([[], []], nh=7), _tile([[(2, 9, 500, 900), (4, 12, 800, 901)], [(4, 8, 3000, 950)]]), _tile([[(7, 6, 100, 2000)], []])]
    st, nh, rounds = otm.reduce_tiles_multi(tiles, W, 8, 3)
    assert st == 0 and nh == 307
    assert rounds == [[(2, 9, 500, 1), (4, 12, 800, 901), (7, 6, 100, 2000)], [(4, 8, 3000, 950)], []]
    assert otm.reduce_tiles_multi([_tile([[], []], nh=7, over=True)], W, 8, 2) == (oc.NONE, 7, [[], []])
    assert otm.reduce_tiles_multi(tiles[:1] + [_tile([[], []], nh=7, over=True)], W, 8, 2)[0] == oc.OVERFLOW


def test_reduce_sections_are_cut_on_their_own():
    """max_partners 1: section 0 keeps b = 1 and cuts b = 2; section 1 holds b = 2's second candidate - b = 1 has none - although
    section 0 cut b = 2."""
    tiles = [_tile([[(1, 9, 500, 1)], []]), _tile([[(2, 9, 600, 2)], []]), _tile([[(2, 8, 5000, 3)], []])]
    st, nh, rounds = otm.reduce_tiles_multi(tiles, W, 1, 2)
    assert st == oc.TRUNCATED and rounds == [[(1, 9, 500, 1)], [(2, 8, 5000, 3)]]
    # a tile row that was truncated: TRUNCATED without any cut here
    st, nh, rounds = otm.reduce_tiles_multi([_tile([[(1, 9, 500, 1)], []], st=oc.TRUNCATED)], W, 1, 2)
    assert st == oc.TRUNCATED and rounds == [[(1, 9, 500, 1)], []]


def test_reduce_one_round_is_reduce_tiles():
    import numpy as np
    rng = np.random.default_rng(6)
    for _ in range(50):
        tiles1, tilesm = [], []
        for t in range(int(rng.integers(1, 6))):
            bs = sorted(set(rng.integers(0, 6, size=int(rng.integers(0, 5))).tolist()))
            cands = [(b, int(rng.integers(6, 10)), int(rng.integers(0, 2000)), int(rng.integers(0, 9000))) for b in bs]
            over, st = bool(rng.integers(0, 2)), int(rng.choice([0, oc.TRUNCATED]))
            st = oc.NONE if not cands else st | (oc.OVERFLOW if over else 0)
            tiles1.append((st, 50, over, cands))
            tilesm.append((st, 50, over, [cands]))
        mp = int(rng.choice([1, 2, 8]))
        s1, h1, c1 = otc.reduce_tiles(tiles1, mp)
        sm, hm, cm = otm.reduce_tiles_multi(tilesm, W, mp, 1)
        assert (s1, h1, [c1]) == (sm, hm, cm)
