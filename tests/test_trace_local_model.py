"""`hinge paf2las --ends local` without a GPU: the numpy model of hinge_trace_local (tests/trace_local_common.py) against a textbook
Smith-Waterman and the tie rules spelled out, the properties a record must have, planted end points moved together and moved
independently (beside hinge_trace_refine's model on the same cases), unrelated pairs, a diagonal that is off by more than W, the
reference's own consensus program on a .las made of local traces; the command line's refusals before a GPU is needed."""
import os
import subprocess

import numpy as np
import pytest

import consensus_common as cc
import trace_common as tc
import trace_local_common as lc
import trace_refine_common as rc
from hinge_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")


# ---- (a) the whole matrix inside the band: a textbook Smith-Waterman, and the rules in their own words -----------------------------------
def _textbook(A, B, m, x):
    H = np.zeros((len(A) + 1, len(B) + 1), np.int64)
    for i in range(1, len(A) + 1):
        for j in range(1, len(B) + 1):
            H[i, j] = max(0, H[i - 1, j - 1] + (m if A[i - 1] == B[j - 1] else -x), H[i - 1, j] - x, H[i, j - 1] - x)
    return H


def _by_the_rules(A, B, m, x):
    """(score, kept columns front to back as (direction, i, j), start cell).  Best cell: the largest H; of equal ones the smallest
    i + j; of those the smallest i.  From it back while H > 0: the diagonal if it gives H, else the gap in B, else the gap in A."""
    H = _textbook(A, B, m, x)
    if H.max() == 0:
        return 0, [], None
    cells = [(i + j, i) for i in range(len(A) + 1) for j in range(len(B) + 1) if H[i, j] == H.max()]
    t, i = sorted(cells)[0]
    j = t - i
    cols = []
    while H[i, j] > 0:
        eq = A[i - 1] == B[j - 1]
        if H[i - 1, j - 1] + (m if eq else -x) == H[i, j]:
            cols.append((0 if eq else 3, i, j))
            i, j = i - 1, j - 1
        elif H[i - 1, j] - x == H[i, j]:
            cols.append((1, i, j))
            i -= 1
        else:
            assert H[i, j - 1] - x == H[i, j]
            cols.append((2, i, j))
            j -= 1
    return int(H.max()), cols[::-1], (i, j)


def _model_tiny(A, B, m, x):
    Ds, Cs, bests = lc.fill_local([(np.asarray(A, np.uint8), np.asarray(B, np.uint8))], 16, m, x)
    if bests[0][0] == 0:
        return 0, [], None
    kept, start = lc.kept_columns(Ds[0], Cs[0], bests[0], 16)
    return bests[0][0], [c[:3] for c in kept], start


def test_tiny_pairs_equal_textbook_smith_waterman_and_the_rules():
    unit = list(lc.TANDEM_UNIT)
    fixed = [(unit * 4, unit * 2, 1, 2),            # a tandem repeat: the score 6 at seven cells
             (unit * 4, unit * 2, 2, 3), (unit * 2, unit * 4, 1, 2), ([0] * 12, [0] * 5, 1, 2), ([0, 1] * 6, [1, 0] * 6, 1, 1),
             ([0, 0, 1, 0, 0], [0, 0, 0, 0], 1, 1),   # ties inside a cell: diagonal and gaps give the same
             ([0, 1, 2, 3], [3, 2, 1, 0], 1, 2), ([0], [1], 1, 2), ([2], [2], 1, 2)]
    H = _textbook(unit * 4, unit * 2, 1, 2)
    assert (H == H.max()).sum() >= 3 and _by_the_rules(unit * 4, unit * 2, 1, 2)[1][-1][1:] == (6, 6)       # of the equal maxima the first in (t, i)
    rng = np.random.default_rng(2)
    rand = []
    for _ in range(400):
        letters = int(rng.integers(2, 5))
        rand.append((rng.integers(0, letters, int(rng.integers(1, 13))).tolist(), rng.integers(0, letters, int(rng.integers(1, 13))).tolist()) + [(1, 2), (1, 1), (2, 3), (3, 1)][int(rng.integers(0, 4))])
    some_tie = 0
    for A, B, m, x in fixed + rand:
        want = _by_the_rules(A, B, m, x)
        assert _model_tiny(A, B, m, x) == want, (A, B, m, x)
        Hm = _textbook(A, B, m, x)
        some_tie += Hm.max() > 0 and (Hm == Hm.max()).sum() > 1
    assert some_tie > 50


def test_better_cell_rule_is_one_total_order():
    """The rule the reduction of the kernel applies pairwise, restated: sorting by it and folding with it agree."""
    def better(s, t, i, s0, t0, i0):
        return s > s0 or (s == s0 and (t < t0 or (t == t0 and i < i0)))
    rng = np.random.default_rng(8)
    for _ in range(200):
        cells = [(int(rng.integers(0, 4)), int(rng.integers(0, 6)), int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 20)))]
        cur = cells[0]
        for c in cells[1:]:
            if better(*c, *cur):
                cur = c
        assert cur == sorted(cells, key=lambda c: (-c[0], c[1], c[2]))[0]


# ---- the hand cases ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    contigs, reads, pl, calls = lc.hand_cases()
    res, stats = {}, {}
    for label, names, kw in calls:
        stats[label] = {}
        res[label] = lc.model_local(contigs, reads, [pl[n] for n in names], stats=stats[label], **kw)
    return contigs, reads, pl, calls, res, stats


def _check_record(contigs, reads, p, r, tspace, match, min_score):
    st, w, ends, tr, df, sc = r
    ab, ae, bb, be = ends
    assert ab < ae and bb < be
    assert sum(tr[1::2]) == be - bb
    assert len(tr) == 2 * tc.n_segments(ab, ae, tspace)
    assert sum(tr[0::2]) == df
    A, B = tc.stretches(contigs, reads, (p[0], p[1], p[2], ab, ae, bb, be))
    assert df >= tc.levenshtein(A, B)
    assert A[0] == B[0] and A[-1] == B[-1]          # the first and the last kept column are matches
    a0, b0 = ab, bb
    for s in range(len(tr) // 2):
        a1 = min((ab // tspace + s + 1) * tspace, ae)
        seg_a, seg_b = tc.stretches(contigs, reads, (p[0], p[1], p[2], a0, a1, b0, b0 + tr[2 * s + 1]))
        assert tr[2 * s] >= tc.levenshtein(seg_a, seg_b)
        a0, b0 = a1, b0 + tr[2 * s + 1]
    assert max(1, min_score) <= sc <= match * min(ae - ab, be - bb)


def test_invariants_on_every_record(hand):
    contigs, reads, pl, calls, res, stats = hand
    n = 0
    for label, names, kw in calls:
        for name, r in zip(names, res[label]):
            if r[0] == tc.OK:
                _check_record(contigs, reads, pl[name], r, kw["tspace"], kw.get("match", 1), kw.get("min_score", lc.MIN_SCORE))
                n += 1
            else:
                assert r[2] is None and r[3] is None and r[4] == 0 and r[5] == 0
    assert n >= 25


def test_hand_cases_are_what_they_are_named(hand):
    contigs, reads, pl, calls, res, stats = hand
    by = {label: dict(zip(names, res[label])) for label, names, kw in calls}
    d = by["w64"]
    # all four end points moved independently, both strands: back within a few bases of the planted ones
    assert d["plain"][:2] == (tc.OK, 64) and max(abs(a - b) for a, b in zip(d["plain"][2][:2], (300, 600))) <= 10
    assert d["plain_comp"][0] == tc.OK and pl["plain_comp"][2] == 1 and max(abs(a - b) for a, b in zip(d["plain_comp"][2][:2], (700, 1100))) <= 25
    # the alignment begins in row 0 / in column 0 of its box
    assert d["row0"][0] == tc.OK and d["row0"][2][0] == 0 and d["row0"][2][2] > lc.widen(pl["row0"], 300, len(reads[pl["row0"][1]]), 50)[5]
    assert d["col0"][0] == tc.OK and d["col0"][2][2] == 0 and d["col0"][2][0] > lc.widen(pl["col0"], 3000, len(reads[pl["col0"][1]]), 50)[3]
    # the start cell one diagonal outside the band: the walk ends there without reading a direction; the first kept column lies
    # on the band's last diagonal, so the placement is TOUCHED at W = 8 and a record at 16
    A, B = tc.stretches(contigs, reads, pl["outside_start"])
    Ds, Cs, bests = lc.fill_local([(A, B)], 8)
    kept, start = lc.kept_columns(Ds[0], Cs[0], bests[0], 8)
    assert start == (12, 20) and start[1] - start[0] - int(Cs[0][12]) + 8 == 16 and kept[0][1:] == (13, 21, 15) and bests[0] == (188, 200, 208)
    assert by["outside_w8"]["outside_start"][:2] == (tc.TOUCHED, 8) and by["outside_w8"]["identical"][:2] == (tc.OK, 8)
    o = by["outside_w8_64"]["outside_start"]
    assert o[:2] == (tc.OK, 16) and o[2][1::2] == (300, 208) and 100 <= o[2][0] <= 112 and o[2][2] - o[2][0] == -92 and o[5] >= 188     # (at 16 the front is inside the band: a chance match may extend it)
    # the tandem repeat: |blen - alen| = 60 runs at W = 64 from the start; ten units against the first ten of thirty
    assert d["tandem"][:2] == (tc.OK, 64) and d["tandem"][2] == (50, 80, 0, 30) and d["tandem"][5] == 30 and by["w8"]["tandem"][:2] == (tc.OK, 64)
    # unrelated: EMPTY after every round
    assert d["unrelated"][:2] == (lc.EMPTY, 256) and by["last_w64"]["unrelated"][:2] == (lc.EMPTY, 64)
    assert by["min_score_1"]["unrelated"][0] in (tc.OK, tc.TOUCHED)                  # (what the default min_score is there to prevent)
    # the diagonal 90 beside the centre line: EMPTY at 64, found at 128; EMPTY when 64 is the last W
    od = pl["off_diagonal"]
    box = lc.widen(od, 3000, len(reads[od[1]]), 50)
    assert lc.local_round([tc.stretches(contigs, reads, box)], [box[3]], 100, 64)[0][0] == lc.EMPTY
    assert d["off_diagonal"][:2] == (tc.OK, 128) and abs(d["off_diagonal"][2][0] - 2400) <= 10 and abs(d["off_diagonal"][2][2] - 90) <= 10
    assert by["last_w64"]["off_diagonal"][:2] == (lc.EMPTY, 64) and by["last_w64"]["plain"] == d["plain"]
    assert stats["w64"]["empty_widened"] == 3 and stats["last_w64"]["empty_widened"] == 0         # off_diagonal once, unrelated twice
    # an identical stretch without room is hinge_trace_run's record
    plain = tc.model_run(contigs, reads, [pl["identical"]], 100, 64, 1024)[0]
    assert d["identical"] == (tc.OK, 64, (1000, 1300, 0, 300), plain[2], 0, 300) and plain[0] == tc.OK
    ic = d["identical_comp"]                                                          # (chance matches in the flanks may extend it by a few bases)
    assert ic[:2] == (tc.OK, 64) and pl["identical_comp"][2] == 1 and max(abs(a - b) for a, b in zip(ic[2], (1150, 1400, 30, 280))) <= 10 and ic[5] >= 250
    # W = 8 as the first band: every status there is, records among them
    assert {r[0] for r in by["w8"].values()} >= {tc.OK, lc.EMPTY} and by["w8"]["identical"][:2] == (tc.OK, 8)
    assert all(r[0] in (tc.OK, lc.EMPTY) for r in by["two_byte"].values())


# ---- (b), (c), (d) planted end points ---------------------------------------------------------------------------------------------------
# 200 seeded cases per regime and error rate, alen 200-500, W 64, E 50, scores 1 / 2; the largest miss of a planted end point over the
# four end points of every case (pytest -s prints them again).
#   moved together (trace_refine_common.REGIMES; band_max 64):     6 % errors: exact 19, out60 22, in40 10, asym 14
#                                                                  15 % errors: exact 27, out60 23, in40 14, asym 17
#   moved independently by -80 .. +80 each (band_max 512: A's and B's lengths differ by up to 320):   6 %: 34;   15 %: 36
# Bound = the largest of a rate's figures plus half of it.  The planted end point is the truth; the model is what is measured.
D_BOUND = {("together", 0.06): 22 + 11, ("together", 0.15): 27 + 13, ("independent", 0.06): 34 + 17, ("independent", 0.15): 36 + 18}
TSPACE = 100
assert max(D_BOUND.values()) <= TSPACE


def _misses(res, truths):
    return [max(abs(g - t) for g, t in zip(r[2], truth)) for r, truth in zip(res, truths) if r[0] == tc.OK]


@pytest.fixture(scope="module")
def sweep():
    out = {}
    for err in (0.06, 0.15):
        for regime, (d0, d1) in rc.REGIMES.items():
            rng = np.random.default_rng([int(err * 100), sorted(rc.REGIMES).index(regime)])          # test_trace_refine_model.py's cases
            contigs, reads, pls, truths = [], [], [], []
            for x in range(200):
                contig, read, given, truth = lc.planted(rng, int(rng.integers(200, 501)), err, d0, d1)
                contigs.append(contig); reads.append(read); truths.append(truth)
                pls.append((x, x) + given[2:])
            out[("together", err, regime)] = (lc.model_local(contigs, reads, pls, TSPACE, 64, 64, extend=50), truths)
        rng = np.random.default_rng([int(err * 100), 99])
        contigs, reads, pls, truths = [], [], [], []
        for x in range(200):
            contig, read, given, truth = lc.planted_independent(rng, int(rng.integers(200, 501)), err, 80)
            contigs.append(contig); reads.append(read); truths.append(truth)
            pls.append((x, x) + given[2:])
        out[("independent", err, "local")] = (lc.model_local(contigs, reads, pls, TSPACE, 64, 512, extend=50), truths)
        out[("independent", err, "refine")] = (rc.model_refine(contigs, reads, pls, TSPACE, 64, 512, extend=50), truths)
    return out


@pytest.mark.parametrize("err", [0.06, 0.15])
def test_planted_end_points_moved_together_are_found(sweep, err):
    worst = {}
    for regime in rc.REGIMES:
        res, truths = sweep[("together", err, regime)]
        assert all(r[0] == tc.OK for r in res), regime                     # none EMPTY at the default min_score, none dropped
        worst[regime] = max(_misses(res, truths))
    print("planted sweep, moved together, %.0f %% errors: largest miss per regime %s (bound %d)" % (err * 100, worst, D_BOUND[("together", err)]))
    assert max(worst.values()) < D_BOUND[("together", err)], worst


@pytest.mark.parametrize("err", [0.06, 0.15])
def test_planted_end_points_moved_independently_are_found(sweep, err):
    res, truths = sweep[("independent", err, "local")]
    assert all(r[0] == tc.OK for r in res)                                  # none EMPTY, none dropped
    miss = _misses(res, truths)
    print("planted sweep, moved independently, %.0f %% errors: largest miss %d, median %.1f (bound %d); final W %s" % (
        err * 100, max(miss), float(np.median(miss)), D_BOUND[("independent", err)], sorted({r[1] for r in res})))
    assert max(miss) < D_BOUND[("independent", err)]


@pytest.mark.parametrize("err", [0.06, 0.15])
def test_local_beats_refine_on_independently_moved_end_points(sweep, err):
    """(c) the acceptance condition: on the same cases the median miss of the local model is below that of model_refine."""
    loc, truths = sweep[("independent", err, "local")]
    ref, _ = sweep[("independent", err, "refine")]
    ml, mr = _misses(loc, truths), _misses(ref, truths)
    print("moved independently, %.0f %% errors: local median %.1f worst %d over %d records; refine median %.1f worst %d over %d" % (
        err * 100, float(np.median(ml)), max(ml), len(ml), float(np.median(mr)), max(mr), len(mr)))
    assert len(ml) >= len(mr) and np.median(ml) < np.median(mr)


def test_unrelated_pairs_are_empty_at_the_default_min_score():
    """(d) 40 pairs of 400 bases and 8 of 1000, through every round up to W = 512; the planted cases above are never EMPTY."""
    rng = np.random.default_rng(9)
    contigs = [rng.integers(0, 4, size=400, dtype=np.uint8) for _ in range(40)] + [rng.integers(0, 4, size=1000, dtype=np.uint8) for _ in range(8)]
    reads = [rng.integers(0, 4, size=len(c), dtype=np.uint8) for c in contigs]
    pls = [(x, x, x % 2, 50, len(c) - 50, 50, len(c) - 50) for x, c in enumerate(contigs)]
    st = {}
    res = lc.model_local(contigs, reads, pls, TSPACE, 64, 512, extend=50, stats=st)
    assert all(r[0] == lc.EMPTY and r[1] == 512 for r in res) and st == dict(empty_widened=3 * 48, rounds=4)
    assert lc.MIN_SCORE == 24


# ---- (e) a diagonal off by more than W ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("err,off", [(0.06, 80), (0.15, -100), (0.15, 120)])
def test_diagonal_off_by_more_than_w(err, off):
    rng = np.random.default_rng([3, abs(off)])
    contig, read, given, truth = lc.planted(rng, 400, err, 0, 0, flank=300)
    g = lc.beside(truth, off)                                                         # the planted alignment whole inside the box
    box = lc.widen(g, len(contig), len(read), 50)
    assert lc.local_round([tc.stretches([contig], [read], box)], [box[3]], TSPACE, 64)[0][0] in (lc.EMPTY, tc.TOUCHED)      # at W
    assert lc.model_local([contig], [read], [g], TSPACE, 64, 64)[0][:2] == (lc.EMPTY, 64)                                   # band_max = W
    st = {}
    r = lc.model_local([contig], [read], [g], TSPACE, 64, 128, stats=st)[0]                                                 # 2 W
    assert r[:2] == (tc.OK, 128) and st == dict(empty_widened=1, rounds=2)
    assert max(abs(a - b) for a, b in zip(r[2], truth)) < D_BOUND[("together", err)]


# ---- the reference's own consensus on local traces ------------------------------------------------------------------------------------------
def test_reference_consensus_accepts_local_traces(oracle_lib, tmp_path):
    from hinge_amd import synth_consensus as sc
    d, pls = lc.perturbed_cns_tiny()
    ts = d.spec.tspace
    res = lc.model_local(d.contigs, d.reads, pls, ts, 128, 1024)
    assert all(r[0] == tc.OK for r in res)                                 # no placement EMPTY or dropped
    far = [max(abs(r[2][k] - int(q[n])) for k, n in enumerate(("abpos", "aepos", "bbpos", "bepos"))) for r, q in zip(res, d.rec)]
    print("local end points of cns_tiny (moved by up to 60) vs the generator's: largest distance %d, median %.1f" % (max(far), float(np.median(far))))
    wd = str(tmp_path)
    sc.write_dataset(d, wd)
    rec = np.zeros(len(res), dtype=formats.LAS_REC_DTYPE)
    tb = 1 if ts <= 125 else 2
    pieces = []
    for k, (p, r) in enumerate(zip(pls, res)):
        rec[k]["aread"], rec[k]["bread"], rec[k]["flags"] = p[0], p[1], p[2]
        rec[k]["abpos"], rec[k]["aepos"], rec[k]["bbpos"], rec[k]["bepos"] = r[2]
        rec[k]["tlen"], rec[k]["diffs"] = len(r[3]), r[4]
        pieces.append(np.asarray(r[3], np.uint8) if tb == 1 else np.asarray(r[3], "<u2").view(np.uint8))
    order = np.lexsort((rec["abpos"], rec["bread"], rec["aread"]))
    pieces = [pieces[k] for k in order]
    formats.write_las(os.path.join(wd, "draft.reads.las"), formats.LasRecords(ts, rec[order], np.concatenate(pieces), np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)))
    fasta, log = cc.run_oracle(oracle_lib, wd)
    assert fasta.count(b">Consensus") == len(d.contigs)
    ref = cc.run_reference(wd)
    if ref is not None:                                                     # live: the reference binary itself, same files
        assert ref[0] == fasta and ref[1] == log


# ---- (f) the command line, before a GPU is needed -----------------------------------------------------------------------------------------
def test_paf2las_ends_local_usage():
    for opts, what in ((["--ends", "sometimes"], b"--ends takes given or refine or local"), (["--extend", "20"], b"belong to --ends refine and --ends local"),
                       (["--ends", "local", "--scores", "3"], b"--scores needs M,X"), (["--ends", "local", "--min-score", "0"], b"usage: paf2las"),
                       (["--ends", "given", "--min-score", "5"], b"belong to --ends refine and --ends local"), (["--ends", "local", "--extend", "-1"], b"usage: paf2las")):
        r = subprocess.run([HINGE, "paf2las", "draft", "reads", "x.paf", "out.las"] + opts, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and what in r.stderr and b"usage: paf2las" in r.stderr and b"--ends given|refine|local" in r.stderr, (opts, r.stderr)
