"""`hinge paf2las --ends refine` without a GPU: the numpy model of hinge_trace_refine (tests/trace_refine_common.py) against the
tie rule, the properties a refined record must have, planted end points, and the reference's own consensus program on a .las made
of refined traces; the command line's new options where they are refused before a GPU is needed."""
import os
import subprocess

import numpy as np
import pytest

import consensus_common as cc
import trace_common as tc
import trace_refine_common as rc
from hinge_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")


# ---- the tie rule -----------------------------------------------------------------------------------------------------------------------
def _brute(scores):
    """Every run, in the rule's words: the largest sum; of equal sums the latest start; of those the latest end."""
    best = None
    for s in range(len(scores)):
        for e in range(s, len(scores)):
            key = (sum(scores[s:e + 1]), s, e)
            if best is None or key > best:
                best = key
    return best


def test_tie_rule_on_hand_built_columns():
    # equal sums at two starts: the latest start
    assert rc.best_run([1, -2, 1]) == (1, 2, 2)
    assert rc.best_run([1, 1, -2, 1, 1]) == (2, 3, 4)
    assert rc.best_run([1, 1, -2, -2, 1, -2, 1, 1]) == (2, 6, 7)
    # equal sums at two ends of one start: the latest end
    assert rc.best_run([1, 1, 1, -1, 1]) == (3, 0, 4)
    assert rc.best_run([2, -2, 2, -2]) == (2, 2, 2)
    assert rc.best_run([1, 1, -2, 1, 1, -2, 1, 1]) == (2, 6, 7)
    assert rc.best_run([3, 3, -3, 3, -3, 3]) == (6, 0, 5)            # ends at 1, at 3 and at 5 all give 6: the latest
    # both at once, and nothing to keep
    assert rc.best_run([1, -1, 1, -1, 1]) == (1, 4, 4)
    assert rc.best_run([-2, -2]) == (-2, 1, 1) and rc.best_run([]) == (0, -1, -1)
    rng = np.random.default_rng(1)
    for _ in range(300):
        m, x = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        sc = [m if v else -x for v in rng.integers(0, 2, size=int(rng.integers(1, 14)))]
        assert rc.best_run(sc) == _brute(sc), sc


def _cols(dirs, W=8):
    """Columns of a path given as directions front to back (all on the centre diagonal's k: no band is involved)."""
    out, i, j = [], 0, 0
    for d in dirs:
        i, j = i + (d != 2), j + (d != 1)
        out.append((d, i, j, W))
    return out


def test_clip_of_hand_built_paths():
    # 3 matches, a substitution, 1 match | kept: the first three (sum 3; with the tail 3 - 2 + 1 = 2)
    st, cells, tr, df, sc = rc.clip(_cols([0, 0, 0, 3, 0]), 0, 100, 8)
    assert (st, cells, tr, df, sc) == (tc.OK, (0, 0, 3, 3), [0, 3], 0, 3)
    # equal sums at two starts (2 | 2): the later run, which lies in the second block of A when the box starts at 97
    st, cells, tr, df, sc = rc.clip(_cols([0, 0, 1, 0, 0]), 97, 100, 8)
    assert (st, cells, tr, df, sc) == (tc.OK, (3, 2, 5, 4), [0, 2], 0, 2)
    # a gap in A inside the kept run belongs to the block of the A base in front of it
    st, cells, tr, df, sc = rc.clip(_cols([0, 0, 0, 2, 0, 0, 0]), 97, 100, 8)
    assert (st, cells, tr, df, sc) == (tc.OK, (0, 0, 6, 7), [1, 4, 0, 3], 1, 4)
    # nothing reaches the minimum score
    assert rc.clip(_cols([0, 0, 3, 0]), 0, 100, 8, min_score=3)[0] == rc.EMPTY
    assert rc.clip(_cols([3, 1, 2]), 0, 100, 8)[0] == rc.EMPTY
    # touched counts on kept columns only
    edge = _cols([0, 0, 0, 3, 3])
    edge[4] = (3, 5, 5, 0)
    assert rc.clip(edge, 0, 100, 8)[0] == tc.OK
    edge[1] = (0, 2, 2, 15)
    assert rc.clip(edge, 0, 100, 8)[0] == tc.TOUCHED


# ---- the hand cases ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    contigs, reads, pl, calls = rc.hand_cases()
    res = {label: rc.model_refine(contigs, reads, [pl[n] for n in names], **kw) for label, names, kw in calls}
    return contigs, reads, pl, calls, res


def _check_record(contigs, reads, p, r, tspace, extend, match, diff):
    st, w, ends, tr, df, sc = r
    ab, ae, bb, be = ends
    assert ab < ae and bb < be
    assert sum(tr[1::2]) == be - bb
    assert len(tr) == 2 * tc.n_segments(ab, ae, tspace)
    assert sum(tr[0::2]) == df
    A, B = tc.stretches(contigs, reads, (p[0], p[1], p[2], ab, ae, bb, be))
    assert df >= tc.levenshtein(A, B)
    # score = match x matches - diff x diffs, the matches counted on the kept columns of the box's own path at the final W
    box = rc.widen(p, len(contigs[p[0]]), len(reads[p[1]]), extend)
    bA, bB = tc.stretches(contigs, reads, box)
    Ds, Cs, end = tc._fill([(bA, bB)], w)
    cols = rc.columns(Ds[0], Cs[0], len(bA), len(bB), w)
    cells = [(0, 0)] + [(c[1], c[2]) for c in cols]
    lo, hi = cells.index((ab - box[3], bb - box[5])), cells.index((ae - box[3], be - box[5]))
    kept = cols[lo:hi]
    matches = sum(c[0] == 0 for c in kept)
    assert len(kept) - matches == df and sc == match * matches - diff * df
    assert kept[0][0] == 0 and kept[-1][0] == 0
    assert A[0] == B[0] and A[-1] == B[-1]          # the first and the last kept column are matches
    a0, b0 = ab, bb
    for s in range(len(tr) // 2):
        a1 = min((ab // tspace + s + 1) * tspace, ae)
        seg_a, seg_b = tc.stretches(contigs, reads, (p[0], p[1], p[2], a0, a1, b0, b0 + tr[2 * s + 1]))
        assert tr[2 * s] >= tc.levenshtein(seg_a, seg_b)
        a0, b0 = a1, b0 + tr[2 * s + 1]


def test_invariants_on_every_record(hand):
    contigs, reads, pl, calls, res = hand
    n = 0
    for label, names, kw in calls:
        for name, r in zip(names, res[label]):
            if r[0] == tc.OK:
                _check_record(contigs, reads, pl[name], r, kw["tspace"], kw.get("extend", 50), kw.get("match", 1), kw.get("diff", 2))
                n += 1
            else:
                assert r[2] is None and r[3] is None and r[4] == 0 and r[5] == 0
    assert n >= 30


def test_score_is_matches_minus_diffs():
    """score = M x matches - X x diffs, counted on the kept columns themselves."""
    rng = np.random.default_rng(4)
    for _ in range(12):
        contig, read, given, truth = rc.planted(rng, int(rng.integers(60, 160)), 0.1, 20, -15, flank=80)
        box = rc.widen(given, len(contig), len(read), 30)
        A, B = tc.stretches([contig], [read], box)
        Ds, Cs, end = tc._fill([(A, B)], 32)
        cols = rc.columns(Ds[0], Cs[0], len(A), len(B), 32)
        for m, x in ((1, 2), (2, 3), (15, 1)):
            best, s, e = rc.best_run([m if c[0] == 0 else -x for c in cols])
            st, cells, tr, df, sc = rc.clip(cols, box[3], 100, 32, m, x)
            if st == tc.OK:
                kept = cols[s:e + 1]
                matches = sum(c[0] == 0 for c in kept)
                assert sc == best == m * matches - x * df and df == len(kept) - matches
                assert kept[0][0] == 0 and kept[-1][0] == 0


def test_hand_cases_are_what_they_are_named(hand):
    contigs, reads, pl, calls, res = hand
    by = {label: dict(zip(names, res[label])) for label, names, kw in calls}
    d = by["defaults_w64"]
    # 1: begins exactly on a trace-point boundary (the back is where the global path leaves the equal stretch: within a few bases of 500)
    assert d["boundary"][:2] == (tc.OK, 64) and d["boundary"][2][0] == 300 and 490 <= d["boundary"][2][1] <= 510
    assert d["one_segment"][0] == tc.OK and 600 <= d["one_segment"][2][0] < d["one_segment"][2][1] <= 700 and len(d["one_segment"][3]) == 2     # 3: one segment, not the box's first
    assert rc.widen(pl["one_segment"], 3000, len(reads[pl["one_segment"][1]]), 50)[3:5] == (540, 760)
    e5 = by["extend_5"]["first_segment"]
    assert rc.widen(pl["first_segment"], 3000, len(reads[pl["first_segment"][1]]), 5)[3:5] == (400, 460)
    assert e5[0] == tc.OK and 400 <= e5[2][0] < e5[2][1] <= 460 and len(e5[3]) == 2           # 2: inside the box's first segment
    # 4: clamped by a sequence start on either strand, and by the contig's end
    assert rc.widen(pl["clamp_front"], 3000, len(reads[pl["clamp_front"][1]]), 50)[3:7] == (6, 270, 0, pl["clamp_front"][6] + 50)
    cc_ = pl["clamp_comp"]
    assert cc_[2] == 1 and rc.widen(cc_, 3000, len(reads[cc_[1]]), 50)[3:7] == (797, 1050, 0, cc_[6] + 50)
    assert rc.widen(pl["clamp_back"], 300, len(reads[pl["clamp_back"][1]]), 50)[4] == 300
    assert all(d[n][0] == tc.OK for n in ("clamp_front", "clamp_comp", "clamp_back", "undershoot", "overshoot_comp"))
    assert abs(d["undershoot"][2][0] - 1800) <= 10 and abs(d["undershoot"][2][1] - 2200) <= 10        # 40 bases won back per end
    assert abs(d["overshoot_comp"][2][0] - 2300) <= 30 and abs(d["overshoot_comp"][2][1] - 2700) <= 30
    # 5: extend 0 never leaves the given box
    for name, r in by["extend_0"].items():
        if r[0] == tc.OK:
            assert pl[name][3] <= r[2][0] and r[2][1] <= pl[name][4] and pl[name][5] <= r[2][2] and r[2][3] <= pl[name][6]
    # 6: an identical stretch without room is hinge_trace_run's record
    plain = tc.model_run(contigs, reads, [pl["identical"]], 100, 64, 1024)[0]
    assert d["identical"] == (tc.OK, 64, (1000, 1300, 0, 300), plain[2], 0, 300) and plain[0] == tc.OK
    # 7: noise is EMPTY at min_score 40, its neighbours keep their records
    n40 = by["noise_min_score_40"]
    assert n40["noise"][0] == rc.EMPTY and n40["undershoot"] == d["undershoot"] and n40["boundary"] == d["boundary"]
    # 8: the tail that touches the band's first diagonal is clipped: OK at the first W, where hinge_trace_run widens
    t = by["tail_touch"]["tail_touch"]
    assert t[:2] == (tc.OK, 16) and t[2][0] == 2600 and 2790 <= t[2][1] < 2816            # (the shifted 150 bases begin at 2816)
    assert tc.model_run(contigs, reads, [pl["tail_touch"]], 100, 16, 1024)[0][1] > 16
    # a kept column on the band's last diagonal does widen
    k = by["touch_kept"]["touch_kept"]
    assert k[:2] == (tc.OK, 32) and k[4] == 30 and rc.refine_round([tc.stretches(contigs, reads, pl["touch_kept"])], [60], 100, 16)[0][0] == tc.TOUCHED
    # 9: kept across 300 inserted bases (a match outweighs fifteen diffs): the segment's B advance does not fit a byte
    assert by["wide"]["wide"][:2] == (tc.WIDE, 512) and by["wide"]["identical"][0] == tc.OK
    # 10: two-byte traces, from W 16
    assert all(r[0] in (tc.OK, rc.EMPTY) for r in by["two_byte_w16"].values())


# ---- planted end points -----------------------------------------------------------------------------------------------------------------
# The sweep below (200 seeded cases per regime and error rate, alen 200-500, W 64, E 50, scores 1 / 2) printed, as the largest miss
# of a planted end point over the four end points of every case (pytest -s prints them again):
#    6 % errors: exact 19, out60 22, in40 10, asym 19
#   15 % errors: exact 27, out60 25, in40 26, asym 18
# D = the largest of a rate's four, plus half of it.  The planted end point is the truth; the model is what is measured.
D_BOUND = {0.06: 22 + 11, 0.15: 27 + 13}
TSPACE = 100


@pytest.fixture(scope="module")
def sweep():
    out = {}
    for err in (0.06, 0.15):
        for regime, (d0, d1) in rc.REGIMES.items():
            rng = np.random.default_rng([int(err * 100), sorted(rc.REGIMES).index(regime)])
            contigs, reads, pls, truths = [], [], [], []
            for x in range(200):
                contig, read, given, truth = rc.planted(rng, int(rng.integers(200, 501)), err, d0, d1)
                contigs.append(contig); reads.append(read); truths.append(truth)
                pls.append((x, x) + given[2:])
            res = rc.model_refine(contigs, reads, pls, TSPACE, 64, 64, extend=50)
            out[(err, regime)] = (res, truths)
    return out


@pytest.mark.parametrize("err", [0.06, 0.15])
def test_planted_end_points_are_found(sweep, err):
    worst = {}
    for regime in rc.REGIMES:
        res, truths = sweep[(err, regime)]
        assert all(r[0] == tc.OK for r in res), regime                     # none EMPTY, none dropped
        worst[regime] = max(max(abs(g - t) for g, t in zip((r[2][0], r[2][1], r[2][2], r[2][3]), truth)) for r, truth in zip(res, truths))
    print("planted sweep, %.0f %% errors: largest miss per regime %s (bound %d)" % (err * 100, worst, D_BOUND[err]))
    if err == 0.06:
        assert max(worst.values()) <= TSPACE // 2, "the default scores do not find 6 % alignments' ends"
    assert max(worst.values()) < D_BOUND[err], worst


def test_unrelated_pairs_are_empty():
    rng = np.random.default_rng(9)
    contigs = [rng.integers(0, 4, size=400, dtype=np.uint8) for _ in range(40)]
    reads = [rng.integers(0, 4, size=400, dtype=np.uint8) for _ in range(40)]
    pls = [(x, x, x % 2, 50, 350, 50, 350) for x in range(40)]
    res = rc.model_refine(contigs, reads, pls, TSPACE, 64, 64, extend=50, min_score=40)
    assert all(r[0] == rc.EMPTY and r[1] == 64 for r in res)


# ---- the reference's own consensus on refined traces -----------------------------------------------------------------------------------------
def test_reference_consensus_accepts_refined_traces(oracle_lib, tmp_path):
    from hinge_amd import synth_consensus as sc
    d, pls = rc.perturbed_cns_tiny()
    ts = d.spec.tspace
    res = rc.model_refine(d.contigs, d.reads, pls, ts, 128, 1024)
    assert all(r[0] == tc.OK for r in res)                                 # no placement clipped out or dropped
    moved = [abs(r[2][0] - int(q["abpos"])) for r, q in zip(res, d.rec)] + [abs(r[2][1] - int(q["aepos"])) for r, q in zip(res, d.rec)]
    print("refined A end points of cns_tiny vs the generator's: largest distance %d, mean %.1f" % (max(moved), sum(moved) / len(moved)))
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


# ---- the command line, before a GPU is needed ---------------------------------------------------------------------------------------------
def test_paf2las_ends_options_usage():
    for opts, what in ((["--ends", "sometimes"], b"--ends takes given or refine"), (["--extend", "20"], b"belong to --ends refine"),
                       (["--ends", "refine", "--scores", "3"], b"--scores needs M,X"), (["--ends", "given", "--min-score", "5"], b"belong to --ends refine")):
        r = subprocess.run([HINGE, "paf2las", "draft", "reads", "x.paf", "out.las"] + opts, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and what in r.stderr and b"usage: paf2las" in r.stderr, (opts, r.stderr)
