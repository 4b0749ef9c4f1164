"""Shared by the `hinge paf2las --ends refine` tests: the numpy model behind hinge_trace_refine ("Refined end
points"), on top of tests/trace_common.py's band fill.  Written from the rule, over forward arrays, not from the kernel's backward
scan:

  the box is widened per side by e = min(extend, room on A, room on B) (B in its strand frame), the band is filled as for
  hinge_trace_run, and the path from (0, 0) to (alen, blen) is read as a list of COLUMNS (one per step; a column lies on the
  band cell it ends in).  A column scores +match on equal bases and -diff otherwise.  Kept: the contiguous run of columns with
  the largest sum; among equal sums the run that starts latest, among those the one that ends latest.  Below max(1, min_score):
  EMPTY.  TOUCHED only when a kept column lies on the band's first or last diagonal.
"""
import numpy as np

import trace_common as tc

EMPTY = 5


def widen(p, alen_whole, blen_whole, extend):
    """The widened box of placement p = (aread, bread, comp, abpos, aepos, bbpos, bepos): both sequences get the same amount per
    side; B's room is measured in the frame its coordinates are in (the complemented one when comp)."""
    a, b, comp, ab, ae, bb, be = [int(v) for v in p]
    e0 = min(extend, ab, bb)
    e1 = min(extend, alen_whole - ae, blen_whole - be)
    return (a, b, comp, ab - e0, ae + e1, bb - e0, be + e1)


def columns(D, C, alen, blen, W):
    """The path's columns front to back: rows of (direction, i, j, k) with (i, j) the cell the column ends in."""
    out = []
    i, j = alen, blen
    for _ in range(alen + blen + 1):
        if i == 0 and j == 0:
            break
        k = j - i - int(C[i]) + W
        d = 2 if i == 0 else int(D[i, k])
        assert d != 255
        out.append((d, i, j, k))
        if d in (0, 3):
            i, j = i - 1, j - 1
        elif d == 1:
            i -= 1
        else:
            j -= 1
    assert i == 0 and j == 0
    return out[::-1]


def best_run(scores):
    """(sum, first, last) of the kept run of a list of column scores (last inclusive), or (0, -1, -1) for an empty list."""
    n = len(scores)
    if n == 0:
        return 0, -1, -1
    P = np.concatenate([[0], np.cumsum(np.asarray(scores, np.int64))])       # P[x] = sum of the first x columns
    after = np.maximum.accumulate(P[:0:-1])[::-1]                              # after[s] = max P[s + 1 ..]: the best end for a start at s
    sums = after - P[:-1]
    best = int(sums.max())
    s = int(np.flatnonzero(sums == best)[-1])                                  # the latest start ...
    e = int(np.flatnonzero(P[s + 1:] == after[s])[-1]) + s                     # ... and its latest end
    return best, s, e


def clip(cols, wab, tspace, W, match=1, diff=2, min_score=1):
    """(status, (i0, j0, i1, j1) or None, trace or None, diffs, score) of one filled box whose path has the columns cols."""
    best, s, e = best_run([match if c[0] == 0 else -diff for c in cols])
    if best < max(1, min_score):
        return EMPTY, None, None, 0, 0
    kept = cols[s:e + 1]
    i1, j1 = kept[-1][1], kept[-1][2]
    d0, i0, j0, _ = kept[0]
    i0, j0 = i0 - (d0 != 2), j0 - (d0 != 1)
    first = (wab + i0) // tspace
    nseg = tc.n_segments(wab + i0, wab + i1, tspace)
    sd, sb = [0] * nseg, [0] * nseg
    for d, i, j, k in kept:
        g = (wab + i - 1) // tspace - first
        sd[g] += d != 0
        sb[g] += d != 1
    touched = any(c[3] == 0 or c[3] == 2 * W - 1 for c in kept)
    tmax = tc.trace_max(tspace)
    wide = max(sd) > tmax or max(sb) > tmax
    st = tc.TOUCHED if touched else tc.WIDE if wide else tc.OK
    if st != tc.OK:
        return st, None, None, 0, 0
    return st, (i0, j0, i1, j1), [int(v) for pr in zip(sd, sb) for v in pr], int(sum(sd)), best


def refine_round(pairs, wabs, tspace, W, match=1, diff=2, min_score=1, chunk=32):
    """One round at W over widened boxes: per pair what clip() answers (NO_PATH from the lengths or an unreached end cell)."""
    out = [None] * len(pairs)
    todo = []
    for x, (a, b) in enumerate(pairs):
        if abs(len(b) - len(a)) > W:
            out[x] = (tc.NO_PATH, None, None, 0, 0)
        else:
            todo.append(x)
    todo.sort(key=lambda x: len(pairs[x][0]))
    for c0 in range(0, len(todo), chunk):
        xs = todo[c0:c0 + chunk]
        Ds, Cs, end = tc._fill([pairs[x] for x in xs], W)
        for x, D, C, e in zip(xs, Ds, Cs, end):
            if e >= tc.INF:
                out[x] = (tc.NO_PATH, None, None, 0, 0)
                continue
            cols = columns(D, C, len(pairs[x][0]), len(pairs[x][1]), W)
            assert sum(c[0] != 0 for c in cols) == e
            out[x] = clip(cols, wabs[x], tspace, W, match, diff, min_score)
    return out


def model_refine(contigs, reads, placements, tspace, band=128, band_max=1024, extend=50, match=1, diff=2, min_score=1):
    """What hinge_trace_refine answers: per placement (status, final W, (abpos', aepos', bbpos', bepos') or None, trace or None,
    diffs, score)."""
    boxes = [widen(p, len(contigs[int(p[0])]), len(reads[int(p[1])]), extend) for p in placements]
    pairs = [tc.stretches(contigs, reads, b) for b in boxes]
    res = [None] * len(boxes)
    pending = list(range(len(boxes)))
    W = band
    for rnd in range(tc.ROUNDS):
        if not pending:
            break
        last = rnd + 1 == tc.ROUNDS or 2 * W > band_max
        got = refine_round([pairs[x] for x in pending], [boxes[x][3] for x in pending], tspace, W, match, diff, min_score)
        nxt = []
        for x, (st, cells, tr, df, sc) in zip(pending, got):
            ends = None
            if st == tc.OK:
                wab, wbb = boxes[x][3], boxes[x][5]
                ends = (wab + cells[0], wab + cells[2], wbb + cells[1], wbb + cells[3])
            res[x] = (st, W, ends, tr, df, sc)
            if st in (tc.TOUCHED, tc.NO_PATH) and not last:
                nxt.append(x)
        pending = nxt
        if last:
            break
        W *= 2
    return res


# ---- generators the CPU and the GPU tests share -------------------------------------------------------------------------------------------
def mutate(rng, seq, p):
    """seq with errors at rate p: a third each deletions, insertions, substitutions."""
    out = []
    for x in np.asarray(seq).tolist():
        u = rng.random()
        if u < p / 3:
            continue
        if u < 2 * p / 3:
            out += [int(rng.integers(0, 4)), x]
        elif u < p:
            out.append(int((x + 1 + rng.integers(0, 3)) % 4))
        else:
            out.append(x)
    return np.asarray(out, np.uint8)


def planted(rng, alen, err, da0, da1, flank=160):
    """One planted alignment: contig[flank, flank + alen) against a read whose middle is that stretch with errors, both between
    unrelated flanks.  The given end points are the planted ones moved by da0 at the front and da1 at the back (positive = too far
    out), the same amount on both sequences.  Returns (contig, read, given placement, planted (ab, ae, bb, be))."""
    contig = rng.integers(0, 4, size=alen + 2 * flank, dtype=np.uint8)
    mid = mutate(rng, contig[flank:flank + alen], err)
    # the planted end points are bases that match: an error at the very end would move the truth itself
    mid = np.concatenate([contig[flank:flank + 1], mid[1:-1] if len(mid) > 2 else mid[:0], contig[flank + alen - 1:flank + alen]]).astype(np.uint8)
    read = np.concatenate([rng.integers(0, 4, size=flank, dtype=np.uint8), mid, rng.integers(0, 4, size=flank, dtype=np.uint8)]).astype(np.uint8)
    truth = (flank, flank + alen, flank, flank + len(mid))
    given = (0, 0, 0, truth[0] - da0, truth[1] + da1, truth[2] - da0, truth[3] + da1)
    return contig, read, given, truth


REGIMES = {"exact": (0, 0), "out60": (60, 60), "in40": (-40, -40), "asym": (100, -30)}


def hand_cases(seed=11):
    """(contigs, reads, placements by name, calls): the placements of the hand cases and the calls that run them; a call is
    (label, names, keyword arguments of model_refine / Context.trace_refine).  What each case is there for is asserted on the
    model's answer in tests/test_trace_refine_model.py::test_hand_cases_are_what_they_are_named."""
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 4, size=3000, dtype=np.uint8)
    contigs = [contig, rng.integers(0, 4, size=300, dtype=np.uint8), rng.integers(0, 4, size=700, dtype=np.uint8)]
    reads, pl = [], {}

    def away(seq):                       # a flank that differs from seq base for base
        return ((np.asarray(seq) + 1 + rng.integers(0, 3, size=len(seq))) % 4).astype(np.uint8)

    def add(name, a, ab, ae, mid, fl, fr, d0=0, d1=0, comp=0, flanks="away"):
        """read = flank + mid + flank; given = the planted end points moved out by d0 / d1 (negative: in)."""
        c = contigs[a]
        left = away(c[ab - fl:ab]) if flanks == "away" else rng.integers(0, 4, size=fl, dtype=np.uint8)
        right = away(c[ae:ae + fr]) if flanks == "away" else rng.integers(0, 4, size=fr, dtype=np.uint8)
        assert len(left) == fl and len(right) == fr
        whole = np.concatenate([left, mid, right]).astype(np.uint8)
        reads.append(tc.revcomp(whole) if comp else whole)
        pl[name] = (a, len(reads) - 1, comp, ab - d0, ae + d1, fl - d0, fl + len(mid) + d1)

    add("boundary", 0, 300, 500, contig[300:500].copy(), 80, 80, 30, 30)                  # 1: the kept run is [300, 500) at tspace 100
    add("first_segment", 0, 410, 450, contig[410:450].copy(), 60, 60, 5, 5)               # 2: with extend 5 the box is [400, 460)
    add("one_segment", 0, 620, 680, contig[620:680].copy(), 90, 90, 30, 30)               # 3: the box spans three blocks, the run one
    add("clamp_front", 0, 10, 200, mutate(rng, contig[10:200], 0.06), 4, 70, 0, 20)       # 4: room 10 on A, 4 on B at the front
    add("clamp_comp", 0, 800, 1000, mutate(rng, contig[800:1000], 0.06), 3, 70, 0, 0, comp=1)   # 4: B's room is at the stored read's END
    add("clamp_back", 1, 100, 300, mutate(rng, contigs[1][100:300], 0.06), 70, 0, 10, 0)    # 4: the contig ends with the placement
    add("identical", 0, 1000, 1300, contig[1000:1300].copy(), 0, 0)                       # 6: no room at all: the box is the given one
    add("noise", 0, 1400, 1700, rng.integers(0, 4, size=300, dtype=np.uint8), 40, 40, flanks="random")   # 7
    add("undershoot", 0, 1800, 2200, mutate(rng, contig[1800:2200], 0.06), 90, 90, -40, -40)
    add("overshoot_comp", 0, 2300, 2700, mutate(rng, contig[2300:2700], 0.15), 90, 90, 60, 60, comp=1)
    # 9: 300 bases inserted inside one segment; kept across the insertion only when a match outweighs it (scores 15, 1)
    # (one base 300 times, not the A base in front of it: the only cheapest path takes the 300 in one piece)
    ins = np.concatenate([contig[2010:2050], np.full(300, (contig[2049] + 1) % 4, np.uint8), contig[2050:2090]])
    add("wide", 0, 2010, 2090, ins, 0, 0)
    # 8: the path reaches the band's first diagonal (W = 16) only in a tail that the clipping drops: 200 equal bases, then 16 bases
    # of A against nothing, 150 equal bases, 16 bases of B against nothing - 32 operations where the straight way costs about a
    # hundred; at scores 1 / 15 the 150 do not pay for the 16 in front of them
    tail = np.concatenate([contig[2816:2966], away(contig[2950:2966])])
    add("tail_touch", 0, 2600, 2966, np.concatenate([contig[2600:2800], tail]), 0, 0)
    # a KEPT column on the band's last diagonal at W = 16: 15 bases inserted, 200 equal ones, 15 skipped (the centre line stays flat)
    c2 = contigs[2]
    add("touch_kept", 2, 60, 560, np.concatenate([c2[60:210], away(c2[210:225]), c2[210:410], c2[425:560]]), 0, 0)
    main = ["boundary", "first_segment", "one_segment", "clamp_front", "clamp_comp", "clamp_back", "identical", "noise", "undershoot", "overshoot_comp"]
    calls = [("defaults_w64", main, dict(tspace=100, band=64, band_max=1024)),
             ("extend_0", main, dict(tspace=100, band=64, band_max=1024, extend=0)),                        # 5
             ("extend_5", ["first_segment", "boundary"], dict(tspace=100, band=16, band_max=64, extend=5)),  # 2
             ("two_byte_w16", main, dict(tspace=200, band=16, band_max=1024)),                              # 10
             ("tspace_7", ["boundary", "clamp_comp", "one_segment"], dict(tspace=7, band=64, band_max=64)),
             ("noise_min_score_40", ["undershoot", "noise", "boundary"], dict(tspace=100, band=64, band_max=64, min_score=40)),   # 7
             ("tail_touch", ["tail_touch"], dict(tspace=100, band=16, band_max=1024, extend=0, match=1, diff=15)),  # 8
             ("touch_kept", ["touch_kept", "identical"], dict(tspace=100, band=16, band_max=64)),
             ("wide", ["identical", "wide", "boundary"], dict(tspace=100, band=16, band_max=1024, match=15, diff=1))]   # 9
    return contigs, reads, pl, calls


def perturbed_many(seed=23, n=130):
    """n short placements on one contig, both strands, every end point moved by up to 20 bases either way."""
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 4, size=3400, dtype=np.uint8)
    reads, pl = [], []
    for x in range(n):
        ab = int(rng.integers(100, 3000))
        ae = ab + int(rng.integers(60, 200))
        mid = mutate(rng, contig[ab:ae], 0.08)
        whole = np.concatenate([rng.integers(0, 4, size=40, dtype=np.uint8), mid, rng.integers(0, 4, size=40, dtype=np.uint8)]).astype(np.uint8)
        comp = int(x % 3 == 0)
        reads.append(tc.revcomp(whole) if comp else whole)
        d0, d1 = int(rng.integers(-20, 21)), int(rng.integers(-20, 21))
        pl.append((0, x, comp, ab - d0, ae + d1, 40 - d0, 40 + len(mid) + d1))
    return [contig], reads, pl


def perturbed_cns_tiny(seed=17, amount=60):
    """cns_tiny's records as placements with every end point moved by a seeded -amount .. +amount, kept inside its sequence."""
    from hinge_amd import synth_consensus as sc
    d = sc.generate(sc.CONFIGS["cns_tiny"])
    rng = np.random.default_rng(seed)
    pls = []
    for q in d.rec:
        alen, blen = len(d.contigs[int(q["aread"])]), len(d.reads[int(q["bread"])])
        mv = rng.integers(-amount, amount + 1, size=4)
        ab, ae = max(int(q["abpos"]) + int(mv[0]), 0), min(int(q["aepos"]) + int(mv[1]), alen)
        bb, be = max(int(q["bbpos"]) + int(mv[2]), 0), min(int(q["bepos"]) + int(mv[3]), blen)
        assert ab < ae and bb < be
        pls.append((int(q["aread"]), int(q["bread"]), int(q["flags"] & 1), ab, ae, bb, be))
    return d, pls
