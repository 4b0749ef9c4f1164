"""Shared by the `hinge paf2las --ends local` tests: the numpy model behind hinge_trace_local ("Local"), written
from the rule and not from the kernels: it fills the band row by row (a prefix maximum settles the gaps in A of a row; the kernels go
anti-diagonal by anti-diagonal), marks the cells with H = 0 in the direction table and walks back until it stands on one (the kernel
keeps no H: it counts the score down).

  the box is widened as for refine (trace_refine_common.widen).  Cell (i, j): i bases of A, j of B consumed;
  centre(i) = floor((2 i (blen - alen) + alen) / (2 alen)); in the band when k = j - i - centre(i) + W is in [0, 2 W).
  H(i, j) = max(0, H(i - 1, j - 1) + (equal ? +match : -diff), H(i - 1, j) - diff, H(i, j - 1) - diff); row 0, column 0 and every
  cell outside the band read as 0.  Ties of a cell: 0 wins; then diagonal, gap in B (from (i - 1, j)), gap in A (from (i, j - 1)).
  Best cell: the largest H; of equal ones the smallest i + j; of those the smallest i.  Kept: the path from the best cell back to
  the first cell with H = 0.  Below max(1, min_score): EMPTY - and, unlike refine, EMPTY widens like NO_PATH while 2 W fits
  band_max.  TOUCHED: a kept column within margin(W) diagonals of the band's first or last one.
"""
import numpy as np

import trace_common as tc
from trace_refine_common import EMPTY, mutate, perturbed_cns_tiny, planted, widen  # noqa: F401  (the tests take them from here)

ZERO = 4                    # direction table: a cell with H = 0 (the walk stops on it)
LOCAL_MARGIN = 3            # TRACE_LOCAL_MARGIN of hinge_amd/csrc/trace_kernels.h: measured (tools/trace_local_measure.py margin)
MIN_SCORE = 24              # the default min_score of the mode (HINGE_TRACE_LOCAL_MIN_SCORE): 16, the largest score of 16 unrelated 7128 x 7128 pairs at W = 1024, plus half


def centre(i, alen, blen):
    return (2 * i * (blen - alen) + alen) // (2 * alen)


def margin(W, m=None):
    """Diagonals at either edge of the band that count as touched: capped so that the W in the middle never do."""
    return min(LOCAL_MARGIN if m is None else m, W // 2)


def fill_local(pairs, W, match=1, diff=2):
    """Per (A, B) pair (|blen - alen| <= W): D[alen + 1, 2 W] uint8 (0 diagonal equal, 3 diagonal different, 1 gap in B, 2 gap in
    A, ZERO where H = 0, 255 outside the matrix), the centres C[alen + 1], and the best cell (score, i1, j1)."""
    n = len(pairs)
    alen = np.array([len(a) for a, _ in pairs], np.int64)
    blen = np.array([len(b) for _, b in pairs], np.int64)
    L, M = int(alen.max()), int(blen.max())
    Ap = np.zeros((n, L + 1), np.int32)
    Bp = np.zeros((n, M + 1), np.int32)
    for x, (a, b) in enumerate(pairs):
        Ap[x, :len(a)] = a
        Bp[x, :len(b)] = b
    C = np.stack([centre(np.arange(L + 1, dtype=np.int64), int(al), int(bl)) for al, bl in zip(alen, blen)]).astype(np.int64)
    K = np.arange(2 * W, dtype=np.int64)[None, :]
    PAD = 2 * W + 2
    D = np.full((n, L + 1, 2 * W), 255, np.uint8)
    j0 = K - W + np.zeros((n, 1), np.int64)
    D[:, 0, :] = np.where((j0 >= 0) & (j0 <= blen[:, None]), ZERO, 255)
    cur = np.zeros((n, 2 * W), np.int64)                                 # row 0
    prevp = np.zeros((n, 2 * W + 2 * PAD), np.int64)                     # whatever lies beside the band reads as 0
    bs, bt, bi = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    rows = np.arange(n)
    for i in range(1, L + 1):
        act = alen >= i
        prevp[:, PAD:PAD + 2 * W] = cur
        shift = (C[:, i] - C[:, i - 1])[:, None]
        j = i + C[:, i][:, None] + K - W
        valid = (j >= 0) & (j <= blen[:, None]) & act[:, None]
        inner = valid & (j >= 1)
        eq = Ap[:, i - 1][:, None] == np.take_along_axis(Bp, np.clip(j - 1, 0, M), axis=1)
        diag = np.take_along_axis(prevp, np.clip(K + shift + PAD, 0, prevp.shape[1] - 1), axis=1) + np.where(eq, match, -diff)
        up = np.take_along_axis(prevp, np.clip(K + shift + 1 + PAD, 0, prevp.shape[1] - 1), axis=1) - diff
        best = np.maximum(diag, up)
        d = np.where(up > diag, 1, np.where(eq, 0, 3))
        E = np.where(inner, np.maximum(best, 0), 0)
        run = np.maximum.accumulate(E + diff * K, axis=1) - diff * K      # the best way in along the row: gaps in A
        H = np.where(inner, run, 0)
        d = np.where(run > best, 2, d)
        D[:, i, :] = np.where(valid, np.where(H > 0, d, ZERO), 255)
        cur = H
        m = H.max(axis=1)
        kk = H.argmax(axis=1)                                              # the first of equal ones: the smallest j of the row
        t = i + j[rows, kk]
        upd = act & (m > 0) & ((m > bs) | ((m == bs) & (t < bt)))          # (equal score and equal t: the earlier row stays)
        bs, bt, bi = np.where(upd, m, bs), np.where(upd, t, bt), np.where(upd, i, bi)
    return ([D[x, :alen[x] + 1] for x in range(n)], [C[x, :alen[x] + 1] for x in range(n)],
            [(int(bs[x]), int(bi[x]), int(bt[x] - bi[x])) for x in range(n)])


def kept_columns(D, C, best, W):
    """The kept path front to back: rows of (direction, i, j, k) with (i, j) the cell the column ends in; and the start cell."""
    _, i, j = best
    out = []
    while i > 0 and j > 0:
        k = j - i - int(C[i]) + W
        if not 0 <= k < 2 * W:                   # one diagonal outside the band: reads as 0
            break
        d = int(D[i, k])
        assert d != 255
        if d == ZERO:
            break
        out.append((d, i, j, k))
        if d in (0, 3):
            i, j = i - 1, j - 1
        elif d == 1:
            i -= 1
        else:
            j -= 1
    return out[::-1], (i, j)


def local_of(D, C, best, wab, tspace, W, match=1, diff=2, min_score=MIN_SCORE, m=None):
    """(status, (i0, j0, i1, j1) or None, trace or None, diffs, score) of one filled box."""
    score, i1, j1 = best
    if score < max(1, min_score):
        return EMPTY, None, None, 0, 0
    kept, (i0, j0) = kept_columns(D, C, best, W)
    assert kept and kept[0][0] == 0 and kept[-1][0] == 0 and i0 < i1 and j0 < j1
    nd = sum(c[0] != 0 for c in kept)
    assert match * (len(kept) - nd) - diff * nd == score
    first = (wab + i0) // tspace
    nseg = tc.n_segments(wab + i0, wab + i1, tspace)
    sd, sb = [0] * nseg, [0] * nseg
    for d, i, j, k in kept:
        g = (wab + i - 1) // tspace - first
        sd[g] += d != 0
        sb[g] += d != 1
    mg = margin(W, m)
    touched = any(c[3] < mg or c[3] >= 2 * W - mg for c in kept)
    tmax = tc.trace_max(tspace)
    wide = max(sd) > tmax or max(sb) > tmax
    st = tc.TOUCHED if touched else tc.WIDE if wide else tc.OK
    if st != tc.OK:
        return st, None, None, 0, 0
    return st, (i0, j0, i1, j1), [int(v) for pr in zip(sd, sb) for v in pr], int(sum(sd)), score


def local_round(pairs, wabs, tspace, W, match=1, diff=2, min_score=MIN_SCORE, m=None, chunk=32):
    """One round at W over widened boxes: per pair what local_of() answers (NO_PATH from the lengths)."""
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
        Ds, Cs, bests = fill_local([pairs[x] for x in xs], W, match, diff)
        for x, D, C, b in zip(xs, Ds, Cs, bests):
            out[x] = local_of(D, C, b, wabs[x], tspace, W, match, diff, min_score, m)
    return out


def model_local(contigs, reads, placements, tspace, band=128, band_max=1024, extend=50, match=1, diff=2, min_score=MIN_SCORE, m=None, stats=None):
    """What hinge_trace_local answers: per placement (status, final W, (abpos', aepos', bbpos', bepos') or None, trace or None,
    diffs, score).  stats (a dict): "empty_widened" = placements that went on to 2 W because they were EMPTY, "rounds"."""
    boxes = [widen(p, len(contigs[int(p[0])]), len(reads[int(p[1])]), extend) for p in placements]
    pairs = [tc.stretches(contigs, reads, b) for b in boxes]
    res = [None] * len(boxes)
    pending = list(range(len(boxes)))
    W = band
    ew = rounds = 0
    for rnd in range(tc.ROUNDS):
        if not pending:
            break
        rounds = rnd + 1
        last = rnd + 1 == tc.ROUNDS or 2 * W > band_max
        got = local_round([pairs[x] for x in pending], [boxes[x][3] for x in pending], tspace, W, match, diff, min_score, m)
        nxt = []
        for x, (st, cells, tr, df, sc) in zip(pending, got):
            ends = None
            if st == tc.OK:
                wab, wbb = boxes[x][3], boxes[x][5]
                ends = (wab + cells[0], wab + cells[2], wbb + cells[1], wbb + cells[3])
            res[x] = (st, W, ends, tr, df, sc)
            if st in (tc.TOUCHED, tc.NO_PATH, EMPTY) and not last:
                nxt.append(x)
                ew += st == EMPTY
        pending = nxt
        if last:
            break
        W *= 2
    if stats is not None:
        stats.update(empty_widened=ew, rounds=rounds)
    return res


# ---- generators the CPU and the GPU tests share -------------------------------------------------------------------------------------------
def planted_independent(rng, alen, err, amount, flank=160):
    """trace_refine_common.planted with all four end points moved independently by a seeded -amount .. +amount."""
    contig, read, given, truth = planted(rng, alen, err, 0, 0, flank)
    mv = rng.integers(-amount, amount + 1, size=4)
    g = (0, 0, 0, truth[0] + int(mv[0]), truth[1] + int(mv[1]), truth[2] + int(mv[2]), truth[3] + int(mv[3]))
    return contig, read, g, truth


TANDEM_UNIT = (0, 1, 2)


def hand_cases(seed=31):
    """(contigs, reads, placements by name, calls): a call is (label, names, keyword arguments of model_local / Context.trace_local).
    What each case is there for is asserted on the model in tests/test_trace_local_model.py::test_hand_cases_are_what_they_are_named."""
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 4, size=3000, dtype=np.uint8)
    unit = np.asarray(TANDEM_UNIT, np.uint8)
    contigs = [contig, rng.integers(0, 4, size=300, dtype=np.uint8), rng.integers(0, 4, size=400, dtype=np.uint8),
               np.concatenate([rng.integers(0, 4, size=50, dtype=np.uint8), np.tile(unit, 30), rng.integers(0, 4, size=50, dtype=np.uint8)]).astype(np.uint8)]
    reads, pl = [], {}

    def junk(n):
        return rng.integers(0, 4, size=n, dtype=np.uint8)

    def add(name, a, whole, comp, ab, ae, bb, be):
        whole = np.asarray(whole, np.uint8)
        assert 0 <= ab < ae <= len(contigs[a]) and 0 <= bb < be <= len(whole)
        reads.append(tc.revcomp(whole) if comp else whole)
        pl[name] = (a, len(reads) - 1, comp, ab, ae, bb, be)

    # all four end points moved independently, both strands (alen 300 and 400, 6 % and 15 % errors)
    mid = mutate(rng, contig[300:600], 0.06)
    add("plain", 0, np.concatenate([junk(80), mid, junk(80)]), 0, 300 - 30, 600 + 20, 80 - 10, 80 + len(mid) + 25)
    mid = mutate(rng, contig[700:1100], 0.15)
    add("plain_comp", 0, np.concatenate([junk(90), mid, junk(90)]), 1, 700 + 25, 1100 - 35, 90 + 5, 90 + len(mid) - 10)
    # the alignment begins in row 0: the contig begins with it, the given B start lies 20 bases in front of the true one
    mid = mutate(rng, contigs[1], 0.06)
    add("row0", 1, np.concatenate([junk(40), mid, junk(20)]), 0, 0, 300, 20, 40 + len(mid))
    # ... and in column 0: the read begins with it, the given A start lies 20 bases in front of the true one
    mid = mutate(rng, contig[1500:1800], 0.06)
    add("col0", 0, np.concatenate([mid, junk(60)]), 0, 1480, 1800, 0, len(mid))
    # the start cell one diagonal outside the band at W = 8 (extend 0: alen 200, blen 208, so c(12) = 0 and c(13) = 1): B = 20
    # bases that differ, then A[12, 200) - the first kept column ends in (13, 21) on the band's last diagonal, its front (12, 20) is at k = 16
    a2 = contigs[2]
    add("outside_start", 2, np.concatenate([(a2[100:120] + 1 + rng.integers(0, 3, size=20)) % 4, a2[112:300]]), 0, 100, 300, 0, 208)
    # many equal maxima: ten units of a tandem repeat against thirty
    add("tandem", 3, np.tile(unit, 10), 0, 50, 140, 0, 30)
    add("unrelated", 0, junk(300), 0, 2000, 2300, 0, 300)
    # the true diagonal 90 beside the centre line: nothing of it in the band at W = 64
    mid = mutate(rng, contig[2400:2700], 0.06)
    add("off_diagonal", 0, np.concatenate([junk(90), mid, junk(100)]), 0, 2400, 2800, 0, 400)
    add("identical", 0, contig[1000:1300].copy(), 0, 1000, 1300, 0, 300)
    add("identical_comp", 0, np.concatenate([junk(30), contig[1150:1400], junk(30)]), 1, 1160, 1390, 40, 270)
    main = ["plain", "plain_comp", "row0", "col0", "tandem", "unrelated", "off_diagonal", "identical", "identical_comp"]
    calls = [("w64", main, dict(tspace=100, band=64, band_max=256)),
             ("w8", main, dict(tspace=100, band=8, band_max=128)),
             ("two_byte", main, dict(tspace=200, band=64, band_max=128)),
             ("last_w64", ["off_diagonal", "plain", "unrelated"], dict(tspace=100, band=64, band_max=64)),
             ("outside_w8", ["outside_start", "identical"], dict(tspace=100, band=8, band_max=8, extend=0)),
             ("outside_w8_64", ["identical", "outside_start"], dict(tspace=100, band=8, band_max=64, extend=0)),
             ("scores_2_3", ["plain", "tandem", "plain_comp", "col0"], dict(tspace=100, band=64, band_max=128, match=2, diff=3, min_score=50)),
             ("min_score_1", ["unrelated", "row0"], dict(tspace=100, band=64, band_max=64, min_score=1)),
             ("tspace_7", ["row0", "identical_comp", "tandem"], dict(tspace=7, band=64, band_max=64, extend=0))]
    return contigs, reads, pl, calls


def beside(truth, off):
    """A given placement that holds the planted alignment truth = (ab, ae, bb, be) whole, with the true diagonal `off` beside the
    box's centre line (positive: towards larger j): one sequence's window grows by |off| per side, the other's by 2 |off| at the
    front only.  The flanks must hold 2 |off| + the extension."""
    d = abs(off)
    if off >= 0:
        return (0, 0, 0, truth[0] - d, truth[1] + d, truth[2] - 2 * d, truth[3])
    return (0, 0, 0, truth[0] - 2 * d, truth[1], truth[2] - d, truth[3] + d)


def perturbed_many(seed=29, n=130):
    """n short placements on one contig, both strands, all four end points moved independently by up to 20 bases either way."""
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
        mv = rng.integers(-20, 21, size=4)
        pl.append((0, x, comp, ab + int(mv[0]), ae + int(mv[1]), 40 + int(mv[2]), 40 + len(mid) + int(mv[3])))
    return [contig], reads, pl
