"""Shared by the `hinge paf2las` tests: a numpy model of the banded alignment behind hinge_trace_run, written
from the specification - the band formula, the tie order, the walk, the widening rounds - and not from the kernels: it fills the
band row by row (a prefix minimum settles the gaps in A of a row), the kernels anti-diagonal by anti-diagonal.

  cell (i, j): i bases of A, j bases of B consumed; centre(i) = floor((2 i (blen - alen) + alen) / (2 alen));
  in the band when k = j - i - centre(i) + W is in [0, 2 W); ties: diagonal, then the gap in B (from (i - 1, j)), then the gap
  in A (from (i, j - 1)); a B-only step belongs to the trace-point segment of the A base in front of it (the first segment at i = 0).
"""
import numpy as np

OK, TOUCHED, NO_PATH, WIDE, STEPS = 0, 1, 2, 3, 4
INF = 1 << 30
ROUNDS = 9          # doublings from the smallest (8) to the largest (2048) legal band; with the defaults 128 -> 1024 there are four


def centre(i, alen, blen):
    return (2 * i * (blen - alen) + alen) // (2 * alen)


def n_segments(ab, ae, tspace):
    return (ae - 1) // tspace - ab // tspace + 1


def trace_max(tspace):
    return 255 if tspace <= 125 else 65534


def revcomp(b):
    return (3 - np.asarray(b)[::-1]).astype(np.uint8)


def stretches(contigs, reads, p):
    """(A, B) of a placement p = (aread, bread, comp, abpos, aepos, bbpos, bepos): B in the complemented frame when comp."""
    a, b, comp, ab, ae, bb, be = [int(v) for v in p]
    r = revcomp(reads[b]) if comp else np.asarray(reads[b])
    return np.asarray(contigs[a])[ab:ae], r[bb:be]


def levenshtein(A, B):
    """Unbanded edit distance (small inputs)."""
    A, B = np.asarray(A), np.asarray(B)
    n = len(B)
    idx = np.arange(n + 1)
    row = idx.copy()
    for x in A:
        best = np.empty(n + 1, np.int64)
        best[0] = row[0] + 1
        best[1:] = np.minimum(row[:-1] + (B != x), row[1:] + 1)
        row = np.minimum.accumulate(best - idx) + idx
    return int(row[n])


def _fill(pairs, W):
    """Directions and end cost of every (A, B) pair at half-width W (|blen - alen| <= W for all).  Rows of all pairs in step.
    Returns (D[n][alen + 1, 2 W] uint8 with 0 diagonal equal, 3 diagonal different, 1 gap in B, 2 gap in A; C[n] centres; end cost[n])."""
    n = len(pairs)
    alen = np.array([len(a) for a, _ in pairs], np.int64)
    blen = np.array([len(b) for _, b in pairs], np.int64)
    L, M = int(alen.max()), int(blen.max())
    Ap = np.zeros((n, L + 1), np.int32)
    Bp = np.zeros((n, M + 1), np.int32)
    for x, (a, b) in enumerate(pairs):
        Ap[x, :len(a)] = a
        Bp[x, :len(b)] = b
    I = np.arange(L + 1, dtype=np.int64)[None, :]
    C = ((2 * I * (blen - alen)[:, None] + alen[:, None]) // (2 * alen[:, None])).astype(np.int32)
    alen, blen = alen.astype(np.int32), blen.astype(np.int32)      # (the centres need 64 bits, the cells do not)
    K = np.arange(2 * W, dtype=np.int32)[None, :]
    PAD = 2 * W + 2
    D = np.full((n, L + 1, 2 * W), 255, np.uint8)
    j = K - W + np.zeros((n, 1), np.int32)
    valid = (j >= 0) & (j <= blen[:, None])
    cur = np.where(valid, j, INF).astype(np.int32)
    D[:, 0, :] = np.where(valid, 2, 255)
    end = np.full(n, INF, np.int64)
    prevp = np.full((n, 2 * W + 2 * PAD), INF, np.int32)
    for i in range(1, L + 1):
        act = alen >= i
        prevp[:, PAD:PAD + 2 * W] = cur
        shift = (C[:, i] - C[:, i - 1])[:, None]
        j = np.int32(i) + C[:, i][:, None] + K - np.int32(W)
        valid = (j >= 0) & (j <= blen[:, None]) & act[:, None]
        kd = np.clip(K + shift + PAD, 0, prevp.shape[1] - 1)
        kg = np.clip(K + shift + 1 + PAD, 0, prevp.shape[1] - 1)
        ne = Ap[:, i - 1][:, None] != np.take_along_axis(Bp, np.clip(j - 1, 0, M), axis=1)
        diag = np.where(j >= 1, np.take_along_axis(prevp, kd, axis=1) + ne.astype(np.int32), np.int32(INF))
        bgap = np.take_along_axis(prevp, kg, axis=1) + np.int32(1)
        best = np.minimum(diag, bgap)
        d = np.where(bgap < diag, 1, np.where(ne, 3, 0))
        best = np.where(valid, np.minimum(best, np.int32(INF)), np.int32(INF))
        run = np.minimum.accumulate(best - K, axis=1) + K          # the cheapest way in along the row: gaps in A
        d = np.where(run < best, 2, d)
        new = np.where(valid, np.minimum(run, np.int32(INF)), np.int32(INF))
        D[:, i, :] = np.where(valid, d, 255)
        cur = np.where(act[:, None], new, cur)
        done = alen == i
        if done.any():
            end[done] = cur[done, W]
    return [D[x, :alen[x] + 1] for x in range(n)], [C[x, :alen[x] + 1] for x in range(n)], end


def _walk(D, C, alen, blen, ab, tspace, W):
    nseg = n_segments(ab, ab + alen, tspace)
    sd, sb = [0] * nseg, [0] * nseg
    i, j, touched = alen, blen, False
    for _ in range(alen + blen + 1):
        if i == 0 and j == 0:
            break
        k = j - i - int(C[i]) + W
        touched = touched or k == 0 or k == 2 * W - 1
        d = 2 if i == 0 else int(D[i, k])
        assert d != 255
        s = (ab + i - 1) // tspace - ab // tspace if i > 0 else 0
        if d in (0, 3):
            i, j = i - 1, j - 1
            sb[s] += 1
            sd[s] += d == 3
        elif d == 1:
            i -= 1
            sd[s] += 1
        else:
            j -= 1
            sb[s] += 1
            sd[s] += 1
    assert i == 0 and j == 0
    tmax = trace_max(tspace)
    wide = any(v > tmax for v in sd) or any(v > tmax for v in sb)
    trace = [v for pr in zip(sd, sb) for v in pr]
    return (TOUCHED if touched else WIDE if wide else OK), trace, sum(sd)


def align_round(pairs, abs_, tspace, W, chunk=32):
    """One round at W: per pair (status, trace or None, diffs)."""
    out = [None] * len(pairs)
    todo = []
    for x, (a, b) in enumerate(pairs):
        if abs(len(b) - len(a)) > W:
            out[x] = (NO_PATH, None, 0)
        else:
            todo.append(x)
    todo.sort(key=lambda x: len(pairs[x][0]))
    for c0 in range(0, len(todo), chunk):
        xs = todo[c0:c0 + chunk]
        Ds, Cs, end = _fill([pairs[x] for x in xs], W)
        for x, D, C, e in zip(xs, Ds, Cs, end):
            if e >= INF:
                out[x] = (NO_PATH, None, 0)
                continue
            st, tr, df = _walk(D, C, len(pairs[x][0]), len(pairs[x][1]), abs_[x], tspace, W)
            assert df == e
            out[x] = (st, tr if st == OK else None, df if st == OK else 0)
    return out


def model_run(contigs, reads, placements, tspace, band=128, band_max=1024, cache=None):
    """What hinge_trace_run answers: per placement (status, final W, trace list or None, diffs).  cache (a dict) keeps every
    (placement index, W) result: a round's answer does not depend on the W the call started from."""
    pairs = [stretches(contigs, reads, p) for p in placements]
    abs_ = [int(p[3]) for p in placements]
    res = [None] * len(pairs)
    pending = list(range(len(pairs)))
    W = band
    for rnd in range(ROUNDS):
        if not pending:
            break
        last = rnd + 1 == ROUNDS or 2 * W > band_max
        fresh = [x for x in pending if cache is None or (x, W) not in cache]
        got = dict(zip(fresh, align_round([pairs[x] for x in fresh], [abs_[x] for x in fresh], tspace, W)))
        if cache is not None:
            cache.update({(x, W): v for x, v in got.items()})
            got = {x: cache[(x, W)] for x in pending}
        nxt = []
        for x in pending:
            st, tr, df = got[x]
            res[x] = (st, W, tr, df)
            if st in (TOUCHED, NO_PATH) and not last:
                nxt.append(x)
        pending = nxt
        if last:
            break
        W *= 2
    return res


# ---- the hand cases of the tests (CPU model test and GPU test share them) --------------------------------------------------------------
def hand_cases(seed=5):
    """(contigs, reads, cases): cases = list of (name, placement, expectation or None)."""
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 4, size=1000, dtype=np.uint8)
    contigs = [contig, rng.integers(0, 4, size=640, dtype=np.uint8)]
    reads, cases = [], []

    def noisy(seq, p=0.06):
        out = []
        for x in seq.tolist():
            u = rng.random()
            if u < p / 3:
                continue
            if u < 2 * p / 3:
                out.append(int(rng.integers(0, 4)))
            if u < p:
                out.append(int((x + 1) % 4))
            else:
                out.append(x)
        return np.asarray(out, np.uint8)

    def add(name, a, ab, ae, seq, comp=0, fl=3, fr=2, expect=None):
        whole = np.concatenate([rng.integers(0, 4, size=fl, dtype=np.uint8), seq, rng.integers(0, 4, size=fr, dtype=np.uint8)]).astype(np.uint8)
        reads.append(revcomp(whole) if comp else whole)
        cases.append((name, (a, len(reads) - 1, comp, ab, ae, fl, fl + len(seq)), expect))

    add("one_block", 0, 130, 170, noisy(contig[130:170]))
    add("odd_ends", 0, 137, 561, noisy(contig[137:561]))
    add("whole_contig", 1, 0, 640, noisy(contigs[1]), fl=0, fr=0)
    add("alen_1", 0, 400, 401, contig[400:401].copy())
    add("identical", 0, 200, 500, contig[200:500].copy(), expect=OK)
    add("comp_strand", 0, 250, 731, noisy(contig[250:731]), comp=1)
    add("block_aligned", 0, 300, 600, noisy(contig[300:600]))
    return contigs, reads, cases


def indel_cases(seed=6):
    """A 30-base insertion and a 30-base deletion in otherwise equal stretches (start W 16), a read far longer than its stretch
    (NO_PATH at any W <= 1024) between two plain neighbours, a 300-base insertion inside one segment (WIDE)."""
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 4, size=2400, dtype=np.uint8)
    reads, pl = [], []

    def add(seq, ab, ae):
        reads.append(np.asarray(seq, np.uint8))
        pl.append((0, len(reads) - 1, 0, ab, ae, 0, len(seq)))

    ins = np.concatenate([contig[100:350], rng.integers(0, 4, size=30, dtype=np.uint8), contig[350:600]])
    add(ins, 100, 600)                                                      # 0: insertion of 30
    add(np.concatenate([contig[700:950], contig[980:1200]]), 700, 1200)     # 1: deletion of 30
    add(contig[1300:1500].copy(), 1300, 1500)                               # 2: neighbour
    add(np.concatenate([contig[1500:1600], rng.integers(0, 4, size=1300, dtype=np.uint8), contig[1600:1700]]), 1500, 1700)   # 3: |blen - alen| = 1300
    add(contig[1700:1900].copy(), 1700, 1900)                               # 4: neighbour
    add(np.concatenate([contig[2010:2050], rng.integers(0, 4, size=300, dtype=np.uint8), contig[2050:2090]]), 2010, 2090)    # 5: 300 inside one segment
    return [contig], reads, pl
