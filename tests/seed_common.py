"""Shared by the `hinge seed` tests and tools: the numpy model behind hinge_seed_run, written from the rule and not
from the kernel: numpy's searchsorted / lexsort / argmax where the kernel has a fixed-trip search, a bitonic sort and a cross-lane
reduction.

  index     every k-mer of every contig at every position (none across two contigs) as (code, gpos), sorted; a code is 2 bits per
            base, the first base on top; gpos = position in the concatenated contigs; a code with more than max_occ entries has none
  job       one per (read, strand); B = the read in the strand's frame, blen its length.  Sampled positions p = 0, s, 2 s, ... <=
            blen - k with s the smallest multiple of step that leaves at most `list` of them.  Hits (d, p, gpos), d = gpos - p + blen,
            enumerated by p then gpos; those beyond `list` are dropped (OVERFLOW)
  window    hits sorted by (d, p); cnt[i] = elements j >= i with d[j] < d[i] + window; best = the largest cnt, of equal ones the
            smallest i; representative = element i + cnt[i] // 2
  more      the next pick: the same among elements whose d is at least `window` away from every chosen [d[i], d[i] + window), i.e.
            d <= lo - window or d >= lo + 2 window; cnt[] itself stays as it was (it counts all elements).  Stop after N picks, at a
            best cnt < min_hits, or at one below half the first pick's (2 cnt < first)
  placement the whole read along the representative's diagonal, clamped to the contig that holds gpos (both cut alike); fewer than
            k bases left: none
  per read  both strands' placements by cnt descending, forward first, d ascending; the first N
"""
import numpy as np

OK, NONE, OVERFLOW = 0, 1, 2
K, STEP, WINDOW, MAX_OCC, LIST = 15, 2, 256, 16, 2048
MIN_HITS = 3                # HINGE_SEED_MIN_HITS of include/hinge_hip.h: 2, the largest best-window count of 16 unrelated 7128-base reads on a random 4.6 Mb draft, plus half (tools/seed_measure.py min-hits)


def revcomp(b):
    return (3 - np.asarray(b, np.uint8)[::-1]).astype(np.uint8)


def kmer_codes(seq, k):
    """The code of the k-mer at every position 0 .. len - k."""
    seq = np.asarray(seq, np.int64)
    n = len(seq) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    c = np.zeros(n, np.int64)
    for t in range(k):
        c = c * 4 + seq[t:t + n]
    return c


class Index:
    def __init__(self, contigs, k=K, max_occ=MAX_OCC):
        self.k, self.max_occ = k, max_occ
        self.clen = np.asarray([len(c) for c in contigs], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.clen)]).astype(np.int64)
        assert int(self.off[-1]) < 2 ** 31
        cs, gs = [], []
        for c, o in zip(contigs, self.off[:-1]):
            kc = kmer_codes(c, k)
            cs.append(kc)
            gs.append(o + np.arange(len(kc), dtype=np.int64))
        codes = np.concatenate(cs) if cs else np.zeros(0, np.int64)
        gpos = np.concatenate(gs) if gs else np.zeros(0, np.int64)
        order = np.argsort(codes, kind="stable")                        # gpos is ascending already
        codes, gpos = codes[order], gpos[order]
        self.all_entries = len(codes)
        if len(codes):
            first = np.concatenate([[True], codes[1:] != codes[:-1]])
            run = np.cumsum(first) - 1
            size = np.bincount(run)
            keep = size[run] <= max_occ
            self.dropped_codes = int((size > max_occ).sum())
            codes, gpos = codes[keep], gpos[keep]
        else:
            self.dropped_codes = 0
        self.codes, self.gpos = codes, gpos

    def contig_of(self, gpos):
        return int(np.searchsorted(self.off, gpos, side="right") - 1)


def stride(blen, k, step, list_):
    """s_j: the smallest multiple of step with at most `list` sampled positions."""
    need = (blen - k) // list_ + 1
    return step * (-(-need // step))


def job_hits(index, B, step=STEP, list_=LIST):
    """(d, p, gpos, overflow) in enumeration order, cut at `list`; None for a read shorter than k."""
    k, blen = index.k, len(B)
    if blen < k:
        return None
    s = stride(blen, k, step, list_)
    p = np.arange(0, blen - k + 1, s, dtype=np.int64)
    assert len(p) <= list_
    codes = kmer_codes(B, k)[p]
    lo = np.searchsorted(index.codes, codes, side="left")
    hi = np.searchsorted(index.codes, codes, side="right")
    occ = hi - lo
    total = int(occ.sum())
    pp = np.repeat(p, occ)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(occ) - occ, occ)
    g = index.gpos[np.repeat(lo, occ) + within] if total else np.zeros(0, np.int64)
    over = total > list_
    pp, g = pp[:list_], g[:list_]
    return g - pp + blen, pp, g, over


def job_picks(index, B, step=STEP, window=WINDOW, list_=LIST, n_max=1, min_hits=MIN_HITS):
    """(status, n_hits, [(cnt, d, p, gpos) per pick]) of one job."""
    h = job_hits(index, B, step, list_)
    if h is None:
        return NONE, 0, []
    d, p, g, over = h
    if len(d) == 0:
        return NONE, 0, []
    order = np.lexsort((p, d))
    d, p, g = d[order], p[order], g[order]
    cnt = np.searchsorted(d, d + window, side="left") - np.arange(len(d))
    ok = np.ones(len(d), bool)
    picks = []
    for _ in range(n_max):
        if not ok.any():
            break
        c = np.where(ok, cnt, -1)
        i = int(np.argmax(c))                                            # the first of equal ones
        best = int(c[i])
        if best < min_hits or (picks and 2 * best < picks[0][0]):
            break
        r = i + best // 2
        picks.append((best, int(d[r]), int(p[r]), int(g[r])))
        lo = int(d[i])
        ok &= (d <= lo - window) | (d >= lo + 2 * window)
    if not picks:
        return NONE, len(d), []
    return (OVERFLOW if over else OK), len(d), picks


def project(index, blen, comp, bread, pick):
    """The placement (aread, bread, comp, abpos, aepos, bbpos, bepos) of a pick, or None."""
    cnt, d, p, gpos = pick
    c = index.contig_of(gpos)
    alen = int(index.clen[c])
    dl = gpos - int(index.off[c]) - p                                    # a = b + dl
    ab, ae, bb, be = dl, dl + blen, 0, blen
    if ab < 0:
        bb, ab = -ab, 0
    if ae > alen:
        be, ae = be - (ae - alen), alen
    if ae - ab < index.k:
        return None
    return (c, bread, comp, ab, ae, bb, be)


def model_seed(contigs, reads, read_ids=None, k=K, step=STEP, window=WINDOW, max_occ=MAX_OCC, list_=LIST, max_placements=1, min_hits=MIN_HITS, index=None, stats=None):
    """What hinge_seed_run answers: (placements [m][7], count [m], diag [m], n_placed per read, status per read (forward, complement))."""
    index = index or Index(contigs, k, max_occ)
    ids = list(range(len(reads))) if read_ids is None else [int(r) for r in read_ids]
    pl, count, diag, n_placed, status = [], [], [], [], []
    for b in ids:
        read = np.asarray(reads[b], np.uint8)
        cand, st = [], []
        for comp in (0, 1):
            s, nh, picks = job_picks(index, revcomp(read) if comp else read, step, window, list_, max_placements, min_hits)
            st.append(s)
            for pk in picks:
                q = project(index, len(read), comp, b, pk)
                if q is not None:
                    cand.append((-pk[0], comp, pk[1], q, pk[3] - pk[2]))
        cand.sort(key=lambda c: c[:3])
        cand = cand[:max_placements]
        for c in cand:
            pl.append(c[3]); count.append(-c[0]); diag.append(c[4])
        n_placed.append(len(cand))
        status.append(tuple(st))
    if stats is not None:
        stats.update(jobs=2 * len(ids), entries=len(index.codes), dropped_codes=index.dropped_codes,
                     overflow=sum(s == OVERFLOW for st in status for s in st), unplaced=sum(n == 0 for n in n_placed))
    return pl, count, diag, n_placed, status


# ---- the recall rule (ISSUE: every generator record of >= 400 contig bases) ----------------------------------------------------------
def recall(d, result, index, window=WINDOW, min_len=400):
    """Per read of the data set (synth_consensus) its longest record against the model's / library's first placement.
    Returns (checked, missed list, left_out list of record lengths)."""
    pl, count, diag, n_placed, status = result
    at = np.concatenate([[0], np.cumsum(n_placed)])
    longest = {}
    for q in d.rec:
        b = int(q["bread"])
        ln = int(q["aepos"]) - int(q["abpos"])
        if b not in longest or ln > longest[b][0]:
            longest[b] = (ln, int(q["aread"]), int(q["flags"]) & 1, int(q["abpos"]), int(q["bbpos"]))
    checked, missed, left_out = 0, [], []
    for b, (ln, a, comp, ab, bb) in sorted(longest.items()):
        if ln < min_len:
            left_out.append(ln)
            continue
        checked += 1
        want = int(index.off[a]) + ab - bb
        hit = False
        for x in range(int(at[b]), int(at[b + 1])):
            if pl[x][0] == a and pl[x][2] == comp and abs(diag[x] - want) <= window + 0.05 * ln:
                hit = True
        if not hit:
            missed.append((b, ln))
    return checked, missed, left_out


# ---- hand-made cases the host test and the GPU test share ------------------------------------------------------------------------------
def repeat_case(seed=5):
    """A contig with one 600-base stretch planted twice, 3 kb apart, and a 500-base read from inside it."""
    rng = np.random.default_rng(seed)
    rep = rng.integers(0, 4, size=600, dtype=np.uint8)
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    contig = np.concatenate([j(1000), rep, j(2400), rep, j(1000)]).astype(np.uint8)
    return [contig], [rep[50:550].copy()]


def edge_calls(seed=7):
    """[(label, contigs, reads, keyword arguments of model_seed, host_only)]."""
    rng = np.random.default_rng(seed)
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cat = lambda *a: np.concatenate(a).astype(np.uint8)
    calls = []
    c = j(3000)
    k = K
    calls.append(("lengths", [c], [c[100:100 + k - 1].copy(), c[200:200 + k].copy(), revcomp(c[300:300 + k + 1])], dict(min_hits=1), True))
    # 64 and 65 sampled positions at step 2: (blen - k) // 2 + 1
    calls.append(("seam", [c], [c[500:500 + k + 126].copy(), c[700:700 + k + 128].copy(), revcomp(c[900:900 + k + 128])], dict(), False))
    calls.append(("step1", [c], [c[1200:1500].copy(), revcomp(c[1600:1903])], dict(step=1), False))
    calls.append(("step3", [c], [c[1200:1500].copy(), revcomp(c[1600:1903])], dict(step=3), False))
    # a code with exactly max_occ (4) and max_occ + 1 entries
    X, Y = j(k), j(k)
    parts = []
    for n in range(5):
        parts += [j(800), X if n < 4 else j(0), j(37), Y]
    cm = cat(*parts, j(300))
    calls.append(("max_occ", [cm], [X.copy(), Y.copy(), revcomp(X)], dict(max_occ=4, min_hits=1, max_placements=8), False))
    # 32 sampled positions x 2 copies = 64 hits = list; a third copy of the first k-mer: 65
    S = j(k + 31)
    c2 = cat(j(200), S, j(300), S, j(200))
    calls.append(("fill64", [c2], [S.copy()], dict(step=1, list_=64, min_hits=4, max_placements=2), False))
    c3 = cat(j(200), S, j(300), S, j(200), S[:k], j(100))
    calls.append(("over65", [c3], [S.copy(), revcomp(S)], dict(step=1, list_=64, min_hits=4, max_placements=2), False))
    big = j(30000)
    calls.append(("long_read", [big], [big[3000:23000].copy()], dict(list_=64), True))
    # contig ends: the first and the last k-mer of either contig; a k-mer made of two contigs' ends
    e0, e1 = j(500), j(700)
    calls.append(("contig_ends", [e0, e1], [e0[:k].copy(), e0[-k:].copy(), e1[:k].copy(), revcomp(e1[-k:]), cat(e0[-8:], e1[:k - 8])], dict(min_hits=1), False))
    # reads hanging over either end, both strands
    h = j(2000)
    w0, w1 = cat(j(100), h[:400]), cat(h[-400:], j(100))
    calls.append(("overhang", [j(300), h], [w0, w1, revcomp(w0), revcomp(w1)], dict(), False))
    rc_, rr = repeat_case()
    for n in (1, 2, 8):
        calls.append(("repeat_n%d" % n, rc_, rr + [revcomp(rr[0])], dict(max_placements=n), False))
    return calls
