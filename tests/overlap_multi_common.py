"""Shared by the `hinge overlap --max-stretches` tests: the numpy model behind hinge_overlap_run_multi and the host program's merge
and duplicate rules, written from the rule and not from the kernel - lexsort, searchsorted and argmax where the
kernel has a bitonic sort, fixed-trip searches, a segmented scan, ballots and dead bits.

  rounds    the hits of a job sorted by (b, d, p) and cnt[i] are overlap_common's.  Every element starts live.  Round r: per b the
            live element of the largest cnt, of equal ones the smallest i; with cnt >= min_hits it is round r's candidate of b,
            (b, cnt, d, p) of element i + cnt // 2 (live or dead).  Then every element of b with d[e] - window < d < d[e] + window
            is dead (e the picked element).  cnt is never recomputed.  Per round: ascending b, the first max_partners (TRUNCATED)
  program   canonical frame: a candidate (a, b, comp, diag) with a > b becomes (b, a, comp, mirrored diag).  Per (a < b, comp) the
            diagonals of both directions sorted; neighbours closer than `window` merge (single linkage); a cluster's representative
            is its member found from a's side of the largest count (without one: its member of the largest count), ties to the
            smaller diagonal - so a pair without a second stretch is aligned along the diagonal the default path takes.  After the alignment the
            records of a key are taken by (A length descending, abpos, bbpos); one is dropped if against a kept one the A ranges
            intersect by more than half the shorter and the smaller of |begin diagonals' difference| and |end diagonals'
            difference| is below `window`
"""
import numpy as np

import overlap_common as oc

NONE, OVERFLOW, TRUNCATED = oc.NONE, oc.OVERFLOW, oc.TRUNCATED
STRETCHES_MAX = 8


def pick_rounds(b, d, p, window, min_hits, stretches):
    """The rounds on hits given as arrays (any order): [round][(b, cnt, d, p)] in ascending b, before any cut at max_partners."""
    b, d, p = (np.asarray(v, np.int64) for v in (b, d, p))
    order = np.lexsort((p, d, b))
    b, d, p = b[order], d[order], p[order]
    n = len(b)
    key = b * (np.int64(1) << 40) + d
    cnt = np.searchsorted(key, key + window, side="left") - np.arange(n)
    starts = np.nonzero(np.concatenate([[True], b[1:] != b[:-1]]))[0] if n else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [n]]) if n else starts
    live = np.ones(n, bool)
    rounds = []
    for _ in range(stretches):
        cands = []
        for s, e in zip(starts, ends):
            w = np.where(live[s:e], cnt[s:e], 0)
            i = int(s + np.argmax(w))                                    # the first of equal ones; all dead: 0 < min_hits
            c = int(w[i - s])
            if c >= min_hits:
                r = i + c // 2
                cands.append((int(b[r]), c, int(d[r]), int(p[r])))
                live[s:e] &= ~((d[s:e] > d[i] - window) & (d[s:e] < d[i] + window))
        rounds.append(cands)
    return rounds


def job_candidates_multi(index, first, a, Q, step=oc.STEP, window=oc.WINDOW, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS, stretches=1):
    """(status, hits kept, [round][(b, cnt, d, p)]) of one job; b a read id of the DB; every round cut at max_partners."""
    h = oc.job_hits(index, first, a, Q, step, list_)
    if h is None or len(h[0]) == 0:
        return NONE, 0, [[] for _ in range(stretches)]
    b, d, p, over = h
    rounds = pick_rounds(b, d, p, window, min_hits, stretches)
    trunc = any(len(c) > max_partners for c in rounds)
    rounds = [[(bb + first, c, dd, pp) for bb, c, dd, pp in cands[:max_partners]] for cands in rounds]
    if not any(rounds):
        return NONE, len(b), rounds
    return (OVERFLOW if over else 0) | (TRUNCATED if trunc else 0), len(b), rounds


def model_overlap_multi(reads, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
                        block_bases=oc.BLOCK_BASES, max_stretches=1):
    """What hinge_overlap_run_multi answers: overlap_common.model_overlap's tuple and, behind it, round [m]; sorted by (a, b, comp, round)."""
    n = len(reads)
    rows, cnt, dg, rep, status, hits, st, rnd = model_overlap_multi_jobs(reads, range(n), k, step, window, max_occ, list_, max_partners, min_hits, block_bases, max_stretches)
    return rows, cnt, dg, rep, [status[a] for a in range(n)], [hits[a] for a in range(n)], st, rnd


def model_overlap_multi_jobs(reads, picks, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
                             block_bases=oc.BLOCK_BASES, max_stretches=1, indexes=None):
    """model_overlap_multi for the reads `picks` as a only, as overlap_common.model_overlap_jobs: status and hits as
    {a: [forward, complement]}; every block's index is built once (indexes: overlap_common.block_index's dict)."""
    rlen = [len(r) for r in reads]
    picks = sorted(set(int(a) for a in picks))
    status = {a: [NONE, NONE] for a in picks}
    hits = {a: [0, 0] for a in picks}
    rows = []
    st = dict(jobs=0, blocks=0, entries=0, dropped_codes=0, overflow=0, truncated=0)
    Q = {a: (np.asarray(reads[a], np.uint8), oc.revcomp(reads[a])) for a in picks}
    for first, end in oc.blocks(rlen, block_bases):
        index = oc.block_index(reads, first, end, k, max_occ, indexes)
        st["blocks"] += 1; st["entries"] += len(index.codes); st["dropped_codes"] += index.dropped_codes
        for a in picks:
            for comp in (0, 1):
                s, nh, rounds = job_candidates_multi(index, first, a, Q[a][comp], step, window, list_, max_partners, min_hits, max_stretches)
                st["jobs"] += 1
                hits[a][comp] += nh
                if s != NONE:
                    status[a][comp] = (0 if status[a][comp] == NONE else status[a][comp]) | s
                    st["overflow"] += bool(s & OVERFLOW); st["truncated"] += bool(s & TRUNCATED)
                for rnd, cands in enumerate(rounds):
                    for b, c, d, p in cands:
                        dg = oc.diag_of(rlen[a], rlen[b], comp, d)
                        ab, ae, bb, be = oc.project(rlen[a], rlen[b], dg, k)
                        rows.append(((a, b, comp, ab, ae, bb, be), c, dg, (d, p), rnd))
    rows.sort(key=lambda r: r[0][:3] + (r[4],))
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], status, hits, st, [r[4] for r in rows]


# ---- the host program's rules ----------------------------------------------------------------------------------------------------
def canonical(rows, diag, cnt, rlen):
    """[(a, b, comp, diag, cnt, from_a)] with a < b: a candidate found from the larger read is mirrored."""
    out = []
    for r, dg, c in zip(rows, diag, cnt):
        a, b, comp = int(r[0]), int(r[1]), int(r[2])
        if a < b:
            out.append((a, b, comp, int(dg), int(c), 1))
        else:
            out.append((b, a, comp, int(oc.alen_blen_mirror(int(rlen[a]), int(rlen[b]), comp, int(dg))), int(c), 0))
    return out


def merge(cands, window=oc.WINDOW):
    """Clusters of canonical candidates -> ([(a, b, comp, diag)] sorted, members merged away)."""
    by_key = {}
    for a, b, comp, dg, c, from_a in cands:
        by_key.setdefault((a, b, comp), []).append((dg, c, from_a))
    out, merged = [], 0
    for key in sorted(by_key):
        m = sorted(by_key[key])
        dgs = np.asarray([x[0] for x in m], np.int64)
        cuts = np.nonzero(np.diff(dgs) >= window)[0] + 1                  # neighbours `window` or more apart: two clusters
        for grp in np.split(np.arange(len(m)), cuts):
            best = min((m[i] for i in grp), key=lambda x: (-x[2], -x[1], x[0]))
            out.append(key + (best[0],))
            merged += len(grp) - 1
    return out, merged


def drop_duplicates(records, window=oc.WINDOW):
    """records [(a, b, comp, abpos, aepos, bbpos, bepos)] -> (kept, sorted by (a, b, comp, abpos, bbpos); dropped count)."""
    by_key = {}
    for r in records:
        by_key.setdefault(tuple(r[:3]), []).append(tuple(int(v) for v in r[3:7]))
    kept, dropped = [], 0
    for key in sorted(by_key):
        mine = []
        for ab, ae, bb, be in sorted(by_key[key], key=lambda q: (-(q[1] - q[0]), q[0], q[2])):
            dup = False
            for kab, kae, kbb, kbe in mine:
                inter = min(ae, kae) - max(ab, kab)
                near = min(abs((bb - ab) - (kbb - kab)), abs((be - ae) - (kbe - kae)))
                if 2 * inter > min(ae - ab, kae - kab) and near < window:
                    dup = True
                    break
            if dup:
                dropped += 1
            else:
                mine.append((ab, ae, bb, be))
        kept += [key + q for q in mine]
    kept.sort(key=lambda r: (r[0], r[1], r[2], r[3], r[5]))
    return kept, dropped


def mirror_record(r, rlen):
    """The same stretch seen from read b: the end points swapped (in the comp frame: counted from the other end)."""
    a, b, comp, ab, ae, bb, be = (int(v) for v in r)
    if not comp:
        return (b, a, comp, bb, be, ab, ae)
    alen, blen = int(rlen[a]), int(rlen[b])
    return (b, a, comp, blen - be, blen - bb, alen - ae, alen - ab)


def program_records(reads, min_len=1000, max_stretches=1, **kw):
    """What `hinge overlap --max-stretches S` writes where the alignment is the projection (noise-free reads whose overlaps end at
    read ends): (records sorted by (a, b, comp, abpos, bbpos), candidates per round, clusters merged away, duplicates dropped)."""
    rlen = [len(r) for r in reads]
    rows, cnt, dg, rep, status, hits, st, rnd = model_overlap_multi(reads, max_stretches=max_stretches, **kw)
    clusters, merged = merge(canonical(rows, dg, cnt, rlen), kw.get("window", oc.WINDOW))
    recs = []
    for a, b, comp, d in clusters:
        q = oc.project(rlen[a], rlen[b], d, kw.get("k", oc.K))
        if q is not None and q[1] - q[0] >= min_len and q[3] - q[2] >= min_len:
            recs.append((a, b, comp) + q)
    kept, dropped = drop_duplicates(recs, kw.get("window", oc.WINDOW))
    both = sorted(kept + [mirror_record(r, rlen) for r in kept], key=lambda r: (r[0], r[1], r[2], r[3], r[5]))
    return both, [rnd.count(x) for x in range(max_stretches)], merged, dropped


# ---- the generator's ground truth for a two-copy repeat (hinge_amd.synth_draft, linear genome) ----------------------------------------
def _pos(d, r, x):
    """Where genome coordinate x lies in stored read r: the genome offset scaled by read length over interval length."""
    ln, g0, g1 = len(d.reads[r]), int(d.g0[r]), int(d.g1[r])
    t = (x - g0) * ln / (g1 - g0)
    return ln - t if d.strand[r] else t


def expected_stretches(d, margin=100, min_shared=2_000):
    """[(a, b, comp, kind, abpos, aepos, bbpos, bepos)] over ordered pairs: kind 'cross' - read a holds one copy whole with `margin`
    bases to spare at both ends and read b holds the other copy likewise: the copy of a against the other copy of b - and, for such a
    pair, kind 'main' if the genome intervals share >= min_shared bases (the generator's record).  Positions in the record's frame."""
    L, c1, c2 = d.spec.repeat
    n = len(d.reads)
    truth = oc.rec_rows(d)
    out = []
    for a in range(n):
        for b in range(n):
            if a == b:
                continue
            comp = int(d.strand[a] != d.strand[b])
            blen = len(d.reads[b])
            n_cross = 0
            for ca, cb in ((c1, c2), (c2, c1)):
                if d.g0[a] <= ca - margin and ca + L + margin <= d.g1[a] and d.g0[b] <= cb - margin and cb + L + margin <= d.g1[b]:
                    pa = sorted((_pos(d, a, ca), _pos(d, a, ca + L)))
                    fb = [blen - _pos(d, b, x) if comp else _pos(d, b, x) for x in (cb, cb + L)]
                    fb.sort()
                    out.append((a, b, comp, "cross", pa[0], pa[1], fb[0], fb[1]))
                    n_cross += 1
            if n_cross and oc.shared_bases(d, a, b) >= min_shared:
                out.append((a, b, comp, "main") + tuple(float(v) for v in truth[(a, b, comp)]))
    return out


# ---- the planted reads the host test and the GPU test share -------------------------------------------------------------------------
def planted_reads(seed=21, window=oc.WINDOW):
    """Reads of 300 .. 1 500 random bases whose pairs overlap in more than one stretch; (reads, names -> index in the list).
      xy0 = X U Y, xy1 = Y V X            two stretches, diagonals |Y| + |V| and -(|X| + |U|)
      rc0, rc1                            the same with the second read stored reverse-complemented
      rep0 = L R M R N, rep1 = L' R M R N'  a main diagonal and two cross ones, |R| + |M| to either side
      win0 = X U Y, win1 = X U' Y         |U'| = |U| + window: the second stretch's diagonal exactly `window` from the first's
      wim0, wim1                          |U'| = |U| + window - 1"""
    rng = np.random.default_rng(seed)
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cat = lambda *a: np.concatenate(a).astype(np.uint8)
    reads, names = [], {}

    def add(name, r):
        names[name] = len(reads)
        reads.append(np.asarray(r, np.uint8))
    X, U, Y, V = j(400), j(330), j(370), j(310)
    add("xy0", cat(X, U, Y)); add("xy1", cat(Y, V, X))
    X, U, Y, V = j(380), j(300), j(420), j(350)
    add("rc0", cat(X, U, Y)); add("rc1", oc.revcomp(cat(Y, V, X)))
    R, M = j(300), j(320)
    add("rep0", cat(j(120), R, M, R, j(150))); add("rep1", cat(j(200), R, M, R, j(90)))
    for name, extra in (("win", window), ("wim", window - 1)):
        X, Y = j(350), j(360)
        add(name + "0", cat(X, j(300), Y)); add(name + "1", cat(X, j(300 + extra), Y))
    return reads, names


def multi_reads():
    """overlap_common.edge_reads() and the planted reads behind them; (reads, names of both)."""
    reads, names = oc.edge_reads()
    more, mn = planted_reads()
    names = dict(names, **{k: v + len(reads) for k, v in mn.items()})
    return reads + more, names
