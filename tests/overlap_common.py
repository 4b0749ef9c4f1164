"""Shared by the `hinge overlap` tests and tools: the numpy model behind hinge_overlap_run and the host program,
written from the rule and not from the kernel: numpy's searchsorted / lexsort / argmax where the kernel has fixed-trip searches, a
bitonic sort, a segmented scan and ballots.

  blocks    the reads in blocks of consecutive ids of at most block_bases bases (a longer read: alone); per block the index of
            seed_common.Index over the block's reads (a code with more than max_occ entries in the block has none)
  job       one per (read a, strand, block); Q = read a in the strand's frame, alen its length; sampled positions as in seed_common.
            Hits (b, d, p): b = the read holding gpos, d = (gpos - off[b]) - p + alen; hits with b == a are discarded first, the rest
            is enumerated by p then gpos and cut at `list` (OVERFLOW)
  groups    hits sorted by (b, d, p); cnt[i] = elements j >= i of the same b with d[j] < d[i] + window; per b the largest cnt, of equal
            ones the smallest i; representative = element i + cnt[i] // 2; a candidate (b, cnt, d, p) if cnt >= min_hits
  partners  ascending b, the first max_partners (TRUNCATED beyond)
  record    A = a forward, B = b in the comp frame: diag = bbpos - abpos = d - alen (forward), blen - d (complement); both reads whole
            along it, clamped to both
  mirror    of (a, b, comp, diag): (b, a, comp, -diag) forward, (b, a, comp, alen - blen + diag) complement
"""
import numpy as np

import seed_common as sm

NONE, OVERFLOW, TRUNCATED = 1, 2, 4
K, STEP, WINDOW, MAX_OCC, LIST, MAX_PARTNERS, MIN_HITS, BLOCK_BASES = 15, 2, 256, 64, 4096, 64, 6, 16 << 20      # MIN_HITS: HINGE_OVERLAP_MIN_HITS (tools/overlap_measure.py min-hits)
READ_MAX = (1 << 20) - 1
revcomp = sm.revcomp


def blocks(rlen, block_bases=BLOCK_BASES):
    """[(first, end)] of the blocks."""
    out, first, bases = [], 0, 0
    for r, ln in enumerate(rlen):
        if r > first and bases + int(ln) > block_bases:
            out.append((first, r))
            first, bases = r, 0
        bases += int(ln)
    if len(rlen):
        out.append((first, len(rlen)))
    return out


def job_hits(index, first, a, Q, step=STEP, list_=LIST, keep_self=False):
    """(b, d, p, overflow) of the block-local target, in enumeration order, cut at `list`; None for a read shorter than k.
    keep_self: what the list would hold if self hits took slots (for tests that show they do not)."""
    k, alen = index.k, len(Q)
    if alen < k:
        return None
    s = sm.stride(alen, k, step, list_)
    p = np.arange(0, alen - k + 1, s, dtype=np.int64)
    codes = sm.kmer_codes(Q, k)[p]
    lo = np.searchsorted(index.codes, codes, side="left")
    hi = np.searchsorted(index.codes, codes, side="right")
    occ = hi - lo
    total = int(occ.sum())
    pp = np.repeat(p, occ)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(occ) - occ, occ)
    g = index.gpos[np.repeat(lo, occ) + within] if total else np.zeros(0, np.int64)
    b = np.searchsorted(index.off, g, side="right") - 1
    keep = ((b + first) != a) | keep_self                                # self hits take no slot
    pp, g, b = pp[keep], g[keep], b[keep]
    over = len(pp) > list_
    pp, g, b = pp[:list_], g[:list_], b[:list_]
    return b, g - index.off[b] - pp + alen, pp, over


def job_candidates(index, first, a, Q, step=STEP, window=WINDOW, list_=LIST, max_partners=MAX_PARTNERS, min_hits=MIN_HITS):
    """(status, hits kept, [(b, cnt, d, p)]) of one job; b a read id of the DB."""
    h = job_hits(index, first, a, Q, step, list_)
    if h is None or len(h[0]) == 0:
        return NONE, 0, []
    b, d, p, over = h
    order = np.lexsort((p, d, b))
    b, d, p = b[order], d[order], p[order]
    n = len(b)
    big = np.int64(1) << 40                                              # beyond any d + window
    key = b * big + d
    cnt = np.searchsorted(key, key + window, side="left") - np.arange(n)
    starts = np.nonzero(np.concatenate([[True], b[1:] != b[:-1]]))[0]
    ends = np.concatenate([starts[1:], [n]])
    cands = []
    for s, e in zip(starts, ends):
        i = int(s + np.argmax(cnt[s:e]))                                 # the first of equal ones
        c = int(cnt[i])
        if c >= min_hits:
            r = i + c // 2
            cands.append((int(b[r]) + first, c, int(d[r]), int(p[r])))
    trunc = len(cands) > max_partners
    cands = cands[:max_partners]
    if not cands:
        return NONE, n, []
    return (OVERFLOW if over else 0) | (TRUNCATED if trunc else 0), n, cands


def diag_of(alen, blen, comp, d):
    return blen - d if comp else d - alen


def project(alen, blen, diag, k=K):
    """(abpos, aepos, bbpos, bepos) of both reads whole along the record-frame diagonal, or None."""
    ab, ae = max(0, -diag), min(alen, blen - diag)
    if ae - ab < k:
        return None
    return ab, ae, ab + diag, ae + diag


def block_index(reads, first, end, k, max_occ, indexes=None):
    """seed_common.Index of the block's reads; indexes: a dict that keeps it for the next caller (a block set's takes a second to build)."""
    key = (first, end, k, max_occ)
    if indexes is None:
        return sm.Index(reads[first:end], k, max_occ)
    if key not in indexes:
        indexes[key] = sm.Index(reads[first:end], k, max_occ)
    return indexes[key]


def three_blocks(rlen):
    """A block_bases that cuts the reads into exactly three blocks: a third of the bases and the longest read on top."""
    bb = sum(rlen) // 3 + max(rlen)
    assert len(blocks(rlen, bb)) == 3
    return bb


def model_overlap(reads, k=K, step=STEP, window=WINDOW, max_occ=MAX_OCC, list_=LIST, max_partners=MAX_PARTNERS, min_hits=MIN_HITS, block_bases=BLOCK_BASES):
    """What hinge_overlap_run answers: (rows [m][7], count [m], diag [m], rep [m] = (d, p), status [n][2], hits [n][2], stats)."""
    n = len(reads)
    rows, cnt, dg, rep, status, hits, st = model_overlap_jobs(reads, range(n), k, step, window, max_occ, list_, max_partners, min_hits, block_bases)
    return rows, cnt, dg, rep, [status[a] for a in range(n)], [hits[a] for a in range(n)], st


def model_overlap_jobs(reads, picks, k=K, step=STEP, window=WINDOW, max_occ=MAX_OCC, list_=LIST, max_partners=MAX_PARTNERS, min_hits=MIN_HITS, block_bases=BLOCK_BASES, indexes=None):
    """model_overlap for the reads `picks` as a only (against every block, both strands): the rows of those a, status and hits as
    {a: [forward, complement]}; of the stats, blocks / entries / dropped_codes are the whole call's, jobs / overflow / truncated
    count the picked jobs.  Every block's index is built once (indexes: block_index's dict)."""
    rlen = [len(r) for r in reads]
    picks = sorted(set(int(a) for a in picks))
    status = {a: [NONE, NONE] for a in picks}
    hits = {a: [0, 0] for a in picks}
    rows = []
    st = dict(jobs=0, blocks=0, entries=0, dropped_codes=0, overflow=0, truncated=0)
    Q = {a: (np.asarray(reads[a], np.uint8), revcomp(reads[a])) for a in picks}
    for first, end in blocks(rlen, block_bases):
        index = block_index(reads, first, end, k, max_occ, indexes)
        st["blocks"] += 1; st["entries"] += len(index.codes); st["dropped_codes"] += index.dropped_codes
        for a in picks:
            for comp in (0, 1):
                s, nh, cands = job_candidates(index, first, a, Q[a][comp], step, window, list_, max_partners, min_hits)
                st["jobs"] += 1
                hits[a][comp] += nh
                if s != NONE:
                    status[a][comp] = (0 if status[a][comp] == NONE else status[a][comp]) | s
                    st["overflow"] += bool(s & OVERFLOW); st["truncated"] += bool(s & TRUNCATED)
                for b, c, d, p in cands:
                    dg = diag_of(rlen[a], rlen[b], comp, d)
                    ab, ae, bb, be = project(rlen[a], rlen[b], dg, k)
                    rows.append(((a, b, comp, ab, ae, bb, be), c, dg, (d, p)))
    rows.sort(key=lambda r: r[0][:3])
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], status, hits, st


def symmetrise(rows, diag, rlen, k=K):
    """rows plus, for every (a, b, comp) without its mirror, (b, a, comp) along the mirrored diagonal; sorted by (a, b, comp).
    Returns (rows, diag, number added)."""
    have = {tuple(r[:3]): (tuple(r), int(dg)) for r, dg in zip(rows, diag)}
    added = 0
    for (a, b, comp), (r, dg) in list(have.items()):
        if (b, a, comp) in have:
            continue
        md = alen_blen_mirror(int(rlen[a]), int(rlen[b]), comp, dg)
        q = project(int(rlen[b]), int(rlen[a]), md, k)
        if q is None:
            continue
        have[(b, a, comp)] = ((b, a, comp) + q, md)
        added += 1
    keys = sorted(have)
    return [have[x][0] for x in keys], [have[x][1] for x in keys], added


def alen_blen_mirror(alen, blen, comp, diag):
    return alen - blen + diag if comp else -diag


def keep_pairs(rows, min_len=1000):
    """The length filter and the pair rule on unaligned rows: a row survives with both lengths >= min_len; a pair only with both of
    its directed rows."""
    ok = {tuple(r[:3]) for r in rows if r[4] - r[3] >= min_len and r[6] - r[5] >= min_len}
    return [r for r in rows if tuple(r[:3]) in ok and (r[1], r[0], r[2]) in ok]


# ---- the generator's ground truth (hinge_amd.synth_draft) ---------------------------------------------------------------------------
def shared_bases(d, a, b):
    """Genome bases the intervals of reads a and b share (linear genomes; negative: the gap between them)."""
    return int(min(d.g1[a], d.g1[b]) - max(d.g0[a], d.g0[b]))


def truth_pairs(d, min_shared):
    """{(a, b, comp)} of all ordered pairs sharing at least min_shared genome bases."""
    out = set()
    n = len(d.reads)
    for a in range(n):
        for b in range(n):
            if a != b and shared_bases(d, a, b) >= min_shared:
                out.add((a, b, int(d.strand[a] != d.strand[b])))
    return out


def rec_rows(d):
    """{(a, b, comp): (abpos, aepos, bbpos, bepos)} of the generator's records."""
    return {(int(q["aread"]), int(q["bread"]), int(q["flags"]) & 1): (int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in d.rec}


# ---- the hand-made set the host test and the GPU test share ------------------------------------------------------------------------------
def edge_reads(seed=9):
    """About 40 reads of 300 .. 1 500 bases cut from a 6 kb genome, either strand, and the special ones; (reads, names -> read id)."""
    rng = np.random.default_rng(seed)
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cat = lambda *a: np.concatenate(a).astype(np.uint8)
    g = j(6000)
    reads, names = [], {}
    for _ in range(30):
        ln = int(rng.integers(300, 1501))
        a = int(rng.integers(0, 6000 - ln + 1))
        r = g[a:a + ln].copy()
        reads.append(revcomp(r) if rng.integers(0, 2) else r)

    def add(name, r):
        names[name] = len(reads)
        reads.append(np.asarray(r, np.uint8))
    add("longest", g[2000:3500].copy())
    add("short", g[100:110].copy())                                      # shorter than k
    add("no_hit", j(400))
    add("twin0", reads[0].copy())                                        # two identical reads (with read 0: three)
    add("twin1", reads[0].copy())
    add("tandem", cat(g[4000:4300], g[4100:4300], g[4300:4600]))         # an internal 200-base tandem copy
    s2 = j(600)                                                          # a pair that overlaps on the complement strand only
    add("comp0", s2[:400].copy())
    add("comp1", revcomp(s2[200:]))
    u = j(100)                                                           # one shared sampled k-mer: a hit count of 1
    add("one0", u)
    add("one1", cat(j(60), u[20:20 + K], j(40)))
    w = j(K + 2 * 63)                                                    # 64 sampled positions, all inside the partner: a hit count of 64
    add("pow0", w)
    add("pow1", cat(j(50), w, j(50)))
    add("tail", g[5000:6000].copy())
    return reads, names


def edge_calls():
    """[(label, keyword arguments of model_overlap)] on edge_reads()."""
    reads, names = edge_reads()
    rlen = [len(r) for r in reads]
    two = three = None
    for bb in range(max(rlen), sum(rlen)):
        bl = blocks(rlen, bb)
        if three is None and len(bl) == 3 and any(e - f == 1 for f, e in bl):
            three = bb
        if two is None and len(bl) == 2:
            two = bb
    assert two and three
    return [("defaults", dict()), ("list64", dict(list_=64)), ("min_hits1", dict(min_hits=1)), ("list64_min_hits1", dict(list_=64, min_hits=1)), ("partners1", dict(max_partners=1)),
            ("two_blocks", dict(block_bases=two)), ("three_blocks", dict(block_bases=three, max_partners=2)), ("step3_window16", dict(step=3, window=16, min_hits=2)),
            ("max_occ2", dict(max_occ=2, min_hits=1))]
