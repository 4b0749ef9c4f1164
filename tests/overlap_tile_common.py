"""Shared by the `hinge overlap --tile` tests and tools: the numpy model behind hinge_overlap_run_tiled, on top of
overlap_common and written from the rule, not from the kernels.

  tiles     T a power of two 64 .. 8192, T <= list * step; adv = T // 2.  The sampled positions of a read are the global ones,
            p = j * step <= alen - k.  Tile t holds those with t * adv <= p < t * adv + T; one tile if alen - k + 1 <= T or alen < k,
            else ceil((alen - k + 1 - T) / adv) + 1
  per tile  overlap_common's job rule on the tile's positions: hits (b, d, p) with d in the whole read's frame, self hits out first,
            enumerated by p then gpos and cut at `list`; groups, picks and candidates as there
  reduce    per (read, strand, block) over the tiles: per b the tile candidate of the largest cnt, of equal ones the lowest tile;
            ascending b, the first max_partners.  NONE without a candidate; else OVERFLOW if any tile dropped hits, TRUNCATED if any
            tile was or more than max_partners distinct b remain; hits = the sum of the tiles' kept hits
"""
import numpy as np

import overlap_common as oc
import seed_common as sm

TILE, TILE_MIN, TILE_MAX = 8192, 64, 8192
READ_MAX = (1 << 30) - 1
NONE, OVERFLOW, TRUNCATED = oc.NONE, oc.OVERFLOW, oc.TRUNCATED


def tile_count(alen, k, tile):
    L = alen - k + 1
    if alen < k or L <= tile:
        return 1
    adv = tile // 2
    return -((L - tile) // -adv) + 1


def blocks(rlen, block_bases=oc.BLOCK_BASES, reads_max=(1 << 20) - 1):
    """overlap_common.blocks, cut at reads_max reads as well."""
    out, first, bases = [], 0, 0
    for r, ln in enumerate(rlen):
        if r > first and (bases + int(ln) > block_bases or r - first == reads_max):
            out.append((first, r))
            first, bases = r, 0
        bases += int(ln)
    if len(rlen):
        out.append((first, len(rlen)))
    return out


def query_hits(index, first, a, Q, step):
    """Every hit of the (read, strand) against the block, before tiles and lists: (b, d, p) by p then gpos, self hits out; None for
    a read shorter than k."""
    k, alen = index.k, len(Q)
    if alen < k:
        return None
    p = np.arange(0, alen - k + 1, step, dtype=np.int64)
    codes = sm.kmer_codes(Q, k)[p]
    lo = np.searchsorted(index.codes, codes, side="left")
    hi = np.searchsorted(index.codes, codes, side="right")
    occ = hi - lo
    total = int(occ.sum())
    pp = np.repeat(p, occ)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(occ) - occ, occ)
    g = index.gpos[np.repeat(lo, occ) + within].astype(np.int64) if total else np.zeros(0, np.int64)
    b = np.searchsorted(index.off, g, side="right") - 1
    keep = (b + first) != a
    pp, g, b = pp[keep], g[keep], b[keep]
    return b, g - index.off[b] - pp + alen, pp


def candidates_of(b, d, p, over, first, window, max_partners, min_hits):
    """overlap_common.job_candidates from a hit list already cut: (status, hits kept, [(b, cnt, d, p)])."""
    n = len(b)
    if n == 0:
        return NONE, 0, []
    order = np.lexsort((p, d, b))
    b, d, p = b[order], d[order], p[order]
    key = b * (np.int64(1) << 40) + d
    cnt = np.searchsorted(key, key + window, side="left") - np.arange(n)
    starts = np.nonzero(np.concatenate([[True], b[1:] != b[:-1]]))[0]
    ends = np.concatenate([starts[1:], [n]])
    cands = []
    for s, e in zip(starts, ends):
        i = int(s + np.argmax(cnt[s:e]))
        c = int(cnt[i])
        if c >= min_hits:
            r = i + c // 2
            cands.append((int(b[r]) + first, c, int(d[r]), int(p[r])))
    trunc = len(cands) > max_partners
    cands = cands[:max_partners]
    if not cands:
        return NONE, n, []
    return (OVERFLOW if over else 0) | (TRUNCATED if trunc else 0), n, cands


def job_tiles(index, first, a, Q, tile=TILE, step=oc.STEP, window=oc.WINDOW, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS):
    """[(status, hits kept, dropped, [(b, cnt, d, p)])] of the job's tiles."""
    nt = tile_count(len(Q), index.k, tile)
    h = query_hits(index, first, a, Q, step)
    if h is None:
        return [(NONE, 0, False, [])]
    b, d, p = h
    adv = tile // 2
    out = []
    for t in range(nt):
        lo, hi = np.searchsorted(p, t * adv, side="left"), np.searchsorted(p, t * adv + tile, side="left")
        over = hi - lo > list_
        hi = min(hi, lo + list_)
        st, nh, cands = candidates_of(b[lo:hi], d[lo:hi], p[lo:hi], over, first, window, max_partners, min_hits)
        out.append((st, nh, bool(over), cands))
    return out


def reduce_tiles(tiles, max_partners=oc.MAX_PARTNERS):
    """(status, hits, [(b, cnt, d, p)]) of a job from job_tiles' list."""
    best = {}
    for st, nh, over, cands in tiles:                                    # ascending tile: of equal counts the first stays
        for c in cands:
            if c[0] not in best or c[1] > best[c[0]][1]:
                best[c[0]] = c
    hits = sum(t[1] for t in tiles)
    if not best:
        return NONE, hits, []
    cands = [best[b] for b in sorted(best)]
    status = 0
    if any(t[2] for t in tiles):
        status |= OVERFLOW
    if len(cands) > max_partners or any(t[0] != NONE and t[0] & TRUNCATED for t in tiles):
        status |= TRUNCATED
    return status, hits, cands[:max_partners]


def model_overlap_tiled(reads, tile=TILE, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
                        block_bases=oc.BLOCK_BASES, picks=None, indexes=None):
    """What hinge_overlap_run_tiled answers, in overlap_common.model_overlap's form: (rows [m][7], count [m], diag [m], rep [m] =
    (d, p), status [n][2], hits [n][2], stats).  stats has model_overlap's entries and tiles, multi_tile_jobs, max_tile_hits.
    picks: only those reads as a (status and hits then hold NONE / 0 for the others)."""
    assert TILE_MIN <= tile <= TILE_MAX and tile & (tile - 1) == 0 and tile <= list_ * step
    n = len(reads)
    rlen = [len(r) for r in reads]
    picks = range(n) if picks is None else sorted(set(int(a) for a in picks))
    status = [[NONE, NONE] for _ in range(n)]
    hits = [[0, 0] for _ in range(n)]
    rows = []
    st = dict(jobs=0, blocks=0, entries=0, dropped_codes=0, overflow=0, truncated=0, tiles=0, multi_tile_jobs=0, max_tile_hits=0)
    for first, end in blocks(rlen, block_bases):
        index = oc.block_index(reads, first, end, k, max_occ, indexes)
        st["blocks"] += 1; st["entries"] += len(index.codes); st["dropped_codes"] += index.dropped_codes
        for a in picks:
            for comp in (0, 1):
                Q = oc.revcomp(reads[a]) if comp else np.asarray(reads[a], np.uint8)
                tiles = job_tiles(index, first, a, Q, tile, step, window, list_, max_partners, min_hits)
                s, nh, cands = reduce_tiles(tiles, max_partners)
                st["jobs"] += 1; st["tiles"] += len(tiles); st["multi_tile_jobs"] += len(tiles) > 1
                st["max_tile_hits"] = max([st["max_tile_hits"]] + [t[1] for t in tiles])
                hits[a][comp] += nh
                if s != NONE:
                    status[a][comp] = (0 if status[a][comp] == NONE else status[a][comp]) | s
                    st["overflow"] += bool(s & OVERFLOW); st["truncated"] += bool(s & TRUNCATED)
                for b, c, d, p in cands:
                    dg = oc.diag_of(rlen[a], rlen[b], comp, d)
                    ab, ae, bb, be = oc.project(rlen[a], rlen[b], dg, k)
                    rows.append(((a, b, comp, ab, ae, bb, be), c, dg, (d, p)))
    rows.sort(key=lambda r: r[0][:3])
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], status, hits, st
