"""Shared by the `hinge overlap --tile T --tile-stretches S` tests and tools: the numpy model behind hinge_overlap_run_tiled_multi
(DESIGN.md 3.15), on top of overlap_common, overlap_multi_common and overlap_tile_common and written from the rule, not from the
kernels.

  per tile  overlap_tile_common's tile job - the same positions, self-hit rule and cut at `list` - and on its hits
            overlap_multi_common.pick_rounds: S rounds of pick and suppress, every round cut at max_partners (TRUNCATED)
  reduce    per (read, strand, block) over all sections of all tile rows.  Round r's pick of b: its live tile candidate of the
            largest cnt, of equal ones the lowest tile's, within a tile the lowest section's.  Afterwards every tile candidate of b
            with |d - d_pick| < window is dead.  S rounds; a b without a live candidate has none later.  Round r keeps the first
            max_partners partners in ascending b.  NONE without a candidate; else OVERFLOW if any tile dropped hits, TRUNCATED if
            any tile row was or a round has more than max_partners partners; hits = the sum of the tiles' kept hits
"""
import numpy as np

import overlap_common as oc
import overlap_multi_common as omc
import overlap_tile_common as otc

NONE, OVERFLOW, TRUNCATED = oc.NONE, oc.OVERFLOW, oc.TRUNCATED
STRETCHES_MAX = omc.STRETCHES_MAX


def job_tiles_multi(index, first, a, Q, tile=otc.TILE, step=oc.STEP, window=oc.WINDOW, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS, stretches=1):
    """[(status, hits kept, dropped, [round][(b, cnt, d, p)])] of the job's tiles; b a read id of the DB."""
    nt = otc.tile_count(len(Q), index.k, tile)
    h = otc.query_hits(index, first, a, Q, step)
    if h is None:
        return [(NONE, 0, False, [[] for _ in range(stretches)])]
    b, d, p = h
    adv = tile // 2
    out = []
    for t in range(nt):
        lo, hi = np.searchsorted(p, t * adv, side="left"), np.searchsorted(p, t * adv + tile, side="left")
        over = bool(hi - lo > list_)
        hi = min(hi, lo + list_)
        rounds = omc.pick_rounds(b[lo:hi], d[lo:hi], p[lo:hi], window, min_hits, stretches) if hi > lo else [[] for _ in range(stretches)]
        trunc = any(len(c) > max_partners for c in rounds)
        rounds = [[(bb + first, c, dd, pp) for bb, c, dd, pp in cands[:max_partners]] for cands in rounds]
        st = NONE if not any(rounds) else (OVERFLOW if over else 0) | (TRUNCATED if trunc else 0)
        out.append((st, int(hi - lo), over, rounds))
    return out


def reduce_tiles_multi(tiles, window=oc.WINDOW, max_partners=oc.MAX_PARTNERS, stretches=1):
    """(status, hits, [round][(b, cnt, d, p)]) of a job from job_tiles_multi's list."""
    by_b = {}
    for t, (st, nh, over, rounds) in enumerate(tiles):
        for sec, cands in enumerate(rounds):
            for b, c, d, p in cands:
                by_b.setdefault(b, []).append((-c, t, sec, d, p))
    out = [[] for _ in range(stretches)]
    for b in sorted(by_b):
        live = by_b[b]
        for r in range(stretches):
            if not live:
                break
            c, t, sec, d, p = min(live)                                  # the largest cnt, the lowest tile, the lowest section
            out[r].append((b, -c, d, p))
            live = [x for x in live if abs(x[3] - d) >= window]
    hits = sum(t[1] for t in tiles)
    if not out[0]:
        return NONE, hits, out
    status = 0
    if any(t[2] for t in tiles):
        status |= OVERFLOW
    if any(len(c) > max_partners for c in out) or any(t[0] != NONE and t[0] & TRUNCATED for t in tiles):
        status |= TRUNCATED
    return status, hits, [c[:max_partners] for c in out]


def model_overlap_tiled_multi(reads, tile=otc.TILE, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
                              block_bases=oc.BLOCK_BASES, max_stretches=1, picks=None, indexes=None):
    """What hinge_overlap_run_tiled_multi answers: overlap_tile_common.model_overlap_tiled's tuple and, behind it, round [m];
    sorted by (a, b, comp, round)."""
    assert otc.TILE_MIN <= tile <= otc.TILE_MAX and tile & (tile - 1) == 0 and tile <= list_ * step and 1 <= max_stretches <= STRETCHES_MAX
    n = len(reads)
    rlen = [len(r) for r in reads]
    picks = range(n) if picks is None else sorted(set(int(a) for a in picks))
    status = [[NONE, NONE] for _ in range(n)]
    hits = [[0, 0] for _ in range(n)]
    rows = []
    st = dict(jobs=0, blocks=0, entries=0, dropped_codes=0, overflow=0, truncated=0, tiles=0, multi_tile_jobs=0, max_tile_hits=0)
    for first, end in otc.blocks(rlen, block_bases):
        index = oc.block_index(reads, first, end, k, max_occ, indexes)
        st["blocks"] += 1; st["entries"] += len(index.codes); st["dropped_codes"] += index.dropped_codes
        for a in picks:
            for comp in (0, 1):
                Q = oc.revcomp(reads[a]) if comp else np.asarray(reads[a], np.uint8)
                tiles = job_tiles_multi(index, first, a, Q, tile, step, window, list_, max_partners, min_hits, max_stretches)
                s, nh, rounds = reduce_tiles_multi(tiles, window, max_partners, max_stretches)
                st["jobs"] += 1; st["tiles"] += len(tiles); st["multi_tile_jobs"] += len(tiles) > 1
                st["max_tile_hits"] = max([st["max_tile_hits"]] + [t[1] for t in tiles])
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


def stretches_missed(d, rows, diag, window=oc.WINDOW, expected=None):
    """The expected stretches (overlap_multi_common.expected_stretches) without a candidate of their key within `window`
    diagonals: [(a, b, comp, kind, ...)]."""
    expected = omc.expected_stretches(d) if expected is None else expected
    by_key = {}
    for r, dg in zip(rows, diag):
        by_key.setdefault((int(r[0]), int(r[1]), int(r[2])), []).append(int(dg))
    missed = []
    for e in expected:
        a, b, comp, kind, ab, ae, bb, be = e
        if not any(abs(dg - (bb - ab)) < window for dg in by_key.get((a, b, comp), [])):                # (the criterion of tests/test_overlap_multi_model.py)
            missed.append(e)
    return missed
