"""`hinge overlap --tile` on the GPU: Context.overlap_run(tile=...) (hinge_overlap_run_tiled: k_overlap_vote_tile and
k_overlap_tile_reduce) value for value against the numpy model (tests/overlap_tile_common.py) - per (read, strand) the status and
the hits kept, per candidate (b, cnt, d, p), its record and its diagonal, and the tile counts of overlap_tile_stats() against the
model's, so that no answer can come from anything but the tiles."""
import os

import numpy as np
import pytest

import overlap_common as oc
import overlap_tile_common as otc
import seed_common as sm
from hinge_amd import formats

pytestmark = pytest.mark.gpu

LONG_LEN = (1 << 20) + 4096 + 37
LONG_KW = dict(step=16, list_=8192)


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


@pytest.fixture(scope="module")
def edge(ctx, tmp_path_factory):
    reads, names = oc.edge_reads()
    return reads, names, str(tmp_path_factory.mktemp("overlap_tile_edge"))


def _set_db(ctx, wd, reads):
    from hinge_amd import capi
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))


def _check(ctx, got, want, label=""):
    pl, count, diag, rep, status, hits = got
    rows, cnt, dg, wrep, wstatus, whits, st = want
    assert status.tolist() == wstatus, label
    assert hits.tolist() == whits, label
    assert [tuple(r) for r in pl.tolist()] == [tuple(int(v) for v in r) for r in rows], label
    assert count.tolist() == cnt and diag.tolist() == dg, label
    assert [tuple(r) for r in rep.tolist()] == wrep, label
    have, tiles = ctx.overlap_stats(), ctx.overlap_tile_stats()
    assert all(have[x] == st[x] for x in ("jobs", "blocks", "entries", "dropped_codes", "overflow", "truncated")), (label, have, st)
    assert all(tiles[x] == st[x] for x in ("tiles", "multi_tile_jobs", "max_tile_hits")), (label, tiles, st)      # the answer came from the tiles
    assert tiles["reduces"] == have["batches"] >= have["blocks"], (label, tiles, have)


def test_edge_set_equals_the_model(ctx, edge):
    reads, names, wd = edge
    cns = _set_db(ctx, wd, reads)
    rlen = [len(r) for r in reads]
    two = next(bb for bb in range(max(rlen), sum(rlen)) if len(oc.blocks(rlen, bb)) == 2)
    three = oc.three_blocks(rlen)
    seen = set()
    calls = [("tile256", dict(tile=256)), ("tile512", dict(tile=512)), ("tile256_step3", dict(tile=256, step=3, window=16, min_hits=2)), ("tile512_step3", dict(tile=512, step=3)),
             ("tile128_list64", dict(tile=128, list_=64, min_hits=1)),                      # (a tile is at most list * step bases)
             ("tile256_list64_step4", dict(tile=256, list_=64, step=4, min_hits=1)),
             ("partners1", dict(tile=256, max_partners=1)), ("partners2", dict(tile=512, max_partners=2)),
             ("two_blocks", dict(tile=256, block_bases=two)), ("three_blocks", dict(tile=512, block_bases=three, max_partners=2))]
    for label, kw in calls:
        want = otc.model_overlap_tiled(reads, **kw)
        got = ctx.overlap_run(**kw)
        _check(ctx, got, want, label)
        seen |= set(got[4].reshape(-1).tolist())
        st = want[6]
        assert st["multi_tile_jobs"] > 50 and st["tiles"] > 2 * st["jobs"], label
        if "list64" in label:
            assert st["overflow"] > 0 and st["max_tile_hits"] == 64, label                 # OVERFLOW in single tiles
        if label.startswith("partners"):
            assert st["truncated"] > 0, label
        if label == "three_blocks":
            assert st["blocks"] == 3 and st["jobs"] == 3 * 2 * len(reads)
        status, hits = got[4], got[5]
        assert status[names["short"]].tolist() == [oc.NONE, oc.NONE] and hits[names["short"]].tolist() == [0, 0]          # shorter than k: one tile, NONE
    assert {0, oc.NONE, oc.OVERFLOW, oc.TRUNCATED} <= seen


def test_batches_keep_a_jobs_tiles_together(ctx, edge, monkeypatch):
    reads, names, wd = edge
    cns = _set_db(ctx, wd, reads)
    want = otc.model_overlap_tiled(reads, tile=256)
    row = 16 + 4 * (4 + 4 * 64)
    monkeypatch.setenv("HINGE_OVERLAP_SCRATCH_BYTES", str(row * 30))                        # about thirty tiles per batch: two or three jobs
    _check(ctx, ctx.overlap_run(tile=256), want, "batches")
    assert ctx.overlap_stats()["batches"] > 20
    monkeypatch.setenv("HINGE_OVERLAP_SCRATCH_BYTES", str(row * 3))                         # fewer than a job's tiles: every job alone
    _check(ctx, ctx.overlap_run(tile=256), want, "one job per batch")
    assert ctx.overlap_stats()["batches"] == 2 * len(reads)
    monkeypatch.delenv("HINGE_OVERLAP_SCRATCH_BYTES")
    monkeypatch.setenv("HINGE_OVERLAP_TILE", "256")                                         # the default from the environment
    _check(ctx, ctx.overlap_run(tiled=True), want, "env")


def test_one_tile_reads_equal_the_whole_read_call(ctx, edge):
    """Every read of the edge set has one tile of 8 192 bases: the tiled call's answer is hinge_overlap_run's, value for value."""
    reads, names, wd = edge
    cns = _set_db(ctx, wd, reads)
    for kw in (dict(), dict(list_=64, min_hits=1, step=128), dict(max_partners=1)):
        plain = ctx.overlap_run(**kw)
        tiled = ctx.overlap_run(tile=8192, **kw)
        for x, y in zip(plain, tiled):
            assert np.array_equal(x, y), kw
        assert ctx.overlap_tile_stats()["tiles"] == ctx.overlap_stats()["jobs"] == 2 * len(reads) and ctx.overlap_tile_stats()["multi_tile_jobs"] == 0
        _check(ctx, tiled, otc.model_overlap_tiled(reads, tile=8192, **kw), str(kw))
    ctx.overlap_run()
    assert ctx.overlap_tile_stats() == dict(tiles=0, multi_tile_jobs=0, max_tile_hits=0, reduces=0)                      # the other calls launch no tile


def test_seam_lengths_and_partners_at_a_seam(ctx, tmp_path):
    """Tile 256 (adv 128), noise-free reads of one genome.  Queries with alen - k + 1 = T - 1, T, T + 1, T + adv, T + adv + 1: one,
    one, two, two and three tiles.  `across`: a partner of 100 shared bases (<= adv) over tile 0's end - tile 0 holds a part of its
    hits, tile 1 all of them, and the whole count comes back.  `inside`: a partner of 90 shared bases inside the half that tiles 1
    and 2 share - equal counts in both, the lower tile's candidate is the answer."""
    T, adv, k = 256, 128, oc.K
    rng = np.random.default_rng(21)
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    g = j(3000)
    seams = [T - 1, T, T + 1, T + adv, T + adv + 1]
    reads = [g[100 * i:100 * i + L + k - 1].copy() for i, L in enumerate(seams)]
    reads += [g[0:900].copy(), oc.revcomp(g[200:800])]                                      # partners of the seam reads
    q = len(reads)
    reads.append(g[1500:2200].copy())                                                      # the query of the two special partners
    across = len(reads)
    reads.append(np.concatenate([j(300), g[1500 + 200:1500 + 300], j(300)]).astype(np.uint8))      # p 200 .. 285 of the query: over 256
    inside = len(reads)
    reads.append(np.concatenate([j(250), g[1500 + 270:1500 + 360], j(250)]).astype(np.uint8))      # p 270 .. 345: inside [256, 384)
    cns = _set_db(ctx, str(tmp_path), reads)
    want = otc.model_overlap_tiled(reads, tile=T)
    got = ctx.overlap_run(tile=T)
    _check(ctx, got, want, "seams")
    assert [otc.tile_count(len(r), k, T) for r in reads[:5]] == [1, 1, 2, 2, 3]
    by_pair = {tuple(r[:3]): (c, tuple(x)) for r, c, x in zip(got[0].tolist(), got[1].tolist(), got[3].tolist())}
    index = sm.Index(reads, k, oc.MAX_OCC)
    tiles = otc.job_tiles(index, 0, q, reads[q], T)
    b, d, p = otc.query_hits(index, 0, q, reads[q], oc.STEP)
    per_tile = lambda x: [next((c[1] for c in t[3] if c[0] == x), 0) for t in tiles]
    whole = int((b == across).sum())
    assert whole >= 43 and per_tile(across)[1] == whole and 6 <= per_tile(across)[0] < whole and 6 <= per_tile(across)[2] < whole       # tiles 0 and 2: a part each
    assert by_pair[(q, across, 0)][0] == whole and 128 <= by_pair[(q, across, 0)][1][1] < 384
    n_in = int((b == inside).sum())
    assert per_tile(inside)[:4] == [0, n_in, n_in, 0] and n_in >= 38
    assert by_pair[(q, inside, 0)] == (n_in, next(c[2:] for c in tiles[1][3] if c[0] == inside))


def test_bad_tiles_are_refused(ctx, edge):
    from hinge_amd import capi
    reads, names, wd = edge
    cns = _set_db(ctx, wd, reads)
    for kw in (dict(tile=100), dict(tile=32), dict(tile=16384), dict(tile=-64), dict(tile=8192, list_=64), dict(tile=512, list_=64, step=7), dict(tile=1 << 30)):
        with pytest.raises(capi.HingeError) as e:
            ctx.overlap_run(**kw)
        assert e.value.code == capi.HINGE_E_ARG, kw
    with pytest.raises(ValueError):
        ctx.overlap_run(tile=256, max_stretches=2)
    ctx.overlap_run(tile=512, list_=64, step=8)                                             # T = list * step: the largest allowed


def test_a_read_of_more_than_2_20_bases(ctx, tmp_path):
    """One random read of 2^20 + 4 133 bases and six noise-free reads of 1 .. 3 kb cut from its start, from across base 2^20 and from
    its last bases, on both strands; step 16, tile 8 192, list 8 192.  The short queries need d = (position in the long read) - p +
    alen above 2^20 - the 31-bit field -, the long query needs its 257 tiles.  hinge_overlap_run still refuses the DB."""
    from hinge_amd import capi
    rng = np.random.default_rng(20)
    big = rng.integers(0, 4, size=LONG_LEN, dtype=np.uint8)
    cuts = [(0, 1000, 0), (500, 3000, 1), ((1 << 20) - 700, 2000, 0), ((1 << 20) - 1500, 3000, 1), (LONG_LEN - 1200, 1200, 0), (LONG_LEN - 2500, 2500, 1)]
    reads = [big[a:a + n].copy() if not c else oc.revcomp(big[a:a + n]) for a, n, c in cuts]
    reads.insert(2, big)                                                                   # (the long read in the middle of the block)
    L = 2
    cns = _set_db(ctx, str(tmp_path), reads)
    want = otc.model_overlap_tiled(reads, tile=8192, **LONG_KW)
    got = ctx.overlap_run(tile=8192, **LONG_KW)
    _check(ctx, got, want, "long")
    assert want[6]["tiles"] == 2 * (otc.tile_count(LONG_LEN, oc.K, 8192) + 6) and otc.tile_count(LONG_LEN, oc.K, 8192) == 257
    pairs = {tuple(r[:3]): x for r, x in zip(got[0].tolist(), got[3].tolist())}
    for s, (a, n, c) in zip([0, 1, 3, 4, 5, 6], cuts):                                      # both directions, on the strand of the cut
        assert (s, L, c) in pairs and (L, s, c) in pairs, (s, c)
        row = next(r for r in got[0].tolist() if tuple(r[:3]) == (s, L, c))
        assert row[3:5] == [0, n] and row[6] - row[5] == n                                  # the short read whole, noise-free
        assert row[5] == (LONG_LEN - a - n if c else a)
    assert max(x[0] for (a, b, c), x in pairs.items() if b == L) > 1 << 20                  # d beyond the 21 bits of hinge_overlap_run's key
    ctx.profile_enable(64)
    with pytest.raises(capi.HingeError) as e:
        ctx.overlap_run(**LONG_KW)
    assert e.value.code == capi.HINGE_E_CAPACITY
    rep = ctx.profile_report()
    assert rep.get("k_overlap_vote", (0.0, 0))[1] == 0 and rep.get("k_overlap_vote_tile", (0.0, 0))[1] == 0
    ctx.overlap_run(tile=8192, **LONG_KW)
    rep = ctx.profile_report()
    assert rep["k_overlap_vote_tile"][1] == 1 and rep["k_overlap_tile_reduce"][1] == 1     # the profiler ids of both kernels
