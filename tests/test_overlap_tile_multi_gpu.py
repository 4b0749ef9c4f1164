"""`hinge overlap --tile T --tile-stretches S` on the GPU: Context.overlap_run(tile=..., tile_stretches=...)
(hinge_overlap_run_tiled_multi: k_overlap_vote_tile_multi and k_overlap_tile_reduce_multi) value for value against the numpy model
(tests/overlap_tile_multi_common.py) - per (read, strand) the status and the hits kept, per candidate (b, cnt, d, p), its round, its
record and its diagonal, and the tile counts of overlap_tile_stats() against the model's - and against the two calls it joins:
hinge_overlap_run_tiled at one round, hinge_overlap_run_multi on reads of one tile."""
import os

import numpy as np
import pytest

import overlap_common as oc
import overlap_multi_common as omc
import overlap_tile_common as otc
import overlap_tile_multi_common as otm
from hinge_amd import formats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


def _set_db(ctx, wd, reads):
    from hinge_amd import capi
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))


@pytest.fixture(scope="module")
def multi(tmp_path_factory):
    reads, names = omc.multi_reads()
    return reads, names, str(tmp_path_factory.mktemp("overlap_tile_multi"))


@pytest.fixture(scope="module")
def models(multi):
    """The model's answers on multi_reads(), computed once per setting and shared; every block's index is built once."""
    reads = multi[0]
    cache, indexes = {}, {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = otm.model_overlap_tiled_multi(reads, indexes=indexes, **kw)
        return cache[key]
    return get


def _kw(kw):
    """The model's keywords as overlap_run's."""
    kw = dict(kw)
    kw["tile_stretches"] = kw.pop("max_stretches")
    return kw


def _check(ctx, got, want, label=""):
    pl, count, diag, rep, status, hits, rnd = got
    rows, cnt, dg, wrep, wstatus, whits, st, wrnd = want
    assert status.tolist() == wstatus, label
    assert hits.tolist() == whits, label
    assert [tuple(r) for r in pl.tolist()] == [tuple(int(v) for v in r) for r in rows], label
    assert count.tolist() == cnt and diag.tolist() == dg, label
    assert [tuple(r) for r in rep.tolist()] == wrep, label
    assert rnd.tolist() == wrnd, label
    have, tiles = ctx.overlap_stats(), ctx.overlap_tile_stats()
    assert all(have[x] == st[x] for x in ("jobs", "blocks", "entries", "dropped_codes", "overflow", "truncated")), (label, have, st)
    assert all(tiles[x] == st[x] for x in ("tiles", "multi_tile_jobs", "max_tile_hits")), (label, tiles, st)      # the answer came from the tiles
    assert tiles["reduces"] == have["batches"] >= have["blocks"], (label, tiles, have)


def _by_pair(got):
    out = {}
    for r, g, rd in zip(got[0].tolist(), got[2].tolist(), got[6].tolist()):
        out.setdefault(tuple(r[:3]), []).append((rd, g))
    return out


def test_multi_reads_equal_the_model(ctx, multi, models):
    """tile 256 and 512, 2 and 3 rounds, step 2 and 3.  At tile 256 no tile of rep0 holds all three diagonals of rep1."""
    reads, names, wd = multi
    cns = _set_db(ctx, wd, reads)
    for tile in (256, 512):
        for S in (2, 3):
            for step in (2, 3):
                kw = dict(tile=tile, max_stretches=S, step=step)
                got = ctx.overlap_run(**_kw(kw))
                _check(ctx, got, models(**kw), str(kw))
                if step == 2:
                    bp = _by_pair(got)
                    a, b = names["xy0"], names["xy1"]
                    assert sorted(g for _, g in bp[(a, b, 0)]) == [-(400 + 330), 370 + 310] and [r for r, _ in bp[(a, b, 0)]] == [0, 1]
                    a, b = names["rep0"], names["rep1"]
                    assert bp[(a, b, 0)][0] == (0, 80) and len(bp[(a, b, 0)]) == S and {g for _, g in bp[(a, b, 0)]} <= {80 - 620, 80, 80 + 620}
                    assert sorted(g for _, g in bp[(names["win0"], names["win1"], 0)]) == [0, oc.WINDOW]
                    assert len(bp[(names["wim0"], names["wim1"], 0)]) == 1
    # rep0 = 120 junk, R (300), M (320), R, 150 junk against rep1: the two cross diagonals lie in different tiles of 256
    index = oc.block_index(reads, 0, len(reads), oc.K, oc.MAX_OCC)
    tiles = otm.job_tiles_multi(index, 0, names["rep0"], reads[names["rep0"]], 256, stretches=3)
    per_tile = [sorted(c[2] for rnd in t[3] for c in rnd if c[0] == names["rep1"]) for t in tiles]
    assert len({d for x in per_tile for d in x}) == 3 and not any(len(x) == 3 for x in per_tile)                # no tile holds all three: the reduce joins them


def test_settings_equal_the_model(ctx, multi, models):
    reads, names, wd = multi
    cns = _set_db(ctx, wd, reads)
    rlen = [len(r) for r in reads]
    two = next(bb for bb in range(max(rlen), sum(rlen)) if len(oc.blocks(rlen, bb)) == 2)
    three = oc.three_blocks(rlen)
    seen = set()
    for label, kw in (("tile128_list64", dict(tile=128, list_=64, min_hits=1, max_stretches=2)), ("partners1", dict(tile=256, max_partners=1, max_stretches=2)),
                      ("two_blocks", dict(tile=256, block_bases=two, max_stretches=3)), ("three_blocks", dict(tile=512, block_bases=three, max_partners=2, max_stretches=2)),
                      ("S8", dict(tile=256, max_stretches=8, window=16, min_hits=2))):
        want = models(**kw)
        got = ctx.overlap_run(**_kw(kw))
        _check(ctx, got, want, label)
        st = want[6]
        seen |= set(got[4].reshape(-1).tolist())
        if label == "tile128_list64":
            assert st["overflow"] > 0 and st["max_tile_hits"] == 64                         # OVERFLOW in single tiles
        if label == "partners1":
            assert st["truncated"] > 0
            per_job = {}
            for r, rd in zip(got[0].tolist(), got[6].tolist()):
                per_job.setdefault((r[0], r[2]), []).append(rd)
            assert all(sorted(v) == list(range(len(v))) for v in per_job.values()) and any(len(v) == 2 for v in per_job.values())      # one candidate per round
        if label == "three_blocks":
            assert st["blocks"] == 3 and st["jobs"] == 3 * 2 * len(reads)
        if label == "S8":
            assert max(got[6].tolist()) == 2
    assert {0, oc.NONE, oc.OVERFLOW, oc.TRUNCATED} <= seen


def test_batches_and_the_environment(ctx, multi, models, monkeypatch):
    reads, names, wd = multi
    cns = _set_db(ctx, wd, reads)
    want = models(tile=256, max_stretches=2)
    row = 16 + 4 * (4 + 2 + 4 * 2 * 64)
    monkeypatch.setenv("HINGE_OVERLAP_SCRATCH_BYTES", str(row * 30))                        # about thirty tiles per batch: two or three jobs
    _check(ctx, ctx.overlap_run(tile=256, tile_stretches=2), want, "batches")
    assert ctx.overlap_stats()["batches"] > 20
    monkeypatch.setenv("HINGE_OVERLAP_SCRATCH_BYTES", str(row * 3))                         # fewer than a job's tiles: every job alone
    _check(ctx, ctx.overlap_run(tile=256, tile_stretches=2), want, "one job per batch")
    assert ctx.overlap_stats()["batches"] == 2 * len(reads)
    monkeypatch.delenv("HINGE_OVERLAP_SCRATCH_BYTES")
    monkeypatch.setenv("HINGE_OVERLAP_TILE", "256")                                         # both defaults from the environment
    monkeypatch.setenv("HINGE_OVERLAP_TILE_STRETCHES", "2")
    _check(ctx, ctx.overlap_run(tiled_multi=True), want, "env")
    _check(ctx, ctx.overlap_run(tiled=True, tile_stretches=2), want, "env tile")


def test_planted_long_reads(ctx, tmp_path):
    """Noise-free reads of 2 .. 3 kb at tile 256 (adv 128), 3 rounds.
      xy0 = X U Y, xy1 = Y V X      two stretches, in different tiles of either read: two candidates, |Y| + |V| and -(|X| + |U|)
      one0, one1                    one stretch of 1 000 bases, seven and more tiles: every tile's candidate has the same d, the first
                                    pick leaves none live - one candidate
      win0 = X U Y, win1 = X U' Y   |U'| = |U| + window: the second stretch - no tile holds both - exactly `window` away: two
      wim0, wim1                    |U'| = |U| + window - 1: one
      eight0, eight1                eight stretches of 60 bases, 100 apart in one read and 300 apart, in the opposite order, in the
                                    other: diagonals 400 apart - at 8 rounds eight candidates, one per round"""
    rng = np.random.default_rng(31)
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cat = lambda *a: np.concatenate(a).astype(np.uint8)
    reads, names = [], {}

    def add(name, r):
        names[name] = len(reads)
        reads.append(np.asarray(r, np.uint8))
    X, U, Y, V = j(800), j(900), j(700), j(600)
    add("xy0", cat(X, U, Y)); add("xy1", cat(Y, V, X))
    Z = j(1000)
    add("one0", cat(j(700), Z, j(900))); add("one1", cat(j(1100), Z, j(400)))
    for name, extra in (("win", oc.WINDOW), ("wim", oc.WINDOW - 1)):
        X, Y = j(900), j(800)
        add(name + "0", cat(X, j(500), Y)); add(name + "1", cat(X, j(500 + extra), Y))
    parts = [j(60) for _ in range(8)]
    add("eight0", cat(*[cat(q, j(40)) for q in parts])); add("eight1", cat(*[cat(q, j(240)) for q in parts[::-1]]))
    cns = _set_db(ctx, str(tmp_path), reads)
    want = otm.model_overlap_tiled_multi(reads, tile=256, max_stretches=3)
    got = ctx.overlap_run(tile=256, tile_stretches=3)
    _check(ctx, got, want, "planted")
    bp = _by_pair(got)
    a, b = names["xy0"], names["xy1"]
    assert sorted(g for _, g in bp[(a, b, 0)]) == [-(800 + 900), 700 + 600] and [r for r, _ in bp[(a, b, 0)]] == [0, 1]
    assert sorted(g for _, g in bp[(b, a, 0)]) == [-(700 + 600), 800 + 900]
    a, b = names["one0"], names["one1"]
    assert bp[(a, b, 0)] == [(0, 400)] and bp[(b, a, 0)] == [(0, -400)]
    index = oc.block_index(reads, 0, len(reads), oc.K, oc.MAX_OCC)
    tiles = otm.job_tiles_multi(index, 0, a, reads[a], 256, stretches=3)
    assert sum(1 for t in tiles if any(c[0] == b for c in t[3][0])) >= 5                     # the stretch spans five or more tiles
    assert sorted(g for _, g in bp[(names["win0"], names["win1"], 0)]) == [0, oc.WINDOW]
    assert bp[(names["wim0"], names["wim1"], 0)] == [(0, 0)]                                 # equal counts: the lowest tile's, X's
    tiles = otm.job_tiles_multi(index, 0, names["wim0"], reads[names["wim0"]], 256, stretches=3)
    assert not any(len({c[2] for rnd in t[3] for c in rnd if c[0] == names["wim1"]}) > 1 for t in tiles)      # no tile holds both stretches
    got = ctx.overlap_run(tile=256, tile_stretches=8)
    _check(ctx, got, otm.model_overlap_tiled_multi(reads, tile=256, max_stretches=8), "planted S8")
    bp = _by_pair(got)
    a, b = names["eight0"], names["eight1"]
    assert [r for r, _ in bp[(a, b, 0)]] == list(range(8))                                  # eight rounds, one candidate each
    assert sorted(g for _, g in bp[(a, b, 0)]) == [2100 - 400 * i for i in range(7, -1, -1)]


def test_one_round_equals_the_tiled_call(ctx, multi):
    """At one round every array is hinge_overlap_run_tiled's, from other kernels."""
    reads, names, wd = multi
    cns = _set_db(ctx, wd, reads)
    for kw in (dict(tile=256), dict(tile=8192), dict(tile=256, max_partners=1), dict(tile=128, list_=64, min_hits=1)):
        ctx.profile_enable(64)                                                              # (the report counts from here)
        tiled = ctx.overlap_run(**kw)
        st_t, ts_t = ctx.overlap_stats(), ctx.overlap_tile_stats()
        rep = ctx.profile_report()
        assert rep["k_overlap_vote_tile"][1] == st_t["batches"] and rep.get("k_overlap_vote_tile_multi", (0.0, 0))[1] == 0
        ctx.profile_enable(64)
        one = ctx.overlap_run(tile_stretches=1, **kw)
        rep = ctx.profile_report()
        assert rep["k_overlap_vote_tile_multi"][1] == rep["k_overlap_tile_reduce_multi"][1] == st_t["batches"]      # the profiler ids of both kernels
        assert rep.get("k_overlap_vote_tile", (0.0, 0))[1] == 0 and rep.get("k_overlap_tile_reduce", (0.0, 0))[1] == 0
        for x, y in zip(tiled, one[:6]):
            assert np.array_equal(x, y), kw
        assert not one[6].any()
        st_o, ts_o = ctx.overlap_stats(), ctx.overlap_tile_stats()
        st_t.pop("index_us"); st_o.pop("index_us")
        assert st_o == st_t and ts_o == ts_t, kw
    ctx.profile_enable(0)


def test_one_tile_reads_equal_the_whole_read_rounds(ctx, multi):
    """Every read of the set has one tile of 8 192 bases: every array and the rounds are hinge_overlap_run_multi's."""
    reads, names, wd = multi
    cns = _set_db(ctx, wd, reads)
    for kw in (dict(), dict(max_partners=1), dict(list_=64, min_hits=1, step=128)):
        whole = ctx.overlap_run(max_stretches=3, **kw)
        tiled = ctx.overlap_run(tile=8192, tile_stretches=3, **kw)
        for x, y in zip(whole, tiled):
            assert np.array_equal(x, y), kw
        assert ctx.overlap_tile_stats()["tiles"] == ctx.overlap_stats()["jobs"] == 2 * len(reads) and ctx.overlap_tile_stats()["multi_tile_jobs"] == 0
    assert max(tiled[6].tolist()) >= 1


def test_bad_arguments_are_refused(ctx, multi):
    from hinge_amd import capi
    reads, names, wd = multi
    cns = _set_db(ctx, wd, reads)
    for kw in (dict(tile=256, tile_stretches=-1), dict(tile=256, tile_stretches=9), dict(tile=100, tile_stretches=2), dict(tile=32, tile_stretches=2),
               dict(tile=16384, tile_stretches=2), dict(tile=-64, tile_stretches=2), dict(tile=8192, list_=64, tile_stretches=2), dict(tile=512, list_=64, step=7, tile_stretches=2)):
        with pytest.raises(capi.HingeError) as e:
            ctx.overlap_run(**kw)
        assert e.value.code == capi.HINGE_E_ARG, kw
    with pytest.raises(ValueError):
        ctx.overlap_run(tile_stretches=2)
    with pytest.raises(ValueError):
        ctx.overlap_run(tile_stretches=2, max_stretches=2)
    with pytest.raises(ValueError):
        ctx.overlap_run(tile=256, tile_stretches=2, max_stretches=2)
    with pytest.raises(ValueError):
        ctx.overlap_run(tile=256, tile_stretches=2, multi=True)
    ctx.overlap_run(tile=512, list_=64, step=8, tile_stretches=8)                           # T = list * step, the most rounds: the largest allowed
