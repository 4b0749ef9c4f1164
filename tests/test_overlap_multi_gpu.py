"""hinge_overlap_run_multi on the GPU: Context.overlap_run(max_stretches=S) value for value against the numpy model
(tests/overlap_multi_common.py) - per (read, strand) the status and the hits kept, per candidate (b, cnt, d, p), its round, its
record and its diagonal - on the edge set of test_overlap_gpu.py plus the planted reads whose pairs overlap in several stretches
(overlap_multi_common.planted_reads); at one stretch every array against hinge_overlap_run's on the same reads."""
import os

import numpy as np
import pytest

import overlap_common as oc
import overlap_multi_common as om
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
def multi(ctx, tmp_path_factory):
    reads, names = om.multi_reads()
    cns = _set_db(ctx, str(tmp_path_factory.mktemp("overlap_multi")), reads)
    return reads, names, cns


@pytest.fixture(scope="module")
def models(multi):
    """The model's answers, computed once per setting and shared."""
    reads = multi[0]
    cache = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = om.model_overlap_multi(reads, **kw)
        return cache[key]
    return get


def _check(got, want, label=""):
    pl, count, diag, rep, status, hits, rnd = got
    rows, cnt, dg, wrep, wstatus, whits, st, wrnd = want
    assert status.tolist() == wstatus, label
    assert hits.tolist() == whits, label
    assert [tuple(r) for r in pl.tolist()] == [tuple(int(v) for v in r) for r in rows], label
    assert count.tolist() == cnt and diag.tolist() == dg, label
    assert [tuple(r) for r in rep.tolist()] == wrep, label
    assert rnd.tolist() == wrnd, label


def _blocks(reads):
    rlen = [len(r) for r in reads]
    two = three = None
    for bb in range(max(rlen), sum(rlen)):
        n = len(oc.blocks(rlen, bb))
        if three is None and n == 3:
            three = bb
        if two is None and n == 2:
            two = bb
    assert two and three
    return two, three


def test_planted_stretches_equal_the_model(ctx, multi, models):
    reads, names, cns = multi
    rlen = [len(r) for r in reads]
    want = models(max_stretches=3)
    got = ctx.overlap_run(max_stretches=3)
    _check(got, want, "S3")
    st, ws = ctx.overlap_stats(), want[6]
    assert all(st[x] == ws[x] for x in ws), (st, ws)
    by_pair = {}
    for r, g, rd in zip(got[0].tolist(), got[2].tolist(), got[6].tolist()):
        by_pair.setdefault(tuple(r[:3]), []).append((rd, g))
    # X U Y against Y V X: two stretches, diagonals |Y| + |V| and -(|X| + |U|), thousands apart; in either direction
    a, b = names["xy0"], names["xy1"]
    assert sorted(g for _, g in by_pair[(a, b, 0)]) == [-(400 + 330), 370 + 310] and [r for r, _ in by_pair[(a, b, 0)]] == [0, 1]
    assert sorted(g for _, g in by_pair[(b, a, 0)]) == [-(370 + 310), 400 + 330]
    # the same with the second read stored reverse-complemented: on the complement strand only
    a, b = names["rc0"], names["rc1"]
    assert len(by_pair[(a, b, 1)]) == 2 and (a, b, 0) not in by_pair
    assert sorted(oc.alen_blen_mirror(rlen[a], rlen[b], 1, g) for _, g in by_pair[(a, b, 1)]) == sorted(g for _, g in by_pair[(b, a, 1)])
    # L R M R N seen by two reads: the main diagonal and the two cross ones, |R| + |M| to either side
    a, b = names["rep0"], names["rep1"]
    assert sorted(g for _, g in by_pair[(a, b, 0)]) == [80 - 620, 80, 80 + 620] and by_pair[(a, b, 0)][0] == (0, 80)
    # diagonals exactly `window` apart: two candidates; window - 1 apart: the second stretch's hits are dead, one candidate
    assert sorted(g for _, g in by_pair[(names["win0"], names["win1"], 0)]) == [0, oc.WINDOW]
    assert [g for _, g in by_pair[(names["wim0"], names["wim1"], 0)]] in ([0], [oc.WINDOW - 1])
    assert max(got[6].tolist()) == 2


def test_settings_equal_the_model(ctx, multi, models):
    reads, names, cns = multi
    two, three = _blocks(reads)
    seen = set()
    for label, kw in (("list64", dict(list_=64, max_stretches=2)), ("partners1", dict(max_partners=1, max_stretches=2)), ("two_blocks", dict(block_bases=two, max_stretches=3)),
                      ("three_blocks", dict(block_bases=three, max_partners=2, max_stretches=2)), ("step3_window16", dict(step=3, window=16, min_hits=2, max_stretches=4)),
                      ("S8", dict(max_stretches=8))):
        want = models(**kw)
        got = ctx.overlap_run(**kw)
        _check(got, want, label)
        st, ws = ctx.overlap_stats(), want[6]
        assert all(st[x] == ws[x] for x in ws), (label, st, ws)
        seen |= set(got[4].reshape(-1).tolist())
        if label == "list64":
            assert st["overflow"] > 0
        if label == "partners1":
            # TRUNCATED per round, the first b kept in each: per (read, strand) one candidate per round, round 0's the smallest b of all
            assert st["truncated"] > 0
            full = models(max_stretches=2)
            first_b = {}
            for r, rd in zip(full[0], full[7]):
                first_b.setdefault((r[0], r[2], rd), r[1])
            assert {(r[0], r[2], rd): r[1] for r, rd in zip(got[0].tolist(), got[6].tolist())} == first_b
        if label in ("two_blocks", "three_blocks"):
            assert st["blocks"] == (2 if label == "two_blocks" else 3) and st["jobs"] == st["blocks"] * 2 * len(reads)
        if label == "S8":
            # eight rounds where no b has more than three picks: the round loop ends early, the rest of the head reads 0
            assert max(got[6].tolist()) == 2
    assert {0, oc.NONE, oc.OVERFLOW, oc.TRUNCATED} <= seen


def test_batches_and_environment(ctx, multi, models, monkeypatch):
    reads, names, cns = multi
    want = models(max_stretches=2)
    W = 4 + 2 + 4 * 2 * 64                                                                              # a job's output at two rounds, 64 partners
    monkeypatch.setenv("HINGE_OVERLAP_SCRATCH_BYTES", str((16 + 4 * W) * 20))                           # twenty jobs per batch
    _check(ctx.overlap_run(max_stretches=2), want, "batches")
    assert ctx.overlap_stats()["batches"] == (2 * len(reads) + 19) // 20
    monkeypatch.delenv("HINGE_OVERLAP_SCRATCH_BYTES")
    monkeypatch.setenv("HINGE_OVERLAP_MAX_STRETCHES", "2")                                              # S from the environment
    _check(ctx.overlap_run(multi=True), want, "env")
    monkeypatch.delenv("HINGE_OVERLAP_MAX_STRETCHES")
    _check(ctx.overlap_run(multi=True), models(max_stretches=1), "env default")


def test_one_stretch_equals_overlap_run(ctx, multi):
    reads, names, cns = multi
    two, three = _blocks(reads)
    for kw in (dict(), dict(list_=64), dict(max_partners=1), dict(block_bases=three, max_partners=2), dict(step=3, window=16, min_hits=2)):
        one = ctx.overlap_run(max_stretches=1, **kw)
        st1 = ctx.overlap_stats()
        old = ctx.overlap_run(**kw)
        st0 = ctx.overlap_stats()
        assert len(one) == 7 and len(old) == 6 and len(old[0]) > 0
        for x, y in zip(one[:6], old):
            assert x.dtype == y.dtype and np.array_equal(x, y), kw
        assert not one[6].any()
        assert {k: v for k, v in st1.items() if k != "index_us"} == {k: v for k, v in st0.items() if k != "index_us"}


def test_candidates_go_into_trace_local(ctx, multi):
    reads, names, cns = multi
    pl = ctx.overlap_run(max_stretches=3)[0]
    alns, trace, diffs, status, score = ctx.trace_local(pl, 100)
    assert len(alns) == len(pl) and int((status[:, 0] == 0).sum()) == len(pl) and int(diffs.sum()) == 0


def test_refusals(ctx, multi, tmp_path):
    from hinge_amd import capi
    reads, names, cns = multi
    for s in (-1, 9):
        with pytest.raises(capi.HingeError) as e:
            ctx.overlap_run(max_stretches=s)
        assert e.value.code == capi.HINGE_E_ARG, s
    with pytest.raises(capi.HingeError) as e:
        ctx.overlap_run(max_stretches=2, list_=100)
    assert e.value.code == capi.HINGE_E_ARG
    # a read beyond the packing limit: refused before any launch
    rng = np.random.default_rng(2)
    big = _set_db(ctx, os.path.join(str(tmp_path), "big"), [reads[0], rng.integers(0, 4, size=oc.READ_MAX + 1, dtype=np.uint8), reads[1]])
    ctx.profile_enable(16)
    with pytest.raises(capi.HingeError) as e:
        ctx.overlap_run(max_stretches=2)
    assert e.value.code == capi.HINGE_E_CAPACITY
    assert ctx.profile_report().get("k_overlap_vote_multi", (0.0, 0))[1] == 0
    # and the new kernel is what a run launches, under its own profiler name
    again = _set_db(ctx, os.path.join(str(tmp_path), "again"), reads)
    ctx.profile_enable(256)                                              # (room for the index build's launches in front of it)
    ctx.overlap_run(max_stretches=2)
    rep = ctx.profile_report()
    assert rep.get("k_overlap_vote_multi", (0.0, 0))[1] == 1 and rep.get("k_overlap_vote", (0.0, 0))[1] == 0
