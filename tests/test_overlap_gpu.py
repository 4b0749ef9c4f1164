"""`hinge overlap` on the GPU: Context.overlap_run value for value against the numpy model (tests/overlap_common.py) - per (read,
strand) the status and the hits kept, per candidate (b, cnt, d, p), its record and its diagonal - on the edge set the host test
shares: about 40 reads of 300 .. 1 500 bases cut from a 6 kb genome and the special ones (overlap_common.edge_reads)."""
import os

import numpy as np
import pytest

import overlap_common as oc
import seed_common as sm
from hinge_amd import formats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


@pytest.fixture(scope="module")
def edge(ctx, tmp_path_factory):
    reads, names = oc.edge_reads()
    cns = _set_db(ctx, str(tmp_path_factory.mktemp("overlap_edge")), reads)
    return reads, names, cns


def _set_db(ctx, wd, reads):
    from hinge_amd import capi
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))


def _check(got, want, label=""):
    pl, count, diag, rep, status, hits = got
    rows, cnt, dg, wrep, wstatus, whits, st = want
    assert status.tolist() == wstatus, label
    assert hits.tolist() == whits, label
    assert [tuple(r) for r in pl.tolist()] == [tuple(int(v) for v in r) for r in rows], label
    assert count.tolist() == cnt and diag.tolist() == dg, label
    assert [tuple(r) for r in rep.tolist()] == wrep, label


def test_edge_set_equals_the_model(ctx, edge):
    reads, names, cns = edge
    seen = set()
    for label, kw in oc.edge_calls():
        want = oc.model_overlap(reads, **kw)
        got = ctx.overlap_run(**kw)
        _check(got, want, label)
        st, ws = ctx.overlap_stats(), want[6]
        assert all(st[x] == ws[x] for x in ws), (label, st, ws)
        assert st["batches"] == st["blocks"]
        seen |= set(got[4].reshape(-1).tolist())
        by_pair = {tuple(r[:3]): (c, tuple(q)) for r, c, q in zip(got[0].tolist(), got[1].tolist(), got[3].tolist())}
        status, hits = got[4], got[5]
        assert status[names["short"]].tolist() == [oc.NONE, oc.NONE] and hits[names["short"]].tolist() == [0, 0]          # shorter than k
        assert status[names["no_hit"]].tolist() == [oc.NONE, oc.NONE] and hits[names["no_hit"]].tolist() == [0, 0]
        if label == "min_hits1":
            # a hit count of 1, and one of exactly 64 - the smallest network, full; the group ends on the list's last element
            assert hits[names["one0"]].tolist() == [1, 0] and by_pair[(names["one0"], names["one1"], 0)][0] == 1
            assert hits[names["pow0"]].tolist() == [64, 0] and by_pair[(names["pow0"], names["pow1"], 0)][0] == 64
            # the pair that overlaps on the complement strand only
            assert (names["comp0"], names["comp1"], 1) in by_pair and (names["comp0"], names["comp1"], 0) not in by_pair
        if label == "list64_min_hits1":
            assert st["overflow"] > 0 and oc.OVERFLOW in seen
            assert hits[names["pow0"]].tolist() == [64, 0] and status[names["pow0"]][0] == 0 and by_pair[(names["pow0"], names["pow1"], 0)][0] == 64
            # self hits took no slot: with them in the list the tandem read's first 64 hits would be others
            t = names["tandem"]
            index = sm.Index(reads, oc.K, oc.MAX_OCC)
            mine = oc.job_hits(index, 0, t, reads[t], oc.STEP, 64)
            with_self = oc.job_hits(index, 0, t, reads[t], oc.STEP, 64, keep_self=True)
            assert t in with_self[0].tolist() and t not in mine[0].tolist() and mine[2].max() > with_self[2].max()
            assert hits[t][0] == 64 and status[t][0] & oc.OVERFLOW
        if label == "partners1":
            assert st["truncated"] > 0
            full = oc.model_overlap(reads)
            first_b = {}
            for r in full[0]:
                first_b.setdefault((r[0], r[2]), r[1])
            assert {(r[0], r[2]): r[1] for r in got[0].tolist()} == first_b                                               # the first b is kept
        if label == "defaults":
            # identical reads find each other over their whole length; the tandem read finds its partners and never itself
            for x, y in ((0, names["twin0"]), (names["twin0"], names["twin1"])):
                assert by_pair[(x, y, 0)][0] == by_pair[(y, x, 0)][0] and got[2][[tuple(r[:3]) for r in got[0].tolist()].index((x, y, 0))] == 0
            assert all(r[0] != r[1] for r in got[0].tolist())
            assert len([r for r in got[0].tolist() if r[0] == names["tandem"]]) >= 3
        if label == "three_blocks":
            assert st["blocks"] == 3 and st["jobs"] == 3 * 2 * len(reads)
    assert {0, oc.NONE, oc.OVERFLOW, oc.TRUNCATED} <= seen


def test_batches_and_environment_defaults(ctx, edge, monkeypatch):
    reads, names, cns = edge
    want = oc.model_overlap(reads)
    monkeypatch.setenv("HINGE_OVERLAP_SCRATCH_BYTES", str((16 + 4 * (4 + 4 * 64)) * 20))              # twenty jobs per batch
    _check(ctx.overlap_run(), want, "batches")
    assert ctx.overlap_stats()["batches"] == (2 * len(reads) + 19) // 20
    monkeypatch.delenv("HINGE_OVERLAP_SCRATCH_BYTES")
    monkeypatch.setenv("HINGE_OVERLAP_MAX_PARTNERS", "1")                                               # a default from the environment
    _check(ctx.overlap_run(), oc.model_overlap(reads, max_partners=1), "env")


def test_candidates_go_into_trace_local_unchanged(ctx, edge):
    reads, names, cns = edge
    pl = ctx.overlap_run()[0]
    alns, trace, diffs, status, score = ctx.trace_local(pl, 100)
    assert len(alns) == len(pl) and int((status[:, 0] == 0).sum()) == len(pl)                           # noise-free reads: every candidate aligns
    assert int(diffs.sum()) == 0


def test_refusals(ctx, edge, tmp_path):
    from hinge_amd import capi
    reads, names, cns = edge
    for kw in (dict(k=7), dict(k=17), dict(window=100), dict(window=8), dict(list_=100), dict(list_=32), dict(list_=16384), dict(max_partners=4097), dict(max_partners=-1),
               dict(max_occ=257), dict(step=-1), dict(min_hits=-1), dict(block_bases=-1), dict(block_bases=1 << 31)):
        with pytest.raises(capi.HingeError) as e:
            ctx.overlap_run(**kw)
        assert e.value.code == capi.HINGE_E_ARG, kw
    # the two DBs differ
    formats.write_db(os.path.join(str(tmp_path), "other"), np.asarray([len(r) for r in reads[:5]], np.int32), bases=reads[:5])
    formats.write_db(os.path.join(str(tmp_path), "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    both = capi.Consensus(ctx, os.path.join(str(tmp_path), "other"), os.path.join(str(tmp_path), "reads"))
    with pytest.raises(capi.HingeError) as e:
        ctx.overlap_run()
    assert e.value.code == capi.HINGE_E_ARG
    # a read beyond the packing limit: refused before any launch
    rng = np.random.default_rng(2)
    long_reads = [reads[0], rng.integers(0, 4, size=oc.READ_MAX + 1, dtype=np.uint8), reads[1]]
    big = _set_db(ctx, os.path.join(str(tmp_path), "big"), long_reads)
    ctx.profile_enable(16)
    with pytest.raises(capi.HingeError) as e:
        ctx.overlap_run()
    assert e.value.code == capi.HINGE_E_CAPACITY
    assert ctx.profile_report().get("k_overlap_vote", (0.0, 0))[1] == 0
    ok = _set_db(ctx, os.path.join(str(tmp_path), "fits"), [reads[0], long_reads[1][:oc.READ_MAX], reads[1]])      # the longest read that fits
    got = ctx.overlap_run()
    _check(got, oc.model_overlap([reads[0], long_reads[1][:oc.READ_MAX], reads[1]]), "fits")
