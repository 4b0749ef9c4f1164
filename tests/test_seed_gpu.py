"""`hinge seed` on the GPU: Context.seed_run value for value against the numpy model (tests/seed_common.py) - placements, count,
diagonal, placements per read, status per strand - on cns_tiny and on the edge list the host test shares (tests/test_seed_host.py
runs the items marked host-only there)."""
import ctypes as C
import os

import numpy as np
import pytest

import seed_common as sm
import trace_common as tc
from hinge_amd import formats
from hinge_amd import synth_consensus as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


@pytest.fixture(scope="module")
def tiny():
    d = sc.generate(sc.CONFIGS["cns_tiny"])
    index = sm.Index(d.contigs)
    want = {n: sm.model_seed(d.contigs, d.reads, max_placements=n, index=index) for n in (1, 2)}
    return d, index, want


def _set_dbs(ctx, wd, contigs, reads):
    from hinge_amd import capi
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "draft"), np.asarray([len(c) for c in contigs], np.int32), bases=contigs)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return capi.Consensus(ctx, os.path.join(wd, "draft"), os.path.join(wd, "reads"))


def _check(got, want, label=""):
    pl, count, diag, n_placed, status = got
    assert n_placed.tolist() == want[3], (label, n_placed.tolist(), want[3])
    assert [tuple(s) for s in status.tolist()] == want[4], label
    assert [tuple(r) for r in pl.tolist()] == [tuple(int(v) for v in p) for p in want[0]], label
    assert count.tolist() == want[1] and diag.tolist() == want[2], label


def test_cns_tiny_equals_the_model(ctx, tiny, tmp_path):
    d, index, want = tiny
    _set_dbs(ctx, str(tmp_path), d.contigs, d.reads)
    got = ctx.seed_run()
    _check(got, want[1], "n1")
    st = ctx.seed_stats()
    assert st["jobs"] == 2 * len(d.reads) and st["batches"] == 1 and st["entries"] == len(index.codes) and st["dropped_codes"] == index.dropped_codes
    assert st["overflow"] == 0 and st["unplaced"] == sum(n == 0 for n in want[1][3])
    # the recall rule on what the GPU answered: no record of >= 400 bases is missed
    checked, missed, left_out = sm.recall(d, ([tuple(r) for r in got[0].tolist()], got[1].tolist(), got[2].tolist(), got[3].tolist(), None), index)
    assert checked >= 40 and missed == [] and all(ln < 400 for ln in left_out)
    _check(ctx.seed_run(max_placements=2), want[2], "n2")


def test_edge_list_equals_the_model(ctx, tmp_path):
    seen = set()
    for label, contigs, reads, kw, host_only in sm.edge_calls():
        if host_only:
            continue
        _set_dbs(ctx, os.path.join(str(tmp_path), label), contigs, reads)
        want = sm.model_seed(contigs, reads, **kw)
        got = ctx.seed_run(**kw)
        _check(got, want, label)
        seen |= set(got[4].reshape(-1).tolist())
        if label == "over65":
            assert ctx.seed_stats()["overflow"] == 2
        if label == "max_occ":
            assert ctx.seed_stats()["dropped_codes"] >= 1
    assert seen == {sm.OK, sm.NONE, sm.OVERFLOW}


def test_read_id_subset_and_two_batches(ctx, tiny, tmp_path, monkeypatch):
    d, index, want = tiny
    _set_dbs(ctx, str(tmp_path), d.contigs, d.reads)
    ids = [5, 0, 17, 5, len(d.reads) - 1]
    _check(ctx.seed_run(read_ids=ids), sm.model_seed(d.contigs, d.reads, read_ids=ids, index=index), "subset")
    assert ctx.seed_stats()["jobs"] == 10
    pl, count, diag, n_placed, status = ctx.seed_run(read_ids=np.zeros(0, np.int32))
    assert len(pl) == 0 and len(n_placed) == 0 and len(status) == 0
    monkeypatch.setenv("HINGE_SEED_SCRATCH_BYTES", str(48 * 20))                   # 16 bytes of job + 32 of results at N = 1: ten reads per batch
    _check(ctx.seed_run(), want[1], "batches")
    assert ctx.seed_stats()["batches"] == (len(d.reads) + 9) // 10 >= 2 and ctx.seed_stats()["jobs"] == 2 * len(d.reads)
    monkeypatch.delenv("HINGE_SEED_SCRATCH_BYTES")
    monkeypatch.setenv("HINGE_SEED_MAX_PLACEMENTS", "2")                           # a default from the environment
    _check(ctx.seed_run(), want[2], "env")


def test_seeded_placements_go_into_trace_local_unchanged(ctx, tiny, tmp_path):
    d, index, want = tiny
    _set_dbs(ctx, str(tmp_path), d.contigs, d.reads)
    pl = ctx.seed_run()[0]
    alns, trace, diffs, status, score = ctx.trace_local(pl, d.spec.tspace)
    assert len(alns) == len(pl) and int((status[:, 0] == tc.OK).sum()) >= len(pl) - 2


def test_refusals(ctx, tiny, tmp_path):
    from hinge_amd import capi
    d, index, want = tiny
    _set_dbs(ctx, str(tmp_path), d.contigs, d.reads)
    for kw in (dict(k=7), dict(k=17), dict(window=100), dict(window=8), dict(list_=100), dict(list_=32), dict(list_=8192), dict(max_placements=9), dict(max_occ=257), dict(step=-1), dict(min_hits=-1)):
        with pytest.raises(capi.HingeError) as e:
            ctx.seed_run(**kw)
        assert e.value.code == capi.HINGE_E_ARG, kw
    with pytest.raises(capi.HingeError) as e:
        ctx.seed_run(read_ids=[0, len(d.reads)])
    assert e.value.code == capi.HINGE_E_RANGE
    # output arrays too small for max_placements records per read: refused before any launch
    n = len(d.reads)
    out, cnt, dg, npl, st, m = np.zeros(n, capi.CNS_ALN_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2 * n, np.int32), C.c_int64(-1)
    prm = np.asarray([0, 0, 0, 0, 0, 2, 0], np.int32)
    args = (out.ctypes.data, cnt.ctypes.data, dg.ctypes.data, npl.ctypes.data, st.ctypes.data, C.byref(m))
    assert ctx.lib.hinge_seed_run(ctx.h, prm.ctypes.data, n, None, n, *args) == capi.HINGE_E_CAPACITY
    assert ctx.lib.hinge_seed_run(ctx.h, None, n - 1, None, n, *args) == capi.HINGE_E_ARG      # without ids: all reads
    assert ctx.lib.hinge_seed_run(ctx.h, None, -1, None, n, *args) == capi.HINGE_OK and m.value == sum(want[1][3])          # -1 = all reads
    assert ctx.lib.hinge_seed_run(ctx.h, None, n, None, n, *args) == capi.HINGE_OK and m.value == sum(want[1][3])   # NULL params = the defaults
