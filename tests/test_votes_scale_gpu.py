"""The vote kernels on indexes of a real block's and a real draft's size: k_overlap_vote, k_overlap_vote_multi and k_seed_vote value
for value against the numpy models (overlap_common, overlap_multi_common, seed_common) where their fixed-trip searches run at
depth - search_top = 2^22 (4.3 M entries), read_top = 1024 (1030 reads in one block), off[] up to 4.3 M - and, small, at k = 8 and
k = 16 (codes with bit 31 set under the search's unsigned compares), which tests/test_overlap_gpu.py and tests/test_seed_gpu.py
leave to the host builds.  The overlap set is index_common.block_set(); of its 2 060 jobs the model answers the 62 of PICKS (the
reads around every power of two the offset search passes, the first, the last, and twenty in between), the library all of them."""
import os

import numpy as np
import pytest

import index_common as ic
import overlap_common as oc
import overlap_multi_common as om
import seed_common as sm
from hinge_amd import synth_consensus as sc
from test_overlap_gpu import _check as _check_overlap, _set_db
from test_seed_gpu import _check as _check_seed, _set_dbs

pytestmark = pytest.mark.gpu

PICKS = [0, 1, 2, 255, 256, 511, 512, 513, 1023, 1024, 1029] + list(range(700, 720))


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    """(reads, the DB's directory, the dict that keeps the model's indexes from test to test)."""
    reads = ic.block_set()
    wd = str(tmp_path_factory.mktemp("votes_block"))
    return reads, wd, {}


def _use(ctx, block):
    reads, wd, indexes = block
    if not os.path.exists(os.path.join(wd, "written")):
        _set_db(ctx, wd, reads)
        open(os.path.join(wd, "written"), "w").close()
    else:
        from hinge_amd import capi
        capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))
    return reads, indexes


def _check_picks(got, want, label):
    """The library's answer for the reads of PICKS against model_overlap_jobs' / model_overlap_multi_jobs': status and hits kept per
    strand, and every row, count, diag, (d, p) and round of those a (both are sorted by (a, b, comp, round))."""
    pl, count, diag, rep, status, hits = got[:6]
    rows, cnt, dg, wrep, wstatus, whits, st = want[:7]
    assert {a: status[a].tolist() for a in wstatus} == wstatus, label
    assert {a: hits[a].tolist() for a in whits} == whits, label
    sel = np.isin(pl[:, 0], sorted(wstatus))
    assert [tuple(r) for r in pl[sel].tolist()] == [tuple(int(v) for v in r) for r in rows], label
    assert count[sel].tolist() == cnt and diag[sel].tolist() == dg, label
    assert [tuple(r) for r in rep[sel].tolist()] == wrep, label
    if len(want) == 8:
        assert got[6][sel].tolist() == want[7], label


def _conditions(want, reads, label):
    """What makes the picks worth comparing, on the model's answer alone."""
    rows, cnt, dg, wrep, wstatus, whits, st = want[:7]
    seen = {s for pair in wstatus.values() for s in pair}
    assert len(rows) >= 100, (label, len(rows))
    assert 0 in seen and oc.NONE in seen and any(s != oc.NONE and s & oc.OVERFLOW for s in seen), (label, seen)
    assert max(h for pair in whits.values() for h in pair) >= oc.LIST, label          # some job fills the list (in every block it meets: at least once)
    assert any(r[1] >= 1024 for r in rows) and any(r[1] < 512 for r in rows), label


def test_overlap_one_block_of_1030_reads(ctx, block):
    reads, indexes = _use(ctx, block)
    want = oc.model_overlap_jobs(reads, PICKS, indexes=indexes)
    _conditions(want, reads, "one_block")
    assert max(h for pair in want[5].values() for h in pair) == oc.LIST
    got = ctx.overlap_run()
    st, ws = ctx.overlap_stats(), want[6]
    assert st["blocks"] == ws["blocks"] == 1 and st["entries"] == ws["entries"] >= 1 << 22 and st["dropped_codes"] == ws["dropped_codes"] and st["jobs"] == 2 * len(reads)
    assert ctx.index_last_stats()["device_builds"] == 1
    _check_picks(got, want, "one_block")
    assert all(r[0] != r[1] for r in got[0].tolist())


def test_overlap_three_blocks(ctx, block):
    """first > 0 and block-relative gpos at depth: three blocks of about 343 reads, every job against each."""
    reads, indexes = _use(ctx, block)
    rlen = [len(r) for r in reads]
    bb = oc.three_blocks(rlen)
    want = oc.model_overlap_jobs(reads, PICKS, block_bases=bb, indexes=indexes)
    _conditions(want, reads, "three_blocks")
    got = ctx.overlap_run(block_bases=bb)
    st, ws = ctx.overlap_stats(), want[6]
    assert st["blocks"] == ws["blocks"] == 3 and st["entries"] == ws["entries"] and st["dropped_codes"] == ws["dropped_codes"] and st["jobs"] == 3 * 2 * len(reads)
    _check_picks(got, want, "three_blocks")


def test_overlap_two_stretches_one_block(ctx, block):
    reads, indexes = _use(ctx, block)
    want = om.model_overlap_multi_jobs(reads, PICKS, max_stretches=2, indexes=indexes)
    _conditions(want, reads, "two_stretches")
    got = ctx.overlap_run(max_stretches=2)
    st, ws = ctx.overlap_stats(), want[6]
    assert st["blocks"] == 1 and st["entries"] == ws["entries"] and st["dropped_codes"] == ws["dropped_codes"]
    _check_picks(got, want, "two_stretches")
    assert set(want[7]) <= {0, 1} and 0 in want[7]


def draft_case(seed=11):
    """(contigs, reads, truth [(contig or None, comp)]): three contigs of 1 000 000, 3 200 000 and 100 000 bases cut from one random
    sequence; reads of 2 .. 6 kb from the first and the last 3 kb of every contig, from the middle of the long one, one hanging over
    each end of the long one (500 random bases outside), both strands, every second one with 5 % substitutions; two unrelated ones."""
    rng = np.random.default_rng(seed)
    S = rng.integers(0, 4, size=4_300_000, dtype=np.uint8)
    contigs = [S[:1_000_000].copy(), S[1_000_000:4_200_000].copy(), S[4_200_000:].copy()]
    j = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cuts = []
    for c, ctg in enumerate(contigs):
        L = len(ctg)
        for ln in (2000, 3000):
            cuts.append((c, ctg[:ln].copy()))
            cuts.append((c, ctg[L - ln:].copy()))
    for _ in range(20):
        ln = int(rng.integers(2000, 6001))
        a = int(rng.integers(1_000_000, 2_200_000))
        cuts.append((1, contigs[1][a:a + ln].copy()))
    cuts.append((1, np.concatenate([j(500), contigs[1][:2500]]).astype(np.uint8)))
    cuts.append((1, np.concatenate([contigs[1][-2500:], j(500)]).astype(np.uint8)))
    reads, truth = [], []
    for x, (c, r) in enumerate(cuts):
        if (x + x // 4) % 2:                                             # (x % 2 is the end of the contig: either kind at both ends)
            at = rng.random(len(r)) < 0.05
            r = np.where(at, (r + rng.integers(1, 4, size=len(r))) % 4, r).astype(np.uint8)
        comp = (x // 2) % 2
        reads.append(sm.revcomp(r) if comp else r)
        truth.append((c, comp))
    for _ in range(2):
        reads.append(j(4000))
        truth.append((None, 0))
    return contigs, reads, truth


def test_seed_on_a_draft_size_index(ctx, tmp_path):
    C = ic.scan_chunk_from_source()
    contigs, reads, truth = draft_case()
    assert [len(c) for c in contigs] == [1_000_000, 3_200_000, 100_000] and 36 <= len(reads) <= 44
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    index = sm.Index(contigs)
    assert len(index.codes) > C * C + 1
    for n in (1, 2):
        want = sm.model_seed(contigs, reads, max_placements=n, index=index)
        got = ctx.seed_run() if n == 1 else ctx.seed_run(max_placements=2)
        st = ctx.seed_stats()
        assert st["entries"] == len(index.codes) > C * C + 1 and st["dropped_codes"] == index.dropped_codes and st["jobs"] == 2 * len(reads)
        _check_seed(got, want, "draft_n%d" % n)
        if n == 1:
            # the model's answer is worth comparing: every planted read on its contig and strand, the unrelated ones nowhere
            rows = {int(r[1]): r for r in want[0]}
            for b, (c, comp) in enumerate(truth):
                if c is None:
                    assert b not in rows and want[4][b] == (sm.NONE, sm.NONE)
                else:
                    assert b in rows and rows[b][0] == c and rows[b][2] == comp, (b, c, comp, rows.get(b))
            gp = [int(index.off[r[0]]) + int(r[3]) for r in want[0]]
            assert max(gp) > 1 << 22 and min(gp) < 1 << 20
            assert {r[2] for r in want[0]} == {0, 1}
    assert ctx.index_last_stats()["device_builds"] == 1


@pytest.mark.parametrize("k,max_occ", ((16, 0), (8, 64)))
def test_overlap_k8_and_k16(ctx, tmp_path, k, max_occ):
    reads, names = oc.edge_reads()
    _set_db(ctx, str(tmp_path), reads)
    kw = dict(k=k, max_occ=max_occ) if max_occ else dict(k=k)
    want = oc.model_overlap(reads, **kw)
    assert len(want[0]) >= 1
    if k == 16:
        assert (sm.Index(reads, 16, oc.MAX_OCC).codes >= 2 ** 31).any()
    got = ctx.overlap_run(**kw)
    _check_overlap(got, want, "k%d" % k)
    st, ws = ctx.overlap_stats(), want[6]
    assert all(st[x] == ws[x] for x in ws), (k, st, ws)
    assert ctx.index_last_stats()["device_builds"] == 1


@pytest.mark.parametrize("k,max_occ", ((16, 0), (8, 64)))
def test_seed_k8_and_k16(ctx, tmp_path, k, max_occ):
    d = sc.generate(sc.CONFIGS["cns_tiny"])
    _set_dbs(ctx, str(tmp_path), d.contigs, d.reads)
    kw = dict(k=k, max_occ=max_occ) if max_occ else dict(k=k)
    index = sm.Index(d.contigs, k, max_occ or sm.MAX_OCC)
    if k == 16:
        assert (index.codes >= 2 ** 31).any()
    want = sm.model_seed(d.contigs, d.reads, index=index, **kw)
    assert len(want[0]) >= 1
    got = ctx.seed_run(**kw)
    _check_seed(got, want, "k%d" % k)
    st = ctx.seed_stats()
    assert st["entries"] == len(index.codes) and st["dropped_codes"] == index.dropped_codes
    assert ctx.index_last_stats()["device_builds"] == 1
