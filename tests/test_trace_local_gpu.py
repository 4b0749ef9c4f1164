"""`hinge paf2las --ends local` on the GPU: hinge_trace_local value for value against the numpy model
(tests/trace_local_common.py) - status, final W, end points, trace, diffs, score - and the chain PAF with independently moved end
points -> paf2las --ends local -> .las -> `hinge consensus` against the reference's own consensus program on the same .las."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import consensus_common as cc
import trace_common as tc
import trace_local_common as lc
import trace_refine_common as rc
from hinge_amd import formats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")
NAMES = ("aread", "bread", "comp", "abpos", "aepos", "bbpos", "bepos")


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    return capi.Context(0)


def _set_dbs(ctx, wd, contigs, reads):
    from hinge_amd import capi
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "draft"), np.asarray([len(c) for c in contigs], np.int32), bases=contigs)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return capi.Consensus(ctx, os.path.join(wd, "draft"), os.path.join(wd, "reads"))


def _check(got, want, placements, tspace):
    """got = Context.trace_local's tuple, want = lc.model_local's list."""
    alns, trace, diffs, status, score = got
    assert len(alns) == len(want) == len(placements)
    at = 0
    for x, (st, w, ends, tr, df, sc) in enumerate(want):
        p = placements[x]
        assert (int(status[x, 0]), int(status[x, 1])) == (st, w), (x, p, status[x], st, w)
        assert int(alns[x]["trace_off"]) == at
        coords = (p[0], p[1], p[2]) + (tuple(ends) if st == tc.OK else tuple(p[3:7]))     # the record's, or as given
        assert tuple(int(alns[x][n]) for n in NAMES) == tuple(int(v) for v in coords), (x, p, alns[x], ends)
        if st == tc.OK:
            n = int(alns[x]["tlen"])
            assert n == len(tr) == 2 * tc.n_segments(ends[0], ends[1], tspace)
            assert trace[at:at + n].tolist() == tr, (x, p)
            assert int(diffs[x]) == df == sum(tr[0::2]) and int(score[x]) == sc
            at += n
        else:
            assert int(alns[x]["tlen"]) == 0 and int(diffs[x]) == 0 and int(score[x]) == 0
    assert at == len(trace)
    assert 0xffff not in trace.tolist() or tspace > 125


@pytest.fixture(scope="module")
def hand():
    contigs, reads, pl, calls = lc.hand_cases()
    want, stats = {}, {}
    for label, names, kw in calls:
        stats[label] = {}
        want[label] = lc.model_local(contigs, reads, [pl[n] for n in names], stats=stats[label], **kw)
    return contigs, reads, pl, calls, want, stats


def test_hand_cases_equal_the_model(ctx, hand, tmp_path):
    """All placements of a call together: W = 64 (two 64-cell chunks per anti-diagonal) and W = 8 as the first band, both strands,
    one- and two-byte trace values, alignments that begin in row 0 and in column 0, a start cell outside the band, the tandem
    repeat's equal maxima, an unrelated pair (EMPTY after the last round), a diagonal 90 off that is found at 2 W."""
    contigs, reads, pl, calls, want, stats = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    seen = set()
    for label, names, kw in calls:
        ps = [pl[n] for n in names]
        got = ctx.trace_local(ps, **kw)
        _check(got, want[label], ps, kw["tspace"])
        seen |= set(got[3][:, 0].tolist())
        st = ctx.trace_stats()
        assert st["empty_widened"] == stats[label]["empty_widened"] and st["rounds"] == stats[label]["rounds"], label
        assert st["empty"] == sum(w[0] == lc.EMPTY for w in want[label]) and st["dropped"] == sum(w[0] != tc.OK for w in want[label])
    assert {tc.OK, tc.TOUCHED, lc.EMPTY} <= seen
    by = dict(zip(calls[0][1], want["w64"]))
    assert calls[0][0] == "w64" and by["off_diagonal"][:2] == (tc.OK, 128) and by["unrelated"][:2] == (lc.EMPTY, 256) and stats["w64"]["empty_widened"] == 3
    # an identical stretch without room: hinge_trace_run's own record
    ident = [pl["identical"]]
    a, t, d, s, sc = ctx.trace_local(ident, 100, 64, 1024)
    a0, t0, d0, s0 = ctx.trace_run(ident, 100, 64, 1024)
    assert a.tobytes() == a0.tobytes() and t.tolist() == t0.tolist() and d.tolist() == d0.tolist() and s.tolist() == s0.tolist() and sc.tolist() == [300]
    # hinge_trace_refine and hinge_trace_run after it, on the same context: their own kernels and results
    want_r = rc.model_refine(contigs, reads, ident, 100, 64, 1024)
    a1, t1, d1, s1, sc1 = ctx.trace_refine(ident, 100, 64, 1024)
    assert s1.tolist() == [[tc.OK, 64]] and t1.tolist() == want_r[0][3] and sc1.tolist() == [300] and ctx.trace_stats()["empty_widened"] == 0


def test_each_hand_case_alone(ctx, hand, tmp_path):
    """No dependence on the neighbours: every placement of every call by itself, under that call's arguments."""
    contigs, reads, pl, calls, want, stats = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    for label, names, kw in calls:
        for k, n in enumerate(names):
            _check(ctx.trace_local([pl[n]], **kw), want[label][k:k + 1], [pl[n]], kw["tspace"])


def test_environment_defaults(ctx, hand, tmp_path, monkeypatch):
    contigs, reads, pl, calls, want, stats = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    by = {label: (names, kw) for label, names, kw in calls}
    names, kw = by["outside_w8_64"]                                              # extend 0, through HINGE_TRACE_EXTEND
    assert kw["extend"] == 0
    monkeypatch.setenv("HINGE_TRACE_EXTEND", "0")
    ps = [pl[n] for n in names]
    _check(ctx.trace_local(ps, kw["tspace"], kw["band"], kw["band_max"]), want["outside_w8_64"], ps, kw["tspace"])
    monkeypatch.delenv("HINGE_TRACE_EXTEND")
    names, kw = by["min_score_1"]                                                # the mode's own default (24) gives way to HINGE_TRACE_MIN_SCORE
    ps = [pl[n] for n in names]
    assert ctx.trace_local(ps, kw["tspace"], kw["band"], kw["band_max"])[3][0].tolist() == [lc.EMPTY, 64]
    monkeypatch.setenv("HINGE_TRACE_MIN_SCORE", "1")
    _check(ctx.trace_local(ps, kw["tspace"], kw["band"], kw["band_max"]), want["min_score_1"], ps, kw["tspace"])
    monkeypatch.delenv("HINGE_TRACE_MIN_SCORE")
    names, kw = by["scores_2_3"]
    monkeypatch.setenv("HINGE_TRACE_MATCH", "2")
    monkeypatch.setenv("HINGE_TRACE_DIFF", "3")
    ps = [pl[n] for n in names]
    _check(ctx.trace_local(ps, kw["tspace"], kw["band"], kw["band_max"], min_score=kw["min_score"]), want["scores_2_3"], ps, kw["tspace"])
    monkeypatch.delenv("HINGE_TRACE_MATCH")
    monkeypatch.delenv("HINGE_TRACE_DIFF")
    # band and band_max from their defaults (128, 1024)
    names, kw = by["w64"]
    ps = [pl[n] for n in names if n != "unrelated"]                              # (an unrelated pair would pay all four rounds)
    _check(ctx.trace_local(ps, 100), lc.model_local(contigs, reads, ps, 100), ps, 100)


def test_many_placements_in_several_batches(ctx, tmp_path, monkeypatch):
    contigs, reads, pl = lc.perturbed_many()
    assert len(pl) == 130
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    want = lc.model_local(contigs, reads, pl, 100)
    assert sum(w[0] == tc.OK for w in want) >= 120
    monkeypatch.setenv("HINGE_TRACE_SCRATCH_BYTES", "400000")                    # 130 x ~230 rows x 64 bytes = 1.9 MB of directions
    _check(ctx.trace_local(pl, 100), want, pl, 100)
    st = ctx.trace_stats()
    assert st["batches"] >= 3 and st["runs"] >= 130 and st["scratch_bytes"] <= 400000
    monkeypatch.delenv("HINGE_TRACE_SCRATCH_BYTES")
    _check(ctx.trace_local(pl, 100), want, pl, 100)
    assert ctx.trace_stats()["batches"] == ctx.trace_stats()["rounds"]


def test_empty_call_and_refusals(ctx, hand, tmp_path):
    from hinge_amd import capi
    contigs, reads, pl, calls, want, stats = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    alns, trace, diffs, status, score = ctx.trace_local(np.zeros((0, 7), np.int64), 100)
    assert len(alns) == 0 and len(trace) == 0 and len(diffs) == 0 and len(status) == 0 and len(score) == 0
    good = pl["plain"]
    for kw in (dict(match=16), dict(diff=16), dict(match=-1), dict(diff=-2), dict(extend=32768), dict(extend=-2), dict(band=12), dict(band=64, band_max=32), dict(band_max=4096)):
        with pytest.raises(capi.HingeError) as e:
            ctx.trace_local([good], 100, **kw)
        assert e.value.code == capi.HINGE_E_ARG, kw
    with pytest.raises(capi.HingeError) as e:
        ctx.trace_local([good, (0, 0, 0, 100, 100, 0, 10)], 100)
    assert e.value.code == capi.HINGE_E_RANGE
    with pytest.raises(capi.HingeError) as e:
        ctx.trace_local([good, (0, len(reads), 0, 100, 200, 0, 10)], 100)
    assert e.value.code == capi.HINGE_E_RANGE
    # a trace array that holds the given placement's segments (4) but not the widened one's (5: no room at the front, 50 at the back)
    good = pl["off_diagonal"]
    assert tc.n_segments(good[3], good[4], 100) == 4 and tc.n_segments(*lc.widen(good, 3000, len(reads[good[1]]), 50)[3:5], 100) == 5
    a = np.zeros(1, dtype=capi.CNS_ALN_DTYPE)
    for name, v in zip(NAMES, good):
        a[name] = v
    out, tr, df, st, sc, nt = np.zeros(1, capi.CNS_ALN_DTYPE), np.zeros(10, np.uint16), np.zeros(1, np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32), C.c_int64(0)
    ends = np.asarray([50, 1, 2, 24], np.int32)
    args = lambda cap: (ctx.h, 1, a.ctypes.data, 100, 64, 128, ends.ctypes.data, out.ctypes.data, tr.ctypes.data, cap, C.byref(nt), df.ctypes.data, st.ctypes.data, sc.ctypes.data)
    assert ctx.lib.hinge_trace_local(*args(8)) == capi.HINGE_E_CAPACITY
    assert ctx.lib.hinge_trace_local(*args(10)) == capi.HINGE_OK and st.tolist() == [tc.OK, 128]
    # NULL ends = the defaults
    assert ctx.lib.hinge_trace_local(*(args(10)[:6] + (None,) + args(10)[7:])) == capi.HINGE_OK
    assert (int(out[0]["abpos"]), int(out[0]["aepos"])) == lc.model_local(contigs, reads, [good], 100, 64, 128)[0][2][:2]


# ---- end to end through the executables -----------------------------------------------------------------------------------------------
def _run(cmd, wd):
    r = subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return r.stdout.decode()


def _write_paf(d, wd, pls):
    """Placements (B in the strand frame) as PAF lines: a `-` line's query coordinates are on the read's forward strand."""
    p = np.asarray(pls, np.int64)
    blen = np.asarray([len(d.reads[b]) for b in p[:, 1]], np.int64)
    qs = np.where(p[:, 2] == 1, blen - p[:, 6], p[:, 5])
    qe = np.where(p[:, 2] == 1, blen - p[:, 5], p[:, 6])
    formats.write_paf(os.path.join(wd, "map.paf"), np.asarray([len(r) for r in d.reads]), p[:, 1], p[:, 0], p[:, 2], qs, qe, p[:, 3], p[:, 4], rlen_b=np.asarray([len(c) for c in d.contigs]))


def test_chain_perturbed_paf_local_consensus_cns_tiny(oracle_lib, tmp_path):
    wd = str(tmp_path)
    d0 = cc.make("cns_tiny", wd)
    d, pls = lc.perturbed_cns_tiny()                                               # every end point moved independently by up to 60
    assert len(pls) == len(d0.rec) and any(p[2] for p in pls) and not all(p[2] for p in pls)
    _write_paf(d, wd, pls)
    os.remove(os.path.join(wd, "draft.reads.las"))                                 # the generator's own: the chain writes its own
    summary = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "draft.reads.las", "--ends", "local"], wd)
    assert "%d placements read, %d written" % (len(pls), len(pls)) in summary and "dropped 0" in summary and "clipped out 0," in summary and "end points moved by" in summary
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    assert las.tspace == d.spec.tspace and len(las.rec) == len(pls)
    # the records are the model's, sorted by (aread, bread, the record's abpos)
    want = lc.model_local(d.contigs, d.reads, pls, d.spec.tspace)
    assert all(w[0] == tc.OK for w in want)
    want = [want[k] for k in sorted(range(len(pls)), key=lambda k: (pls[k][0], pls[k][1], want[k][2][0]))]
    tr = las.trace.astype(np.int64)
    for k, (r, w) in enumerate(zip(las.rec, want)):
        assert w[0] == tc.OK and (int(r["abpos"]), int(r["aepos"]), int(r["bbpos"]), int(r["bepos"])) == w[2] and int(r["diffs"]) == w[4]
        assert tr[las.trace_off[k]:las.trace_off[k + 1]].tolist() == w[3]
    hip = cc.run_product(wd)                                                       # exit status 0
    assert hip[0].count(b">Consensus") == len(d.contigs)
    ref = cc.run_reference(wd) or cc.run_oracle(oracle_lib, wd)                    # the reference's own program where it was built, else the restatement pinned to it
    assert hip[0] == ref[0] and hip[1] == ref[1]                                   # byte-identical FASTA and stdout
    # --scores and --min-score reach the library: at 2,3 with a minimum no 1 800-base read reaches, everything is clipped out
    s2 = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "none.las", "--ends", "local", "--scores", "2,3", "--min-score", "5000"], wd)
    assert "%d placements read, 0 written" % len(pls) in s2 and "clipped out %d," % len(pls) in s2


def test_ends_given_and_refine_write_what_they_wrote(tmp_path):
    """--ends given (and no --ends) and --ends refine are untouched by the third mode: given = the bytes that follow from the format
    and the plain model's traces (tc.model_run), refine = the records of rc.model_refine."""
    import struct
    wd = str(tmp_path)
    d = cc.make("cns_tiny", wd)
    assert d.spec.tspace <= 125
    pls = [(int(q["aread"]), int(q["bread"]), int(q["flags"] & 1), int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in d.rec]
    _write_paf(d, wd, pls)
    pls.sort(key=lambda p: (p[0], p[1], p[3]))
    want = struct.pack("<qi", len(pls), d.spec.tspace)
    for p, (st, w, tr, df) in zip(pls, tc.model_run(d.contigs, d.reads, pls, d.spec.tspace)):
        assert st == tc.OK
        want += struct.pack("<9i", len(tr), df, p[3], p[5], p[4], p[6], p[2], p[0], p[1]) + bytes(4) + bytes(tr)
    s0 = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "plain.las"], wd)
    s1 = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "given.las", "--ends", "given"], wd)
    assert open(os.path.join(wd, "plain.las"), "rb").read() == want
    assert open(os.path.join(wd, "given.las"), "rb").read() == want
    assert s0 == s1 and "clipped out" not in s0
    _run([HINGE, "paf2las", "draft", "reads", "map.paf", "refine.las", "--ends", "refine"], wd)
    ref = rc.model_refine(d.contigs, d.reads, pls, d.spec.tspace)
    assert all(r[0] == tc.OK for r in ref)
    want = struct.pack("<qi", len(pls), d.spec.tspace)
    for k in sorted(range(len(pls)), key=lambda k: (pls[k][0], pls[k][1], ref[k][2][0])):
        p, (st, w, e, tr, df, sc) = pls[k], ref[k]
        want += struct.pack("<9i", len(tr), df, e[0], e[2], e[1], e[3], p[2], p[0], p[1]) + bytes(4) + bytes(tr)
    assert open(os.path.join(wd, "refine.las"), "rb").read() == want
