"""`hinge paf2las --ends refine` on the GPU: hinge_trace_refine value for value against the numpy model
(tests/trace_refine_common.py) - status, final W, refined coordinates, trace, diffs, score - and the chain PAF with perturbed end
points -> paf2las --ends refine -> .las -> `hinge consensus` against the reference's own consensus program on the same .las."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import consensus_common as cc
import trace_common as tc
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
    """got = Context.trace_refine's tuple, want = rc.model_refine's list."""
    alns, trace, diffs, status, score = got
    assert len(alns) == len(want) == len(placements)
    at = 0
    for x, (st, w, ends, tr, df, sc) in enumerate(want):
        p = placements[x]
        assert (int(status[x, 0]), int(status[x, 1])) == (st, w), (x, p, status[x], st, w)
        assert int(alns[x]["trace_off"]) == at
        coords = (p[0], p[1], p[2]) + ((ends[0], ends[1], ends[2], ends[3]) if st == tc.OK else tuple(p[3:7]))     # refined, or as given
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
    contigs, reads, pl, calls = rc.hand_cases()
    want = {label: rc.model_refine(contigs, reads, [pl[n] for n in names], **kw) for label, names, kw in calls}
    return contigs, reads, pl, calls, want


def test_hand_cases_equal_the_model(ctx, hand, tmp_path):
    contigs, reads, pl, calls, want = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    seen = set()
    for label, names, kw in calls:
        ps = [pl[n] for n in names]
        got = ctx.trace_refine(ps, **kw)
        _check(got, want[label], ps, kw["tspace"])
        seen |= set(got[3][:, 0].tolist())
        if label == "noise_min_score_40":
            assert got[3][:, 0].tolist() == [tc.OK, rc.EMPTY, tc.OK]
            st = ctx.trace_stats()
            assert st["empty"] == 1 and st["dropped"] == 1
    assert {tc.OK, tc.WIDE, rc.EMPTY} <= seen
    # the identical stretch without room: hinge_trace_run's own record
    ident = [pl["identical"]]
    a, t, d, s, sc = ctx.trace_refine(ident, 100, 64, 1024)
    a0, t0, d0, s0 = ctx.trace_run(ident, 100, 64, 1024)
    assert a.tobytes() == a0.tobytes() and t.tolist() == t0.tolist() and d.tolist() == d0.tolist() and s.tolist() == s0.tolist() and sc.tolist() == [300]
    # the clipped tail: OK at the first W here, widened by hinge_trace_run on the same box
    tail = [pl["tail_touch"]]
    assert ctx.trace_refine(tail, 100, 16, 1024, extend=0, match=1, diff=15)[3].tolist() == [[tc.OK, 16]]
    assert ctx.trace_run(tail, 100, 16, 1024)[3][0, 1] > 16
    # a kept column on the band's edge still widens
    assert ctx.trace_refine([pl["touch_kept"]], 100, 16, 64)[3].tolist() == [[tc.OK, 32]]
    assert ctx.trace_stats()["widened"] == 1


def test_each_hand_case_alone(ctx, hand, tmp_path):
    """No dependence on the neighbours: every placement of every call by itself, under that call's arguments."""
    contigs, reads, pl, calls, want = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    for label, names, kw in calls:
        for k, n in enumerate(names):
            _check(ctx.trace_refine([pl[n]], **kw), want[label][k:k + 1], [pl[n]], kw["tspace"])


def test_environment_defaults(ctx, hand, tmp_path, monkeypatch):
    contigs, reads, pl, calls, want = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    label, names, kw = calls[1]                                                  # extend 0, through HINGE_TRACE_EXTEND
    assert kw["extend"] == 0
    monkeypatch.setenv("HINGE_TRACE_EXTEND", "0")
    ps = [pl[n] for n in names]
    _check(ctx.trace_refine(ps, kw["tspace"], kw["band"], kw["band_max"]), want[label], ps, kw["tspace"])
    monkeypatch.delenv("HINGE_TRACE_EXTEND")
    monkeypatch.setenv("HINGE_TRACE_MIN_SCORE", "40")
    label, names, kw = calls[5]
    assert kw["min_score"] == 40
    ps = [pl[n] for n in names]
    _check(ctx.trace_refine(ps, kw["tspace"], kw["band"], kw["band_max"]), want[label], ps, kw["tspace"])


def test_many_placements_in_several_batches(ctx, tmp_path, monkeypatch):
    contigs, reads, pl = rc.perturbed_many()
    assert len(pl) == 130
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    want = rc.model_refine(contigs, reads, pl, 100)
    monkeypatch.setenv("HINGE_TRACE_SCRATCH_BYTES", "400000")                    # 130 x ~230 rows x 64 bytes = 1.9 MB of directions
    _check(ctx.trace_refine(pl, 100), want, pl, 100)
    st = ctx.trace_stats()
    assert st["batches"] >= 3 and st["runs"] == 130 and st["scratch_bytes"] <= 400000 and st["empty"] == 0
    monkeypatch.delenv("HINGE_TRACE_SCRATCH_BYTES")
    _check(ctx.trace_refine(pl, 100), want, pl, 100)
    assert ctx.trace_stats()["batches"] == 1


def test_empty_call_and_refusals(ctx, hand, tmp_path):
    from hinge_amd import capi
    contigs, reads, pl, calls, want = hand
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    alns, trace, diffs, status, score = ctx.trace_refine(np.zeros((0, 7), np.int64), 100)
    assert len(alns) == 0 and len(trace) == 0 and len(diffs) == 0 and len(status) == 0 and len(score) == 0
    good = pl["undershoot"]
    for kw in (dict(match=16), dict(diff=16), dict(match=-1), dict(diff=-2), dict(extend=32768), dict(extend=-2)):
        with pytest.raises(capi.HingeError) as e:
            ctx.trace_refine([good], 100, **kw)
        assert e.value.code == capi.HINGE_E_ARG, kw
    with pytest.raises(capi.HingeError) as e:
        ctx.trace_refine([good, (0, 0, 0, 100, 100, 0, 10)], 100)
    assert e.value.code == capi.HINGE_E_RANGE
    # a trace array that holds the given placement's segments (4) but not the widened one's (6)
    assert tc.n_segments(good[3], good[4], 100) == 4 and tc.n_segments(good[3] - 50, good[4] + 50, 100) == 6
    a = np.zeros(1, dtype=capi.CNS_ALN_DTYPE)
    for name, v in zip(NAMES, good):
        a[name] = v
    out, tr, df, st, sc, nt = np.zeros(1, capi.CNS_ALN_DTYPE), np.zeros(12, np.uint16), np.zeros(1, np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32), C.c_int64(0)
    ends = np.asarray([50, 1, 2, 1], np.int32)
    args = lambda cap: (ctx.h, 1, a.ctypes.data, 100, 0, 0, ends.ctypes.data, out.ctypes.data, tr.ctypes.data, cap, C.byref(nt), df.ctypes.data, st.ctypes.data, sc.ctypes.data)
    assert ctx.lib.hinge_trace_refine(*args(8)) == capi.HINGE_E_CAPACITY
    assert ctx.lib.hinge_trace_refine(*args(12)) == capi.HINGE_OK and st[0] == tc.OK
    # NULL ends = the defaults
    assert ctx.lib.hinge_trace_refine(*(args(12)[:6] + (None,) + args(12)[7:])) == capi.HINGE_OK
    assert (int(out[0]["abpos"]), int(out[0]["aepos"])) == rc.model_refine(contigs, reads, [good], 100)[0][2][:2]


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


def test_chain_perturbed_paf_refine_consensus_cns_tiny(oracle_lib, tmp_path):
    wd = str(tmp_path)
    d0 = cc.make("cns_tiny", wd)
    d, pls = rc.perturbed_cns_tiny()
    assert len(pls) == len(d0.rec) and any(p[2] for p in pls) and not all(p[2] for p in pls)
    _write_paf(d, wd, pls)
    os.remove(os.path.join(wd, "draft.reads.las"))                                 # the generator's own: the chain writes its own
    summary = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "draft.reads.las", "--ends", "refine"], wd)
    assert "%d placements read, %d written" % (len(pls), len(pls)) in summary and "dropped 0" in summary and "clipped out 0," in summary and "end points moved by" in summary
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    assert las.tspace == d.spec.tspace and len(las.rec) == len(pls)
    # the records are the model's refined ones, sorted by (aread, bread, refined abpos)
    want = rc.model_refine(d.contigs, d.reads, pls, d.spec.tspace)
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


def test_ends_given_is_the_default_byte_for_byte(tmp_path):
    """Without --ends, and with --ends given, paf2las writes what it wrote before the option existed: the .las whose bytes follow
    from the format (align.h:98-110) and the plain model's traces (tc.model_run, which has no notion of refinement) - the header,
    then per placement in (aread, bread, abpos) order the 40-byte record and one byte per trace value."""
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
    assert s0 == s1 and "clipped out" not in s0 and "%d placements read, %d written" % (len(pls), len(pls)) in s0
