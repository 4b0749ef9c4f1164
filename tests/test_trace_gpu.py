"""`hinge paf2las` on the GPU: hinge_trace_run value for value against the numpy model (tests/trace_common.py), and the chain
PAF -> paf2las -> .las -> `hinge consensus` against the reference's own consensus program on the same .las."""
import collections
import os
import subprocess

import numpy as np
import pytest

import consensus_common as cc
import trace_common as tc
from hinge_amd import formats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")


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
    """got = Context.trace_run's tuple, want = tc.model_run's list: status, final W, trace and diffs of every placement."""
    alns, trace, diffs, status = got
    assert len(alns) == len(want) == len(placements)
    at = 0
    for x, (st, w, tr, df) in enumerate(want):
        assert (int(status[x, 0]), int(status[x, 1])) == (st, w), (x, placements[x], status[x], st, w)
        assert int(alns[x]["trace_off"]) == at
        for name, v in zip(("aread", "bread", "comp", "abpos", "aepos", "bbpos", "bepos"), placements[x]):
            assert int(alns[x][name]) == int(v)                                  # order kept
        if st == tc.OK:
            n = int(alns[x]["tlen"])
            assert n == len(tr) == 2 * tc.n_segments(placements[x][3], placements[x][4], tspace)
            assert trace[at:at + n].tolist() == tr, (x, placements[x])
            assert int(diffs[x]) == df == sum(tr[0::2])
            at += n
        else:
            assert int(alns[x]["tlen"]) == 0 and int(diffs[x]) == 0
    assert at == len(trace)
    assert 0xffff not in trace.tolist() or tspace > 125


def test_hand_cases_equal_the_model(ctx, tmp_path):
    contigs, reads, cases = tc.hand_cases()
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    pl = [p for _, p, _ in cases]
    assert any(p[2] for p in pl) and any(not p[2] for p in pl)                   # both strands
    _check(ctx.trace_run(pl, 100), tc.model_run(contigs, reads, pl, 100), pl, 100)
    for k in range(len(pl)):                                                      # each one alone: no dependence on its neighbours
        _check(ctx.trace_run(pl[k:k + 1], 100), tc.model_run(contigs, reads, pl[k:k + 1], 100), pl[k:k + 1], 100)
    # two-byte traces and a small band
    _check(ctx.trace_run(pl, 200, 8, 64), tc.model_run(contigs, reads, pl, 200, 8, 64), pl, 200)


@pytest.mark.parametrize("band", [1024, 2048])
def test_widest_bands_launch(ctx, tmp_path, band):
    """The LDS rings of the fill grow with W: 72 KiB at 1024 (beyond the default dynamic limit), 144 KiB at the largest legal band."""
    contigs, reads, cases = tc.hand_cases()
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    pl = [p for n, p, _ in cases if n in ("one_block", "alen_1", "comp_strand")]
    _check(ctx.trace_run(pl, 100, band, band), tc.model_run(contigs, reads, pl, 100, band, band), pl, 100)


def test_indels_widen_long_reads_drop_wide_segments_flagged(ctx, tmp_path):
    contigs, reads, pl = tc.indel_cases()
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    want = tc.model_run(contigs, reads, pl, 100, 16, 1024)
    got = ctx.trace_run(pl, 100, 16, 1024)
    _check(got, want, pl, 100)
    status = got[3]
    assert status[0].tolist()[0] == tc.OK and status[0, 1] in (32, 64) and status[1, 0] == tc.OK and status[1, 1] in (32, 64)
    assert status[3].tolist() == [tc.NO_PATH, 1024]                              # |blen - alen| > W_MAX: no record ...
    assert status[2].tolist() == [tc.OK, 16] and status[4].tolist() == [tc.OK, 16]   # ... its neighbours unaffected
    assert status[5].tolist() == [tc.WIDE, 512]                                  # 300 bases inserted inside one segment
    st = ctx.trace_stats()
    assert st["dropped"] == 2 and st["widened"] == 2 and st["rounds"] == 7
    # from the defaults (128 / 1024): the same verdicts
    _check(ctx.trace_run(pl, 100), tc.model_run(contigs, reads, pl, 100), pl, 100)


def test_many_placements_in_several_batches(ctx, tmp_path, monkeypatch):
    rng = np.random.default_rng(21)
    contig = rng.integers(0, 4, size=3000, dtype=np.uint8)
    reads, pl = [], []
    for x in range(130):
        ab = int(rng.integers(0, 2800))
        ae = ab + int(rng.integers(60, 200))
        seq = contig[ab:ae].copy()
        hit = rng.random(len(seq)) < 0.08
        seq[hit] = (seq[hit] + 1) % 4
        seq = np.delete(seq, rng.integers(0, len(seq), size=3))
        comp = int(x % 3 == 0)
        reads.append(tc.revcomp(seq) if comp else seq)
        pl.append((0, x, comp, ab, ae, 0, len(seq)))
    _set_dbs(ctx, str(tmp_path), [contig], reads)
    want = tc.model_run([contig], reads, pl, 100)
    monkeypatch.setenv("HINGE_TRACE_SCRATCH_BYTES", "400000")                    # 130 x ~130 rows x 64 bytes = 1.1 MB of directions
    _check(ctx.trace_run(pl, 100), want, pl, 100)
    st = ctx.trace_stats()
    assert st["batches"] >= 3 and st["runs"] == 130 and st["scratch_bytes"] <= 400000
    monkeypatch.delenv("HINGE_TRACE_SCRATCH_BYTES")
    _check(ctx.trace_run(pl, 100), want, pl, 100)
    assert ctx.trace_stats()["batches"] == 1


def test_empty_call_and_refusals(ctx, tmp_path):
    from hinge_amd import capi
    contigs, reads, cases = tc.hand_cases()
    _set_dbs(ctx, str(tmp_path), contigs, reads)
    alns, trace, diffs, status = ctx.trace_run(np.zeros((0, 7), np.int64), 100)
    assert len(alns) == 0 and len(trace) == 0 and len(diffs) == 0 and len(status) == 0
    good = cases[1][1]
    for bad in ((0, 0, 0, 100, 100, 0, 10), (0, 0, 0, 10, 20, 5, 5), (0, 0, 0, 0, 1001, 0, 10), (0, 0, 0, 0, 10, 0, 100000), (5, 0, 0, 0, 10, 0, 10), (0, -1, 0, 0, 10, 0, 10)):
        with pytest.raises(capi.HingeError) as e:
            ctx.trace_run([good, bad], 100)
        assert e.value.code == capi.HINGE_E_RANGE
    with pytest.raises(capi.HingeError) as e:
        ctx.trace_run([good], 100, 12, 64)                                       # not a multiple of 8
    assert e.value.code == capi.HINGE_E_ARG
    # a trace array that is too small
    import ctypes as C
    a = np.zeros(1, dtype=capi.CNS_ALN_DTYPE)
    for name, v in zip(("aread", "bread", "comp", "abpos", "aepos", "bbpos", "bepos"), good):
        a[name] = v
    out, tr, df, st, nt = np.zeros(1, capi.CNS_ALN_DTYPE), np.zeros(4, np.uint16), np.zeros(1, np.int32), np.zeros(2, np.int32), C.c_int64(0)
    rc = ctx.lib.hinge_trace_run(ctx.h, 1, a.ctypes.data, 100, 0, 0, out.ctypes.data, tr.ctypes.data, 4, C.byref(nt), df.ctypes.data, st.ctypes.data)
    assert rc == capi.HINGE_E_CAPACITY


# ---- the generator's own records as placements ---------------------------------------------------------------------------------------
def _placements(d):
    return [(int(q["aread"]), int(q["bread"]), int(q["flags"] & 1), int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in d.rec]


@pytest.fixture(scope="module")
def synth_sets(tmp_path_factory):
    from hinge_amd import synth_consensus as sc
    out = {}
    for name in ("cns_tiny", "cns_noisy"):
        d = sc.generate(sc.CONFIGS[name])
        pl = _placements(d)
        cache = {}
        out[name] = (d, pl, cache, tc.model_run(d.contigs, d.reads, pl, d.spec.tspace, 64, 1024, cache=cache), str(tmp_path_factory.mktemp(name)))
    return out


@pytest.mark.parametrize("name", ["cns_tiny", "cns_noisy"])
def test_generator_records_as_placements(ctx, synth_sets, name):
    d, pl, cache, want, wd = synth_sets[name]
    _set_dbs(ctx, wd, d.contigs, d.reads)
    got = ctx.trace_run(pl, d.spec.tspace, 64, 1024)
    status, diffs = got[3], got[2]
    assert int((status[:, 0] != tc.OK).sum()) == 0, collections.Counter(map(tuple, status.tolist()))    # zero dropped
    _check(got, want, pl, d.spec.tspace)
    # the generator's path is one path inside the band: an optimum cannot be worse
    assert (diffs <= d.rec["diffs"]).all()
    if name == "cns_noisy":
        got16 = ctx.trace_run(pl, d.spec.tspace, 16, 1024)
        assert int((got16[3][:, 0] != tc.OK).sum()) == 0 and int((got16[3][:, 1] > 16).sum()) > 0
        _check(got16, tc.model_run(d.contigs, d.reads, pl, d.spec.tspace, 16, 1024, cache=cache), pl, d.spec.tspace)
        assert ctx.trace_stats()["widened"] == int((got16[3][:, 1] > 16).sum())


# ---- end to end through the executables -----------------------------------------------------------------------------------------------
def _fasta(path, names, seqs, line=70):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n" % n)
            t = "".join("ACGT"[v] for v in s)
            for k in range(0, len(t), line):
                f.write(t[k:k + line] + "\n")


def _forward_query(d):
    """PAF query coordinates of the records: a `-` line's are on the read's forward strand."""
    r = d.rec
    comp = (r["flags"] & 1).astype(np.int64)
    blen = np.asarray([len(d.reads[b]) for b in r["bread"]], np.int64)
    qs = np.where(comp == 1, blen - r["bepos"], r["bbpos"])
    qe = np.where(comp == 1, blen - r["bbpos"], r["bepos"])
    return comp, qs, qe


def _run(cmd, wd):
    r = subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return r.stdout.decode()


def _check_chain(d, wd, summary):
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    assert las.tspace == d.spec.tspace
    key = lambda r: (int(r["aread"]), int(r["bread"]), int(r["flags"] & 1), int(r["abpos"]), int(r["aepos"]), int(r["bbpos"]), int(r["bepos"]))
    assert collections.Counter(map(key, las.rec)) == collections.Counter(map(key, d.rec))           # (a)
    order = [(int(r["aread"]), int(r["bread"]), int(r["abpos"])) for r in las.rec]
    assert order == sorted(order)
    tb = 1 if las.tspace <= 125 else 2
    tr = las.trace.astype(np.int64) if tb == 1 else np.ascontiguousarray(las.trace).view("<u2").astype(np.int64)
    for k, r in enumerate(las.rec):
        t = tr[las.trace_off[k] // tb:las.trace_off[k + 1] // tb]
        assert len(t) == r["tlen"] and int(t[0::2].sum()) == r["diffs"] and int(t[1::2].sum()) == r["bepos"] - r["bbpos"]
    assert "%d placements read, %d written" % (len(d.rec), len(d.rec)) in summary and "dropped 0" in summary
    hip = cc.run_product(wd)                                                       # (c): exit status 0, i.e. no CNS_ST_WAVES
    assert hip[0].count(b">Consensus") == len(d.contigs)
    ref = cc.run_reference(wd)
    if ref is None:
        pytest.skip("oracle/_ref/consensus was never built: the reference half of this test needs it")
    assert hip[0] == ref[0] and hip[1] == ref[1]                                  # (b): byte-identical FASTA and stdout


def test_chain_from_fasta_and_paf_alone_cns_tiny(tmp_path):
    """correct-head -> fasta2db -> paf2las (--read-names for the reads, the id between slashes for the contigs) -> consensus."""
    from hinge_amd import synth_consensus as sc
    d = sc.generate(sc.CONFIGS["cns_tiny"])
    wd = str(tmp_path)
    _fasta(os.path.join(wd, "draft.raw.fasta"), ["Draft%d some text" % i for i in range(len(d.contigs))], d.contigs)
    _fasta(os.path.join(wd, "reads.fasta"), ["read_%d len=%d" % (i, len(r)) for i, r in enumerate(d.reads)], d.reads)
    _run([HINGE, "correct-head", "draft.raw.fasta", "draft.fasta", "draft_map.txt"], wd)
    _run([HINGE, "fasta2db", "draft.fasta", "draft"], wd)
    _run([HINGE, "fasta2db", "reads.fasta", "reads"], wd)
    comp, qs, qe = _forward_query(d)
    assert comp.any() and not comp.all()                                           # (d): `-` and `+` lines
    with open(os.path.join(wd, "map.paf"), "w") as f:
        for r, c, s, e in zip(d.rec, comp.tolist(), qs.tolist(), qe.tolist()):
            a, b = int(r["aread"]), int(r["bread"])
            f.write("read_%d\t%d\t%d\t%d\t%s\tm000_000/%d/0_%d\t%d\t%d\t%d\t0\t0\t255\n" % (b, len(d.reads[b]), s, e, "-" if c else "+", a + 1, len(d.contigs[a]), len(d.contigs[a]),
                                                                                        int(r["abpos"]), int(r["aepos"])))
    with open(os.path.join(wd, "nominal.ini"), "w") as f:
        f.write("[consensus]\nmin_length = 500;\n")
    summary = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "draft.reads.las", "--read-names", "reads.fasta"], wd)
    _check_chain(d, wd, summary)


def test_chain_two_byte_traces_cns_twobyte(tmp_path):
    wd = str(tmp_path)
    d = cc.make("cns_twobyte", wd)
    comp, qs, qe = _forward_query(d)
    assert comp.any()
    formats.write_paf(os.path.join(wd, "map.paf"), np.asarray([len(r) for r in d.reads]), d.rec["bread"], d.rec["aread"], comp, qs, qe, d.rec["abpos"], d.rec["aepos"],
                      rlen_b=np.asarray([len(c) for c in d.contigs]))
    os.remove(os.path.join(wd, "draft.reads.las"))                                 # the generator's own: the chain writes its own
    summary = _run([HINGE, "paf2las", "draft", "reads", "map.paf", "draft.reads.las", "--tspace", "200"], wd)
    _check_chain(d, wd, summary)
