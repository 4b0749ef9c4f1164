"""GPU parity of `hinge filter` on reads too long for the LDS histogram of the mask/annotate kernel (more than 5120 coverage
bins: ~204 kb): the long-read tier (hinge_amd/csrc/filter_long_kernels.h) behind every route that runs the sweep.  The data set is
`ultra_long` (reads up to 1.3 Mb, tests/test_long_reads_oracle.py holds it to being non-vacuous); every file is the CPU oracle's,
byte for byte, and every case checks that the tier did run."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, clone_dataset, run_in
from test_long_reads_oracle import long_read_ids

pytestmark = pytest.mark.gpu

FILTER_FILES = [".mas", ".cmas", ".repeat.txt", ".hinges.txt", ".coverage.txt", ".cov.flag", ".self.flag"]
CLI_FILES = ["G.mas", "G.cmas", "G.repeat.txt", "G.hinges.txt", "G.coverage.txt", "G.cov.flag", "G.self.flag", "G.homologous.txt",
             "G.filtered.fasta", "G.max", "G.contained.txt", "G.garbage.txt", "G.killed.hinges", "G.edges.hinges", "G.edges.hinges2",
             "G.hinge.list", "G.deadends.txt", "G.hgraph", "G.debug", "G.edges.greedy", "G.edges.1", "G.edges.2", "G.edges.skipped",
             "edges.g_out.txt", "edges.fwd.backup.txt", "edges.bkw.backup.txt"]
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")


@pytest.fixture(scope="module")
def ultra(datasets, oracle_lib, tmp_path_factory):
    """(data set directory, directory with the oracle's filter + maximal + layout files, read lengths)."""
    from hinge_amd import formats
    src, _ = datasets("ultra_long")
    wd_o = clone_dataset(src, str(tmp_path_factory.mktemp("ultra_oracle")))
    assert run_in(wd_o, oracle_lib.oracle_filter, b"G", b"G.las", 0, b"G", b"nominal.ini", b"") == 0
    assert run_in(wd_o, oracle_lib.oracle_maximal, b"G", b"G.las", 0, b"G", b"nominal.ini") == 0
    assert run_in(wd_o, oracle_lib.oracle_layout, b"G", b"G.las", 0, b"G", b"G", b"nominal.ini") == 0
    rlen = formats.read_db_index(os.path.join(src, "G"))["rlen"]
    assert len(long_read_ids(rlen)) >= 20
    return src, wd_o, rlen


def _hip_filter(wd, ctx, packed):
    from hinge_amd import stages
    return run_in(wd, stages.run_filter, "G", "G.las", "G", "nominal.ini", False, 0, True, False, ctx, packed)


def _compare(wd_o, wd_h, files=FILTER_FILES, prefix="G"):
    bad = [s for s in files if not filecmp.cmp(os.path.join(wd_o, prefix + s), os.path.join(wd_h, prefix + s), shallow=False)]
    assert not bad, "differs from the oracle: %s" % bad


def _tables(ctx):
    mask, cmask, flags = ctx.get_masks()
    off, pos, typ, ish = ctx.get_annotations()
    nb, cov = ctx.get_coverage()
    return dict(min_cov=ctx.get_min_cov(), mask=mask, cmask=cmask, flags=flags, off=off, pos=pos, typ=typ, ish=ish, nb=nb, cov=cov,
                counters=tuple(ctx.counters()))


def _pileups(src, rlen):
    from hinge_amd import formats
    recs = formats.read_las(os.path.join(src, "G.las"))
    pile = formats.pileups_from_las(recs, rlen)
    return pile, int(recs.rec["aread"][0]), int(recs.rec["aread"][-1])


@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("packed", [False, True])
def test_filter_matches_oracle_on_ultra_long_reads(ultra, tmp_path, packed, general):
    """stages.run_filter: packed = the route of the executables (the one-sweep pass, the coverage bins from the sweep), else
    stats + median + mask_annotate and hinge_filter_coverage_bins; general = 1: no fast kernel, the general kernel owns the sweep."""
    from hinge_amd import capi
    src, wd_o, rlen = ultra
    wd_h = clone_dataset(src, str(tmp_path / "hip"))
    ctx = capi.Context(0)
    ctx.force_general_mask(general)
    assert _hip_filter(wd_h, ctx, packed) == 0
    assert ctx.long_reads() == len(long_read_ids(rlen)) > 0
    if packed:
        assert ctx.spec_stats()[0] >= 1, "the route of the executables must be the one-sweep pass"
    _compare(wd_o, wd_h)
    ctx.close()


# (band, bias) as in test_one_sweep_gpu.py: |bias| <= band leaves the long reads of the guard-band list to MODE_FINAL, beyond it
# every long read runs again
@pytest.mark.parametrize("band,bias,general", [(1, 1, 0), (0, 0, 0), (1, 4, 0), (2, -2, 1), (3, 2, 1), (1, -3, 1)])
def test_one_sweep_on_ultra_long_reads_under_forced_mispredictions(ultra, tmp_path, band, bias, general):
    from hinge_amd import capi
    src, wd_o, rlen = ultra
    wd_h = clone_dataset(src, str(tmp_path / "hip"))
    ctx = capi.Context(0)
    ctx.force_general_mask(general)
    ctx.debug_spec(band=band, sample=4096, bias=bias)
    assert _hip_filter(wd_h, ctx, True) == 0
    verified, off, outside, guard, pred, exact = ctx.spec_stats()
    assert verified >= 1
    if abs(bias) > band:
        assert outside >= 1, "band %d, bias %d: the verification must have ordered the part again" % (band, bias)
    if bias != 0 and abs(bias) <= band:
        assert off >= 1
    assert ctx.long_reads() > 0
    _compare(wd_o, wd_h)
    ctx.close()


def _oracle_tied_tables(ultra, tmp_path):
    """The tables of a context whose files were just compared with the oracle's (the route of the executables)."""
    from hinge_amd import capi
    src, wd_o, rlen = ultra
    wd_h = clone_dataset(src, str(tmp_path / "hip_ref"))
    ref = capi.Context(0)
    assert _hip_filter(wd_h, ref, True) == 0
    _compare(wd_o, wd_h)
    want = _tables(ref)
    ref.close()
    return want


def _same_tables(got, want):
    assert got["min_cov"] == want["min_cov"] and got["counters"] == want["counters"]
    for k in ("mask", "cmask", "flags", "off", "pos", "typ", "ish", "nb", "cov"):
        assert np.array_equal(got[k], want[k]), k


def test_hinge_filter_run_on_ultra_long_reads(ultra, tmp_path):
    """hinge_filter_run (sweep, finish and hinges without a host round trip) and hinge_filter_sweep + hinge_filter_hinges on plain
    hinge_set_pileups: the tables of a context whose files are the oracle's."""
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    src, wd_o, rlen = ultra
    want = _oracle_tied_tables(ultra, tmp_path)
    pile, r0, r1 = _pileups(src, rlen)
    P = default_filter_params()
    for run in (False, True):
        ctx = capi.Context(0)
        ctx.set_reads(rlen, None)
        ctx.set_pileups(r0, r1, pile.row_ptr, pile.a_span, pile.b_span, pile.b_flag)
        ctx.coverage_out(True)
        if run:
            ctx.filter_run(P)
            ctx.check()
        else:
            ctx.set_min_cov(P.min_cov)
            ctx.filter_sweep(P)
            ctx.filter_hinges(P)
        assert ctx.long_reads() == len(long_read_ids(rlen))
        _same_tables(_tables(ctx), want)
        ctx.close()


@pytest.mark.parametrize("general", [0, 1])
def test_long_reads_of_the_guard_band_list_run_in_mode_final(ultra, tmp_path, general):
    """A wide band with an exact prediction: the verification keeps the sweep, and long reads with a bin inside the band are on the
    guard-band list - the long-read tier's MODE_FINAL launch over that list decides them (not its re-run of every long read, which
    the mispredicted cases above cover)."""
    from hinge_amd import capi
    src, wd_o, rlen = ultra
    wd_h = clone_dataset(src, str(tmp_path / "hip"))
    ctx = capi.Context(0)
    ctx.force_general_mask(general)
    ctx.debug_spec(band=3, sample=4096, bias=0)
    assert _hip_filter(wd_h, ctx, True) == 0
    verified, off, outside, guard, pred, exact = ctx.spec_stats()
    n_long, n_final = ctx.long_reads(), ctx.long_reads_final()
    print("guard-band list %d reads, long reads %d, of them on the list %d" % (guard, n_long, n_final))
    assert verified >= 1 and outside == 0 and guard > 0
    assert 0 < n_final < n_long, "long reads on the guard-band list: %d of %d" % (n_final, n_long)
    _compare(wd_o, wd_h)
    ctx.close()


def test_one_context_through_a_coarse_reso_and_back(ultra, tmp_path):
    """reso 40, then a reso at which the longest read fits the LDS slot (no long read for those parameters), then reso 40 again on
    the same context and part: the list of long reads is built again, the third pass gives what a fresh context gives."""
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    src, wd_o, rlen = ultra
    want = _oracle_tied_tables(ultra, tmp_path)
    pile, r0, r1 = _pileups(src, rlen)
    ctx = capi.Context(0)
    ctx.set_reads(rlen, None)
    ctx.set_pileups(r0, r1, pile.row_ptr, pile.a_span, pile.b_span, pile.b_flag)
    ctx.coverage_out(True)
    for reso, n_long in ((40, len(long_read_ids(rlen))), (400, 0), (40, len(long_read_ids(rlen)))):
        P = default_filter_params()
        P.reso = reso
        assert (int(np.max(rlen)) + P.cut_off) // 400 + 4 <= 5120
        ctx.set_min_cov(P.min_cov)
        ctx.filter_sweep(P)
        ctx.filter_hinges(P)
        assert ctx.long_reads() == n_long, "reso %d" % reso
        if reso == 40:
            _same_tables(_tables(ctx), want)
    # the two-sweep calls take the same turn
    for reso in (400, 40):
        P = default_filter_params()
        P.reso = reso
        ctx.set_min_cov(P.min_cov)
        ctx.filter_stats_median(P, fetch=True)
        ctx.filter_mask_annotate(P)
        ctx.filter_hinges(P)
        assert ctx.long_reads() == (0 if reso == 400 else len(long_read_ids(rlen)))
    _same_tables(_tables(ctx), want)
    ctx.close()


def test_a_read_of_2_to_the_30_bases_is_refused_before_any_launch():
    """The annotation code packs position << 1 | type into an int: HINGE_E_CAPACITY from the first call of a pass."""
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    rlen = np.array([6000, 1 << 30, 6000], np.int32)
    row_ptr = np.array([0, 1, 1, 2], np.int64)
    a_span = np.array([[0, 5000], [100, 5900]], np.int32)
    b_span = np.array([[0, 5000], [100, 5900]], np.int32)
    b_flag = np.array([2, 0], np.uint32)   # bread | comp << 31
    P = default_filter_params()
    ctx = capi.Context(0)
    ctx.set_reads(rlen, None)
    ctx.set_min_cov(P.min_cov)
    ctx.set_pileups(0, 2, row_ptr, a_span, b_span, b_flag)
    for call in (lambda: ctx.filter_stats(P), lambda: ctx.filter_mask_annotate(P), lambda: ctx.filter_sweep(P), lambda: ctx.filter_run(P)):
        with pytest.raises(capi.HingeError) as ex:
            call()
        assert ex.value.code == capi.HINGE_E_CAPACITY and "2^30" in str(ex.value)
    ctx.close()


@pytest.mark.parametrize("env", [{}, {"HINGE_FINAL_BATCH": "0"}, {"HINGE_K2_BATCH": "0"}])
def test_batched_calls_with_one_ultra_long_part(ultra, datasets, tmp_path, monkeypatch, env):
    """Two resident parts through the *_batch_async calls, `ultra_long` and `tiny`: only the first has long reads.  The tables of
    the ultra_long part are those of a context whose files were just compared with the oracle's; the tiny part's those of its own
    single-part pass; twice, the second time on warm buffers."""
    from hinge_amd import capi, formats
    from hinge_amd.config import default_filter_params
    src, wd_o, rlen = ultra
    P = default_filter_params()
    want_u = _oracle_tied_tables(ultra, tmp_path)
    tsrc, _ = datasets("tiny")
    trlen = formats.read_db_index(os.path.join(tsrc, "G"))["rlen"]
    parts = [(rlen,) + _pileups(src, rlen), (trlen,) + _pileups(tsrc, trlen)]

    def make(part):
        rl, pile, r0, r1 = part
        ctx = capi.Context(0)
        ctx.set_reads(rl, None)
        ctx.set_min_cov(P.min_cov)
        span16, max_pile, in_range = capi.pack_spans(pile.row_ptr, pile.a_span, rl)
        ctx.set_pileups_packed(r0, r1, pile.row_ptr, pile.a_span, pile.b_span, pile.b_flag, span16, max_pile, in_range)
        ctx.coverage_out(True)
        return ctx

    t = make(parts[1])
    t.filter_sweep(P)
    t.filter_hinges(P)
    assert t.long_reads() == 0
    want_t = _tables(t)
    t.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctxs = [make(p) for p in parts]
    for _ in range(2):
        for c in ctxs:
            c.set_min_cov(P.min_cov)
        capi.sweep_batch_async(ctxs, P)
        capi.finish_batch_async(ctxs, P)
        capi.hinges_batch_async(ctxs, P)
        for c, w in zip(ctxs, (want_u, want_t)):
            c.check()
            got = _tables(c)
            assert got["min_cov"] == w["min_cov"] and got["counters"] == w["counters"]
            for k in ("mask", "cmask", "flags", "off", "pos", "typ", "ish", "nb", "cov"):
                assert np.array_equal(got[k], w[k]), k
        assert ctxs[0].long_reads() == len(long_read_ids(rlen)) and ctxs[1].long_reads() == 0
    for c in ctxs:
        c.close()


def test_coverage_bins_of_ultra_long_reads(ultra):
    """hinge_filter_coverage_bins (cutoff 0) against the oracle's .coverage.txt, read by read; the long reads are there."""
    from hinge_amd import capi
    src, wd_o, rlen = ultra
    pile, r0, r1 = _pileups(src, rlen)
    ctx = capi.Context(0)
    ctx.set_reads(rlen, None)
    ctx.set_pileups(r0, r1, pile.row_ptr, pile.a_span, pile.b_span, pile.b_flag)
    nb, cov = ctx.coverage_bins(r0, r1, 40, 0)
    ctx.close()
    off = np.concatenate([[0], np.cumsum(nb.astype(np.int64))])
    ids = set(int(i) for i in long_read_ids(rlen))
    seen = 0
    for l in open(os.path.join(wd_o, "G.coverage.txt")):
        t = l.split()
        i = int(t[1])
        want = np.array([int(x.split(",")[1]) for x in t[2:]], np.int64)
        got = cov[off[i - r0]:off[i - r0 + 1]]
        assert len(want) == len(got) and np.array_equal(want, got), "read %d" % i
        if i in ids:
            seen += 1
            assert len(want) > 5120
    assert seen == len(ids) > 0


def _run(wd, *args, env=None):
    r = subprocess.run([HINGE] + list(args), cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    assert r.returncode == 0, r.stdout.decode()[-2000:]


def test_executables_on_ultra_long_reads(ultra, tmp_path):
    """Reads_filter, get_maximal_reads and hinging, then hinge_pipeline: every file the oracle's."""
    src, wd_o, rlen = ultra
    wd_h = clone_dataset(src, str(tmp_path / "cli"))
    for sub, extra in (("filter", []), ("maximal", []), ("layout", ["-o", "G"])):
        _run(wd_h, sub, "--db", "G", "--las", "G.las", "-x", "G", "--config", "nominal.ini", *extra)
    _compare(wd_o, wd_h, CLI_FILES, "")
    assert os.path.getsize(os.path.join(wd_h, "G.edges.hinges")) > 0 and os.path.getsize(os.path.join(wd_h, "G.max")) > 0
    wd_p = clone_dataset(src, str(tmp_path / "pipeline"))
    _run(wd_p, "pipeline", "--db", "G", "--las", "G.las", "-x", "G", "--config", "nominal.ini", "-o", "G")
    _compare(wd_o, wd_p, CLI_FILES, "")
    # the general kernel in front of the long-read tier (no fast kernel)
    wd_g = clone_dataset(src, str(tmp_path / "general"))
    _run(wd_g, "filter", "--db", "G", "--las", "G.las", "-x", "G", "--config", "nominal.ini", env=dict(os.environ, HINGE_DEBUG_GENERAL_MASK="1"))
    _compare(wd_o, wd_g)


@pytest.mark.parametrize("sweep", [False, True])
def test_malformed_pileup_of_a_long_read_is_still_a_range_error(ultra, sweep):
    """One coordinate beyond rlen + cut_off on a long read: HINGE_E_RANGE with ST_RANGE's own message, from the long-read tier."""
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    src, wd_o, rlen = ultra
    pile, r0, r1 = _pileups(src, rlen)
    ids = [int(i) for i in long_read_ids(rlen) if pile.row_ptr[i + 1] > pile.row_ptr[i]]
    i = ids[len(ids) // 2]
    a_span = pile.a_span.copy()
    a_span[int(pile.row_ptr[i]), 1] = int(rlen[i]) + 300 + 2000
    P = default_filter_params()
    ctx = capi.Context(0)
    ctx.set_reads(rlen, None)
    ctx.set_min_cov(P.min_cov)
    ctx.set_pileups(r0, r1, pile.row_ptr, a_span, pile.b_span, pile.b_flag)
    with pytest.raises(capi.HingeError) as ex:
        if sweep:
            ctx.filter_sweep(P)
        else:
            ctx.filter_stats_median(P, fetch=True)
            ctx.filter_mask_annotate(P)
    assert ex.value.code == capi.HINGE_E_RANGE and "beyond read length + cut_off" in str(ex.value)
    assert ctx.long_reads() > 0
    ctx.close()


def test_no_long_read_no_long_tier(datasets, oracle_lib, tmp_path):
    """The control: `long_reads` (4-120 kb, general-kernel hand-backs included) never launches the tier."""
    from hinge_amd import capi
    src, _ = datasets("long_reads")
    wd_o = clone_dataset(src, str(tmp_path / "oracle"))
    wd_h = clone_dataset(src, str(tmp_path / "hip"))
    assert run_in(wd_o, oracle_lib.oracle_filter, b"G", b"G.las", 0, b"G", b"nominal.ini", b"") == 0
    ctx = capi.Context(0)
    assert _hip_filter(wd_h, ctx, True) == 0
    assert ctx.fallback_reads() > 0 and ctx.long_reads() == 0
    _compare(wd_o, wd_h)
    ctx.close()
