"""GPU parity of k_mask_annotate_q20 on the 16|16 span copy - where it reads its per-read tables (list entry, row bounds, length,
bin count, coverage offset) through scalar loads - against the general mask / annotate kernel on the same pile-ups
(hinge_debug_force_general_mask), table by table: masks, coverage masks, flags, coverage bins and their counts, annotation
offsets, positions, types, the hinge marks and the counters (work-list size among them); and against the CPU oracle's files where
a data set has them.  The look-ups change no result by construction: what these cases guard against is a wrong or out-of-range
look-up (a fault, another read's row) at the edges - the part's last row, empty rows, handed-back reads, a wavefront's last draw,
the parts of a ragged batched launch.  Few persistent workgroups (HINGE_K2_WGS=8), so that every wavefront draws dozens of reads
in a row."""
import filecmp
import os

import numpy as np
import pytest

from conftest import clone_dataset, run_in, write_ini

pytestmark = pytest.mark.gpu

FILTER_FILES = [".mas", ".cmas", ".repeat.txt", ".hinges.txt", ".coverage.txt", ".cov.flag", ".self.flag"]
TABLES = ("mask", "cmask", "flags", "off", "pos", "typ", "ish", "nb", "cov")
# the three passes K2 has an instance for: the exact MIN_COV (SPEC = 0), the one-sweep pass with band 1 (SPEC = 1) and with any
# band (SPEC = 2); the prediction is biased so that reads land on the guard-band list
ROUTES = ["exact", ("spec", 1, 1), ("spec", 2, -2)]


def _env(monkeypatch, wgs=8, **more):
    monkeypatch.setenv("HINGE_K2_WGS", str(wgs))
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _pile_of(datasets, name):
    from hinge_amd import formats
    src, _ = datasets(name)
    rlen = formats.read_db_index(os.path.join(src, "G"))["rlen"]
    recs = formats.read_las(os.path.join(src, "G.las"))
    pile = formats.pileups_from_las(recs, rlen)
    return rlen, pile, int(recs.rec["aread"][0]), int(recs.rec["aread"][-1])


def _cut(pile, cuts):
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s, e = int(pile.row_ptr[a]), int(pile.row_ptr[b])
        rp = np.ascontiguousarray(np.clip(pile.row_ptr, s, e) - s)       # (n_reads + 1 entries: empty rows outside the part)
        parts.append((a, b - 1, rp, pile.a_span[s:e].copy(), pile.b_span[s:e].copy(), pile.b_flag[s:e].copy()))
    return parts


def _make(rlen, part, P, sums):
    """A context as an ingest sets it up: the 16|16 span copy, facts, bins and (sums) the sums."""
    from hinge_amd import capi
    r0, r1, rp, a, b, f = part
    ctx = capi.Context(0)
    ctx.set_reads(rlen, None)
    ctx.set_min_cov(P.min_cov)
    span16, max_pile, in_range = capi.pack_spans(rp, a, rlen)
    assert in_range, "the 16|16 copy needs every coordinate inside its read"
    ctx.set_pileups_packed(r0, r1, rp, a, b, f, span16, max_pile, in_range)
    ctx.set_pile_bins(capi.pile_bins(rp[r0:r1 + 2], a, rlen[r0:r1 + 1], 40), 40)
    if sums:
        ctx.set_pile_cov(capi.pile_cov(rp[r0:r1 + 2], a, rlen[r0:r1 + 1], 40), 40)
    ctx.coverage_out(True)
    return ctx


def _fetch(ctx):
    mask, cmask, flags = ctx.get_masks()
    off, pos, typ, ish = ctx.get_annotations()
    nb, cov = ctx.get_coverage()
    return dict(min_cov=ctx.get_min_cov(), mask=mask, cmask=cmask, flags=flags, off=off, pos=pos, typ=typ, ish=ish, nb=nb, cov=cov, counters=tuple(ctx.counters()))


def _assert_same(got, want, what=""):
    assert got["min_cov"] == want["min_cov"], what
    for k in TABLES:
        assert np.array_equal(got[k], want[k]), "%s %s" % (k, what)
    assert got["counters"] == want["counters"], what


def _run(rlen, part, P, route, general=0):
    """One part through one pass + the hinge calls.  "exact": the exact-first pass; ("spec", band, bias): the one-sweep pass under a
    biased prediction; ("plain", MIN_COV): hinge_filter_mask_annotate with MIN_COV given (no median: parts without a long read)."""
    ctx = _make(rlen, part, P, sums=route == "exact")
    ctx.force_general_mask(general)
    if route == "exact":
        ctx.filter_sweep(P, fetch=True)
        assert general or ctx.spec_stats()[0] == 0, "must have been the exact-first pass"
    elif route[0] == "spec":
        ctx.debug_spec(band=route[1], sample=4096, bias=route[2])
        ctx.filter_sweep(P, fetch=True)
        assert ctx.spec_stats()[0] >= 1, "must have been the one-sweep pass"
    else:
        ctx.set_min_cov(route[1])
        ctx.filter_mask_annotate(P)
    ctx.filter_hinges(P)
    out = _fetch(ctx)
    out["handed_back"] = ctx.fallback_reads()
    if route != "exact" and route[0] == "spec":
        out["guard"] = ctx.spec_stats()[3]
    ctx.close()
    return out


def _both(monkeypatch, rlen, part, P, route, **env):
    _env(monkeypatch, **env)
    want = _run(rlen, part, P, route, general=1)
    got = _run(rlen, part, P, route)
    _assert_same(got, want, "the fast kernel against the general one, %s" % (route,))
    return got


@pytest.mark.parametrize("name", ["tiny", "edges", "long_reads", "chimera"])
def test_data_sets_table_by_table_and_the_oracles_files(datasets, oracle_lib, tmp_path, monkeypatch, name):
    from hinge_amd import capi, stages
    from hinge_amd.config import default_filter_params
    rlen, pile, r0, r1 = _pile_of(datasets, name)
    P = default_filter_params()
    part = _cut(pile, [r0, r1 + 1])[0]
    guard = 0
    for route in ROUTES:
        out = _both(monkeypatch, rlen, part, P, route)
        guard += max(out.get("guard", 0), 0)
    if name == "chimera":
        assert guard > 0, "needs reads that leave through the guard-band list"
        assert len(out["pos"]) > 0 and int(np.sum(out["ish"])) > 0
    if name == "long_reads":
        assert out["handed_back"] > 0, "needs reads the fast kernel hands back"

    # `hinge filter`'s files against the CPU oracle's
    class IngestContext(capi.Context):   # (behind the bins stages.run_filter hands over, the sums an ingest hands over with them)
        def set_reads(self, rlen, qv_mask=None):
            self._rlen = np.asarray(rlen)
            return super().set_reads(rlen, qv_mask)

        def set_pileups_packed(self, r_begin, r_end, row_ptr, a_span, *args, **kwargs):
            self._pile = (int(r_begin), int(r_end), row_ptr, a_span)
            return super().set_pileups_packed(r_begin, r_end, row_ptr, a_span, *args, **kwargs)

        def set_pile_bins(self, nbins, reso=40, on_device=False):
            super().set_pile_bins(nbins, reso, on_device)
            p0, p1, row_ptr, a_span = self._pile
            self.set_pile_cov(capi.pile_cov(row_ptr[p0:p1 + 2], a_span, self._rlen[p0:p1 + 1], reso), reso)

    src, _ = datasets(name)
    dirs = {}
    for side in ("oracle", "hip"):
        dirs[side] = clone_dataset(src, str(tmp_path / side))
        write_ini(os.path.join(dirs[side], "nominal.ini"))
    assert run_in(dirs["oracle"], oracle_lib.oracle_filter, b"G", b"G.las", 0, b"G", b"nominal.ini", b"") == 0
    _env(monkeypatch)
    ctx = IngestContext(0)
    assert run_in(dirs["hip"], stages.run_filter, "G", "G.las", "G", "nominal.ini", False, 0, True, False, ctx, True) == 0
    ctx.close()
    bad = [s for s in FILTER_FILES if not filecmp.cmp(os.path.join(dirs["oracle"], "G" + s), os.path.join(dirs["hip"], "G" + s), shallow=False)]
    assert not bad, "differs from the oracle: %s" % bad


# ---- synthetic parts: short reads with small pile-ups, long reads with deep ones, and their strict alternation (the deal's order
# mixes the neighbours anyway): every combination of neighbours in a wavefront's sequence of draws ------------------------------------

def _synth(seed, rlen, counts):
    """Pile-ups of len(rlen) reads with counts[i] overlaps each: prefix, suffix and inner spans, B reads at random, rows sorted by B."""
    rng = np.random.default_rng(seed)
    rlen = np.asarray(rlen, np.int32)
    n = len(rlen)
    a = np.repeat(np.arange(n), counts)
    m = len(a)
    b = (a + 1 + rng.integers(0, n - 1, m)) % n
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    rl = rlen[a].astype(np.int64)
    x, y = (rng.random(m) * rl).astype(np.int64), (rng.random(m) * rl).astype(np.int64)
    kind = rng.integers(0, 3, m)
    ab = np.where(kind == 0, 0, np.minimum(x, y))
    ae = np.where(kind == 1, rl, np.maximum(x, y))
    ae = np.maximum(ae, np.minimum(ab + 1, rl))
    bl = rlen[b].astype(np.int64)
    ln = np.minimum(ae - ab, bl)
    bb = ((bl - ln) * rng.random(m)).astype(np.int64)
    comp = rng.integers(0, 2, m).astype(np.uint32)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    a_span = np.ascontiguousarray(np.stack([ab, ae], axis=1).astype(np.int32))
    b_span = np.ascontiguousarray(np.stack([bb, bb + ln], axis=1).astype(np.int32))
    b_flag = np.ascontiguousarray(b.astype(np.uint32) | (comp << np.uint32(31)))
    return rlen, (0, n - 1, row_ptr, a_span, b_span, b_flag)


def _short(rng, n):
    return rng.integers(400, 4001, n), rng.integers(0, 201, n)


def _long(rng, n):
    return rng.integers(15000, 19001, n), rng.integers(256, 400, n)


@pytest.mark.parametrize("kind", ["short", "long", "alternating"])
def test_synthetic_parts(monkeypatch, kind):
    from hinge_amd.config import default_filter_params
    rng = np.random.default_rng(7)
    n = 320
    if kind == "short":
        rl, cnt = _short(rng, n)
    elif kind == "long":
        rl, cnt = _long(rng, n)
    else:
        (rs, cs), (rL, cL) = _short(rng, n), _long(rng, n)
        odd = np.arange(n) % 2 == 1
        rl, cnt = np.where(odd, rL, rs), np.where(odd, cL, cs)
    rlen, part = _synth(11, rl, cnt)
    P = default_filter_params()
    routes = [("plain", 12)]                      # (no read of 5 kb: the median is undefined, MIN_COV is given)
    if kind != "short":
        routes += ROUTES
    for route in routes:
        out = _both(monkeypatch, rlen, part, P, route)
        assert np.any(out["mask"][:, 1] > out["mask"][:, 0]) and int(out["nb"].sum()) > 0


ROW_LENGTHS = [0, 1, 63, 64, 65, 511, 512, 513, 1025]


@pytest.mark.parametrize("last", [65, 1, 512])
def test_row_lengths_the_last_row_and_rows_behind_a_handed_back_read(monkeypatch, last):
    """Rows of 0 .. 1025 overlaps and one of 4 000 on reads of every length; the part's last row ends in a partial batch (65, 1: the
    loads run into the span copy's padding) or a full one.  Six reads, the last but one among them, have 65 536 overlaps: the fast
    kernel hands them back at the top.  Without those six the part is eligible for the exact-first pass."""
    from hinge_amd.config import default_filter_params
    rng = np.random.default_rng(3)
    n = 271
    cnt = np.array([ROW_LENGTHS[i % len(ROW_LENGTHS)] for i in range(n)])
    rl = rng.integers(300, 19001, n)
    cnt[100], rl[100] = 4000, 2000
    cnt[n - 1] = last
    P = default_filter_params()
    rlen, part = _synth(5, rl, cnt)
    _both(monkeypatch, rlen, part, P, "exact")
    heavy = [20, 21, 90, 160, 230, n - 2]
    cnt[heavy] = 65536
    rlen, part = _synth(5, rl, cnt)
    for route in [("plain", 12), ("spec", 1, 1)]:
        out = _both(monkeypatch, rlen, part, P, route)
        assert out["handed_back"] == len(heavy)


@pytest.mark.parametrize("steal", ["0", "1", "2"])
def test_ragged_batched_launch_is_the_per_part_result(datasets, monkeypatch, steal):
    """hinge_filter_sweep_batch_async over parts of n/2, n/3, n/6 - 1 and one read in every HINGE_K2_STEAL mode (a wavefront that
    moves on to the next part reads that part's tables), twice (the second time on the advanced item counters), against every
    part's own sweep through the general kernel."""
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    rlen, pile, r0, r1 = _pile_of(datasets, "chimera")
    n = len(rlen)
    parts = _cut(pile, [0, n // 2, n // 2 + n // 3, n - 1, n])
    P = default_filter_params()
    _env(monkeypatch, wgs=64, HINGE_K2_BATCH="0")
    want = []
    for part in parts:
        ctx = _make(rlen, part, P, sums=True)
        ctx.force_general_mask(1)
        ctx.filter_sweep(P)
        ctx.filter_hinges(P)
        want.append(_fetch(ctx))
        ctx.close()
    _env(monkeypatch, wgs=64, HINGE_K2_BATCH="1", HINGE_K2_STEAL=steal)   # (64: the batched launch's buffers are sized for no fewer)
    ctxs = [_make(rlen, part, P, sums=True) for part in parts]
    ctxs[0].profile_enable(64)
    for _ in range(2):
        for c in ctxs:
            c.set_min_cov(P.min_cov)
        capi.sweep_batch_async(ctxs, P)
        capi.finish_batch_async(ctxs, P)
        capi.hinges_batch_async(ctxs, P)
        for c, w in zip(ctxs, want):
            c.check()
            _assert_same(_fetch(c), w, "HINGE_K2_STEAL=%s" % steal)
    assert ctxs[0].profile_report()["k_mask_annotate"][1] == 2, "one batched K2 launch per step"
    assert sum(len(w["pos"]) for w in want) > 0
    for c in ctxs:
        c.close()
