"""GPU parity of the exact-first pass (include/hinge_hip.h, hinge_set_pile_cov): with the ingest's per-read coverage sums the part's
median is known before the sweep, so the pass is k_exact_begin + K2 with the exact MIN_COV - no k_spec_predict, no k_median_hist,
no guard-band launch.  Everything it produces is what the speculative pass produces from the same data (HINGE_INGEST_COV=0) and
what the CPU oracle writes, bit for bit; whatever is not eligible takes the speculative (or the two-sweep) pass as before."""
import filecmp
import os

import numpy as np
import pytest

from conftest import clone_dataset, run_in, write_ini

pytestmark = pytest.mark.gpu

FILTER_FILES = [".mas", ".cmas", ".repeat.txt", ".hinges.txt", ".coverage.txt", ".cov.flag", ".self.flag"]
GONE = ("k_spec_predict", "k_median_hist", "k_mask_annotate_final")     # (the profile name of k_mask_final_batch is k_mask_annotate_final)


def _ingest_context(device=0):
    """A context that receives, behind the bins stages.run_filter hands over, the sums an ingest would hand over with them."""
    from hinge_amd import capi

    class IngestContext(capi.Context):
        def set_reads(self, rlen, qv_mask=None):
            self._rlen = np.asarray(rlen)
            return super().set_reads(rlen, qv_mask)

        def set_pileups_packed(self, r_begin, r_end, row_ptr, a_span, *args, **kwargs):
            self._pile = (int(r_begin), int(r_end), row_ptr, a_span)
            return super().set_pileups_packed(r_begin, r_end, row_ptr, a_span, *args, **kwargs)

        def set_pile_bins(self, nbins, reso=40, on_device=False):
            super().set_pile_bins(nbins, reso, on_device)
            r0, r1, row_ptr, a_span = self._pile
            self.set_pile_cov(capi.pile_cov(row_ptr[r0:r1 + 2], a_span, self._rlen[r0:r1 + 1], reso), reso)

    return IngestContext(device)


def _hip_filter(wd, mlas, ctx, ini="nominal.ini"):
    from hinge_amd import stages
    return run_in(wd, stages.run_filter, "G", "G" if mlas else "G.las", "G", ini, mlas, 0, True, False, ctx, True)


def _same_files(wd_a, wd_b, what):
    bad = [s for s in FILTER_FILES if not filecmp.cmp(os.path.join(wd_a, "G" + s), os.path.join(wd_b, "G" + s), shallow=False)]
    assert not bad, "differs from %s: %s" % (what, bad)


@pytest.mark.parametrize("name,mlas,ini", [("tiny", False, ""), ("tiny_mlas", True, ""), ("long_reads", False, ""), ("edges", False, ""),
                                           ("chimera", False, "ec = 90"), ("chimera", False, "min_cov = 25")])
def test_stage_files_are_the_oracles_and_the_speculative_passes(datasets, oracle_lib, tmp_path, monkeypatch, name, mlas, ini):
    """`hinge filter`'s files through the exact-first pass: the CPU oracle's and, with HINGE_INGEST_COV=0, the speculative pass's.
    tiny_mlas: three parts through one context, MIN_COV carried over as the running maximum; est_cov: the override (filter.cpp:671);
    min_cov = 25: above cov_est / 3 of that data set, the configured value stays."""
    src, _ = datasets(name)
    dirs = {}
    for side in ("oracle", "exact", "spec"):
        dirs[side] = clone_dataset(src, str(tmp_path / side))
        write_ini(os.path.join(dirs[side], "nominal.ini"), extra_filter=ini)
    las = b"G" if mlas else b"G.las"
    assert run_in(dirs["oracle"], oracle_lib.oracle_filter, b"G", las, 1 if mlas else 0, b"G", b"nominal.ini", b"") == 0
    ctx = _ingest_context()
    ctx.profile_enable(64)
    assert _hip_filter(dirs["exact"], mlas, ctx) == 0
    verified, off, outside, guard, pred, exact = ctx.spec_stats()
    assert (verified, off, outside, guard) == (0, 0, 0, 0) and pred == exact, "the pass must have been exact-first"
    rep = ctx.profile_report()
    assert rep["k_exact_begin"][1] >= 1 and all(rep[k][1] == 0 for k in GONE), rep
    min_cov = ctx.get_min_cov()
    if name == "long_reads":
        assert ctx.fallback_reads() > 0, "needs reads the fast kernel hands back (with the exact MIN_COV)"
    ctx.close()
    _same_files(dirs["oracle"], dirs["exact"], "the oracle")
    monkeypatch.setenv("HINGE_INGEST_COV", "0")
    ctx = _ingest_context()
    assert _hip_filter(dirs["spec"], mlas, ctx) == 0
    assert ctx.spec_stats()[0] >= 1, "HINGE_INGEST_COV=0 must keep the speculative pass"
    assert ctx.get_min_cov() == min_cov
    ctx.close()
    _same_files(dirs["spec"], dirs["exact"], "the speculative pass")
    if ini.startswith("min_cov"):
        assert min_cov == 25
    if ini.startswith("ec"):
        assert min_cov == 30


def _pile_of(datasets, name):
    from hinge_amd import formats
    src, _ = datasets(name)
    rlen = formats.read_db_index(os.path.join(src, "G"))["rlen"]
    recs = formats.read_las(os.path.join(src, "G.las"))
    pile = formats.pileups_from_las(recs, rlen)
    return rlen, pile, int(recs.rec["aread"][0]), int(recs.rec["aread"][-1])


def _cut(pile, n, cuts):
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s, e = int(pile.row_ptr[a]), int(pile.row_ptr[b])
        rp = np.ascontiguousarray(np.clip(pile.row_ptr, s, e) - s)       # (n_reads + 1 entries: empty rows outside the part)
        parts.append((a, b - 1, rp, pile.a_span[s:e].copy(), pile.b_span[s:e].copy(), pile.b_flag[s:e].copy()))
    return parts


def _make(rlen, part, P, sums=True, mean=None):
    """A context as an ingest sets it up: packed spans, facts, bins and (sums=True) the coverage sums."""
    from hinge_amd import capi
    r0, r1, rp, a, b, f = part
    ctx = capi.Context(0)
    ctx.set_reads(rlen, None)
    ctx.set_min_cov(P.min_cov)
    span16, max_pile, in_range = capi.pack_spans(rp, a, rlen)
    ctx.set_pileups_packed(r0, r1, rp, a, b, f, span16, max_pile, in_range)
    ctx.set_pile_bins(capi.pile_bins(rp[r0:r1 + 2], a, rlen[r0:r1 + 1], 40), 40)
    if sums:
        ctx.set_pile_cov(capi.pile_cov(rp[r0:r1 + 2], a, rlen[r0:r1 + 1], 40), 40)
    if mean is not None:
        ctx.attach_mean_cov(mean)
    ctx.coverage_out(True)
    return ctx


def _fetch(ctx):
    mask, cmask, flags = ctx.get_masks()
    off, pos, typ, ish = ctx.get_annotations()
    nb, cov = ctx.get_coverage()
    return dict(min_cov=ctx.get_min_cov(), mask=mask, cmask=cmask, flags=flags, off=off, pos=pos, typ=typ, ish=ish, nb=nb, cov=cov, counters=tuple(ctx.counters()))


def _assert_same(got, want):
    assert got["min_cov"] == want["min_cov"] and got["counters"] == want["counters"]
    for k in ("mask", "cmask", "flags", "off", "pos", "typ", "ish", "nb", "cov"):
        assert np.array_equal(got[k], want[k]), k
    if "est" in want:
        assert got["est"] == want["est"]
    if "mean" in want:
        assert np.array_equal(got["mean"], want["mean"])


def _sweep_one(rlen, part, P, sums, knob=None):
    """One part through hinge_filter_sweep + hinges, the means in an attached table: everything the pass leaves behind."""
    import torch
    mean = torch.full((len(rlen),), -2 ** 31, dtype=torch.int32, device="cuda:0")
    ctx = _make(rlen, part, P, sums=sums, mean=mean)
    if knob is not None:
        knob(ctx)
    ctx.profile_enable(32)
    est = ctx.filter_sweep(P, fetch=True)
    ctx.filter_hinges(P)
    out = _fetch(ctx)
    out["est"] = (est.cov_est, est.n_long, est.total_cov, est.num_slot)
    out["mean"] = mean.cpu().numpy()
    out["spec"] = ctx.spec_stats()
    out["launches"] = {k: v[1] for k, v in ctx.profile_report().items() if v[1]}
    ctx.close()
    return out


def _is_exact_first(out):
    return out["spec"][:4] == (0, 0, 0, 0) and out["spec"][4] == out["spec"][5] and out["launches"].get("k_exact_begin", 0) >= 1 and not any(k in out["launches"] for k in GONE)


def _is_speculative(out):
    return out["spec"][0] >= 1 and "k_exact_begin" not in out["launches"] and out["launches"].get("k_spec_predict", 0) >= 1 and out["launches"].get("k_median_hist", 0) >= 1


@pytest.mark.parametrize("name", ["chimera", "long_reads"])
def test_one_part_table_by_table(datasets, monkeypatch, name):
    """hinge_filter_sweep with the sums against the same call under HINGE_INGEST_COV=0: estimate, n_long, totals, MIN_COV, the means
    (attached table), masks, bins, annotations, hinges, work-list size - and which kernels ran."""
    from hinge_amd.config import default_filter_params
    rlen, pile, r0, r1 = _pile_of(datasets, name)
    P = default_filter_params()
    part = _cut(pile, len(rlen), [r0, r1 + 1])[0]
    got = _sweep_one(rlen, part, P, True)
    assert _is_exact_first(got), (got["spec"], got["launches"])
    monkeypatch.setenv("HINGE_INGEST_COV", "0")
    want = _sweep_one(rlen, part, P, True)
    assert _is_speculative(want), (want["spec"], want["launches"])
    _assert_same(got, want)
    assert len(got["pos"]) > 0 and int(np.sum(got["ish"])) > 0 and got["est"][1] > 0


def test_what_is_not_eligible_keeps_its_pass(datasets, monkeypatch):
    """One out-of-range coordinate (nbins = -1 for that read), hinge_debug_spec called, no sums, delete_telomere: today's passes,
    with today's results."""
    from hinge_amd.config import default_filter_params
    rlen, pile, r0, r1 = _pile_of(datasets, "chimera")
    P = default_filter_params()
    part = _cut(pile, len(rlen), [r0, r1 + 1])[0]
    monkeypatch.setenv("HINGE_INGEST_COV", "0")
    want = _sweep_one(rlen, part, P, True)
    monkeypatch.delenv("HINGE_INGEST_COV")
    # hinge_debug_spec called / no sums handed over: the speculative pass
    for sums, knob in ((True, lambda c: c.debug_spec(band=1)), (False, None)):
        got = _sweep_one(rlen, part, P, sums, knob)
        assert _is_speculative(got), (got["spec"], got["launches"])
        _assert_same(got, want)
    # one coordinate behind the end of its read
    r0_, r1_, rp, a, b, f = part
    i = next(i for i in range(r0_, r1_ + 1) if rp[i + 1] - rp[i] > 3 and rlen[i] >= 5000)
    a2 = a.copy().reshape(-1, 2)
    a2[rp[i] + 1, 1] = rlen[i] + 7
    bad = (r0_, r1_, rp, a2.reshape(a.shape), b, f)
    got = _sweep_one(rlen, bad, P, True)
    assert _is_speculative(got), (got["spec"], got["launches"])
    monkeypatch.setenv("HINGE_INGEST_COV", "0")
    _assert_same(got, _sweep_one(rlen, bad, P, True))
    monkeypatch.delenv("HINGE_INGEST_COV")
    # delete_telomere: still two sweeps (k_cov_stats first), sums or not
    import copy
    PT = copy.copy(P)
    PT.delete_telomere = 1
    got = _sweep_one(rlen, part, PT, True)
    assert got["spec"][3] == -1 and got["launches"].get("k_cov_stats", 0) >= 1 and "k_exact_begin" not in got["launches"]
    monkeypatch.setenv("HINGE_INGEST_COV", "0")
    _assert_same(got, _sweep_one(rlen, part, PT, True))


def test_part_without_a_long_read_is_undefined_as_before(datasets):
    """No read of 5 000 bp or more (every length and coordinate of the data set cut to 4 999): ST_NO_LONG_READ from the
    exact-first pass too, the same error."""
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    rlen, pile, r0, r1 = _pile_of(datasets, "chimera")
    P = default_filter_params()
    rl = np.minimum(rlen, 4999).astype(rlen.dtype)
    p0 = _cut(pile, len(rlen), [r0, r0 + 40])[0]
    part = (p0[0], p0[1], p0[2], np.minimum(p0[3], 4999), p0[4], p0[5])
    errs = []
    for sums in (True, False):
        ctx = _make(rl, part, P, sums=sums)
        with pytest.raises(capi.HingeError) as ex:
            ctx.filter_sweep(P, fetch=True)
        errs.append((ex.value.code, str(ex.value)))
        assert ctx.spec_stats()[0] == (0 if sums else 1)          # exact-first / the speculative pass
        ctx.close()
    assert errs[0] == errs[1] and errs[0][0] == -4


def test_batch_of_ragged_parts_and_the_running_maximum(datasets, monkeypatch):
    """hinge_filter_sweep_batch_async / finish / hinges over ragged parts (n/2, n/3, the rest, one read) with the sums, against the
    same calls under HINGE_INGEST_COV=0, twice (the second pass on a current mean table); one k_exact_begin launch per step and none
    of the three launches it replaces.  Then two parts through ONE context in sequence, the second with the smaller median: MIN_COV
    stays the running maximum."""
    import torch
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    rlen, pile, r0, r1 = _pile_of(datasets, "chimera")
    n = len(rlen)
    parts = _cut(pile, n, [0, n // 2, n // 2 + n // 3, n - 1, n])
    P = default_filter_params()

    def run(steps=2):
        mean = torch.full((n,), -2 ** 31, dtype=torch.int32, device="cuda:0")
        ctxs = [_make(rlen, part, P, mean=mean) for part in parts]
        ctxs[0].profile_enable(64)
        outs = []
        for _ in range(steps):
            for c in ctxs:
                c.set_min_cov(P.min_cov)
            capi.sweep_batch_async(ctxs, P)
            capi.finish_batch_async(ctxs, P)
            capi.hinges_batch_async(ctxs, P)
            step = []
            for c in ctxs:
                c.check()
                o = _fetch(c)
                o["mean"] = mean.cpu().numpy()
                step.append(o)
            outs.append(step)
        launches = {k: v[1] for k, v in ctxs[0].profile_report().items() if v[1]}
        spec = [c.spec_stats() for c in ctxs]
        for c in ctxs:
            c.close()
        return outs, launches, spec

    got, launches, spec = run()
    assert launches.get("k_exact_begin") == 2 and not any(k in launches for k in GONE), launches
    assert launches.get("k_mask_annotate") == 2, "one batched K2 launch per step: %s" % launches
    assert all(s[:4] == (0, 0, 0, 0) and s[4] == s[5] for s in spec), spec
    monkeypatch.setenv("HINGE_INGEST_COV", "0")
    want, launches0, spec0 = run()
    monkeypatch.delenv("HINGE_INGEST_COV")
    assert all(k in launches0 for k in GONE[:2]) and "k_exact_begin" not in launches0 and all(s[0] == 2 for s in spec0)
    for step_g, step_w in zip(got, want):
        for g, w in zip(step_g, step_w):
            _assert_same(g, w)
    assert sum(len(w["pos"]) for w in want[0]) > 0

    # two parts through one context: the whole data set, then every second overlap of its first half (about half the coverage)
    whole = _cut(pile, n, [0, n])[0]
    h0, h1, rp, a, b, f = _cut(pile, n, [0, n // 2])[0]
    keep = np.zeros(len(f), bool)
    keep[::2] = True
    rp2 = np.concatenate([[0], np.cumsum(keep)])[rp]
    a2, b2 = a.reshape(-1, 2)[keep].reshape(-1), b.reshape(-1, 2)[keep].reshape(-1)
    thin = (h0, h1, np.ascontiguousarray(rp2), np.ascontiguousarray(a2.reshape((-1,) + a.shape[1:])), np.ascontiguousarray(b2.reshape((-1,) + b.shape[1:])), f[keep].copy())
    res = {}
    for env in ("1", "0"):
        monkeypatch.setenv("HINGE_INGEST_COV", env)
        ctx = capi.Context(0)
        ctx.set_reads(rlen, None)
        ctx.set_min_cov(P.min_cov)
        seq = []
        for part in (whole, thin):
            pr0, pr1, prp, pa, pb, pf = part
            span16, max_pile, in_range = capi.pack_spans(prp, pa, rlen)
            ctx.set_pileups_packed(pr0, pr1, prp, pa, pb, pf, span16, max_pile, in_range)
            ctx.set_pile_bins(capi.pile_bins(prp[pr0:pr1 + 2], pa, rlen[pr0:pr1 + 1], 40), 40)
            ctx.set_pile_cov(capi.pile_cov(prp[pr0:pr1 + 2], pa, rlen[pr0:pr1 + 1], 40), 40)
            ctx.coverage_out(True)
            est = ctx.filter_sweep(P, fetch=True)
            ctx.filter_hinges(P)
            o = _fetch(ctx)
            o["est"] = (est.cov_est, est.n_long, est.total_cov, est.num_slot)
            o["verified"] = ctx.spec_stats()[0]
            seq.append(o)
        ctx.close()
        res[env] = seq
    assert [o["verified"] for o in res["1"]] == [0, 0] and [o["verified"] for o in res["0"]] == [1, 2]
    first, second = res["1"]
    assert second["est"][0] < first["est"][0] and second["est"][0] // 3 < first["min_cov"], "the second part must have the smaller median"
    assert second["min_cov"] == first["min_cov"] == max(P.min_cov, first["est"][0] // 3)
    for g, w in zip(res["1"], res["0"]):
        _assert_same(g, w)
