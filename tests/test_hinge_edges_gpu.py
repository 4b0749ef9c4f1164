"""Every route of the hinge calling on the hand-built parts of tests/hinge_edges_common.py: k_hinge_count's two counts, the
order-independent evaluation of k_hinge_call_light and of k_hinge_call<CAP>, the replay of std::sort behind them, the serial exact
kernel - each has to leave the tables of the model (tests/spec_model.py with std::sort's order from the oracle library, held to
the oracle program by tests/test_hinge_edges.py), read for read.  A failure names the case read."""
import numpy as np
import pytest

import hinge_edges_common as he

pytestmark = pytest.mark.gpu

ROUTES = {"default": {}, "lean0": {"HINGE_CALL_LEAN": "0"}, "light0": {"HINGE_CALL_LIGHT": "0"}, "mini1": {"HINGE_CALL_MINI": "1"},
          "group0": {"HINGE_CALL_GROUP": "0"}, "waves4": {"HINGE_COUNT_WAVES": "4"}, "int32": {"HINGE_COUNT_INT32": "1"}, "exact1": {}, "exact2": {}}
PO_CAP_SMALL = 2048


@pytest.fixture(scope="module")
def parts(oracle_lib, tmp_path_factory):
    """(part, model result, packed facts) by name: built and modelled once, read by every route."""
    cache = {}

    def get(name):
        if name not in cache:
            part = he.make_part(name, str(tmp_path_factory.mktemp(name)))
            cache[name] = (part, he.model(part, part.fp, oracle_lib, with_facts=not name.startswith("overflow")), he.pack(part))
        return cache[name]

    return get


def _context(part, packed, force_exact=0):
    from hinge_amd import capi
    rlen, row_ptr, a_span, b_span, b_flag = part.cols
    ctx = capi.Context(0)
    if force_exact:
        ctx.force_exact(force_exact)
    ctx.set_reads(rlen, None)
    if packed is not None:
        span16, max_pile, in_range = packed
        assert span16 is not None and in_range
        ctx.set_pileups_packed(part.r0, part.r1, row_ptr, a_span, b_span, b_flag, span16, max_pile, in_range)
    else:
        ctx.set_pileups(part.r0, part.r1, row_ptr, a_span, b_span, b_flag)
    return ctx


def _compare(ctx, part, m, what):
    """MIN_COV, masks, annotations and is_hinge against the model, read for read."""
    assert ctx.get_min_cov() == m["min_cov"], what
    mask, cmask, _ = ctx.get_masks()
    off, pos, typ, ish = ctx.get_annotations()
    name_of = {i: c for c, i in part.read_of.items()}
    assert np.array_equal(mask, m["mask"]), (what, [name_of.get(i, i) for i in np.nonzero((mask != m["mask"]).any(1))[0][:5]])
    assert np.array_equal(cmask, m["cmask"]), what
    for i in range(part.r0, part.r1 + 1):
        sl = range(int(off[i]), int(off[i + 1]))
        annos = [(int(pos[t]), int(typ[t])) for t in sl]
        assert annos == m["annos"][i], (what, name_of.get(i, i), annos, m["annos"][i])
        hinges = [(int(pos[t]), int(typ[t])) for t in sl if ish[t]]
        assert hinges == m["hinges"][i], (what, name_of.get(i, i), "hinges", hinges, "model", m["hinges"][i])


def _open_annotations(part, m):
    """(undecided by the two counts, of them on pile-ups beyond the half-size instance, order_matters, support > SUP)."""
    allf = [(f["n"], a) for f in m["facts"].values() if not f["gated"] for a in f["a"]]
    return (sum(a["undecided"] for n, a in allf), sum(a["undecided"] for n, a in allf if n > PO_CAP_SMALL), sum(a["order_matters"] for n, a in allf),
            sum(a["support"] > part.fp.hinge_min_support for n, a in allf))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", he.PARTS)
def test_every_route_leaves_the_models_tables(parts, monkeypatch, name, route):
    part, m, packed = parts(name)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    force = int(route[-1]) if route.startswith("exact") else 0
    n_open, n_open_big, n_order, n_scanned = _open_annotations(part, m)
    assert n_open >= n_order >= 1
    for call in ("sweep_hinges", "run"):
        for hand in (None, packed):
            what = (name, route, call, "packed" if hand is not None else "plain")
            ctx = _context(part, hand, force)
            if call == "run":
                ctx.filter_run(part.fp)
                ctx.check()
            else:
                ctx.set_min_cov(part.fp.min_cov)
                ctx.filter_sweep(part.fp)
                ctx.filter_hinges(part.fp)
            _compare(ctx, part, m, what)
            half, full = ctx.heavy_items()
            queued = int(ctx.counters()[1])
            ctx.close()
            # non-vacuity, from the model's own supporter lists: what k_hinge_count left open, and to which instance it went
            if force == 0:
                assert (half + full, full) == (n_open, n_open_big), what
            if force == 1:
                assert queued == n_scanned >= n_order, what         # every scanned annotation took the serial exact kernel
            if name == "named" and route == "default":
                assert n_open_big >= 4 and queued >= 1, what          # pile_4097: its pile-up does not fit the replay's LDS


def test_two_parts_in_one_batched_launch_keep_their_own_tables(parts):
    """hinges_batch_async over two resident parts, one handed over packed and one not: the batch runs the int32 form of k_hinge_count
    for both, and each part keeps its own tables."""
    from hinge_amd import capi
    (pa, ma, packed_a), (pb, mb, _) = parts("drawn_shipped_1"), parts("drawn_shipped_2")
    ctxs = [_context(pa, packed_a), _context(pb, None)]
    for c in ctxs:
        c.set_min_cov(pa.fp.min_cov)
    capi.sweep_batch_async(ctxs, pa.fp)
    capi.finish_batch_async(ctxs, pa.fp)
    capi.hinges_batch_async(ctxs, pa.fp)
    for c, part, m in zip(ctxs, (pa, pb), (ma, mb)):
        c.check()
        _compare(c, part, m, ("batch", part.name))
        assert sum(c.heavy_items()) == _open_annotations(part, m)[0]
    assert ma["hinges"] != mb["hinges"]
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("name,route", [("overflow", "exact1"), ("overflow", "default"), ("overflow_queue", "exact1")])
def test_exact_queue_and_arena_overflow_and_rerun(parts, name, route):
    """4200 queued annotations on pile-ups of 205 overlaps: a fresh context's exact queue holds 4096 entries and its arena 2^22 ints,
    so under force_exact(1) the first pass overflows both, hinge_filter_hinges grows them and runs the pass again.  overflow_queue:
    the same reads unpadded overflow the queue alone (the arena's rerun would cover for a queue that is grown but not run again)."""
    part, m, _ = parts(name)
    ctx = _context(part, None, 1 if route == "exact1" else 0)
    ctx.set_min_cov(part.fp.min_cov)
    ctx.filter_sweep(part.fp)
    ctx.filter_hinges(part.fp)
    _compare(ctx, part, m, (name, route))
    queued = int(ctx.counters()[1])
    ctx.close()
    if route == "exact1":
        assert queued > 4096, "a queue of 4096 entries cannot give this without the rerun"
