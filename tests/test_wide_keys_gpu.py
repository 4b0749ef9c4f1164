"""The hand-off for sort keys that span 2^20 or more inside the hinge calling: the LEAN instance of k_hinge_call cannot sort them
(block_std_sort_desc_keys returns false), files the annotation in the exact queue, and the serial exact kernel has to be launched
for it.  The part is hand-made (tests/wide_keys_common.py), the expected tables are the model's (tests/spec_model.py, held to the
figures of tests/test_wide_keys.py); every route that can take the annotation must leave the same tables."""
import numpy as np
import pytest

import wide_keys_common as wk

pytestmark = pytest.mark.gpu

ROUTES = ["default", "lean0", "exact1", "exact2"]


@pytest.fixture(scope="module")
def expected(oracle_lib):
    """(part, model result) by (S, shape): computed once, read by every route."""
    from hinge_amd.config import default_filter_params
    cache = {}

    def get(S, shape):
        if (S, shape) not in cache:
            part = wk.make_part(S, shape)
            cache[(S, shape)] = (part, wk.model(part, default_filter_params(), oracle_lib))
        return cache[(S, shape)]

    return get


@pytest.mark.parametrize("call", ["sweep_hinges", "run"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", wk.SHAPES)
@pytest.mark.parametrize("S", [40, 100])
def test_wide_key_annotation_is_decided_like_the_model(expected, monkeypatch, S, shape, route, call):
    from hinge_amd import capi
    from hinge_amd.config import default_filter_params
    (rlen, row_ptr, a_span, b_span, b_flag), m = expected(S, shape)
    assert wk.span(m["sorts"][1]) >= 1 << 20 and (S <= 64 or wk.span(m["sorts"][0]) >= 1 << 20)
    P = default_filter_params()
    if route == "lean0":
        monkeypatch.setenv("HINGE_CALL_LEAN", "0")
    ctx = capi.Context(0)
    if route.startswith("exact"):
        ctx.force_exact(int(route[-1]))
    ctx.set_reads(rlen, None)
    ctx.set_pileups(0, S, row_ptr, a_span, b_span, b_flag)
    if call == "run":
        ctx.filter_run(P)
        ctx.check()
    else:
        ctx.set_min_cov(P.min_cov)
        ctx.filter_sweep(P)
        ctx.filter_hinges(P)
    assert ctx.long_reads() == 1
    assert ctx.get_min_cov() == m["min_cov"]
    mask, cmask, _ = ctx.get_masks()
    off, pos, typ, ish = ctx.get_annotations()
    queued = int(ctx.counters()[1])
    ctx.close()
    assert np.array_equal(mask, m["mask"]) and np.array_equal(cmask, m["cmask"])
    got_annos = {i: [(int(pos[t]), int(typ[t])) for t in range(int(off[i]), int(off[i + 1]))] for i in range(S + 1)}
    got_hinges = {i: [(int(pos[t]), int(typ[t])) for t in range(int(off[i]), int(off[i + 1])) if ish[t]] for i in range(S + 1)}
    assert got_annos == m["annos"]
    if route == "default":
        assert queued >= 1, "the annotation did not take the hand-off this test is about"
    assert got_hinges == m["hinges"], (route, call, queued)
