"""The depth-limit fallback of the device replay of std::sort (hinge_amd/csrc/pileup_order.h): hinge_sort::heapsort_ by one lane,
in the level walk (depth == 0) and in the in-register finish of 17 .. 64 element segments (dep == 0), of the packed form and of
the wide form.  Keys from tests/sort_killer_common.py: they run libstdc++'s introsort out of depth WITH ties, so where the heap
part leaves equal keys decides the comparison.  One workgroup per call."""
import numpy as np
import pytest

import sort_killer_common as skc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def killer(tmp_path_factory):
    return skc.harness(tmp_path_factory)


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference():
    """The reference's own comparators behind std::sort, where oracle/_ref was built (None otherwise: the oracle alone decides)."""
    import oracle
    return oracle.ref_lib()


@pytest.mark.parametrize("form", ["packed", "wide"])
@pytest.mark.parametrize("n,q", skc.CASES)
def test_device_replay_matches_std_sort_in_heapsort_fallback(killer, ctx, oracle_lib, reference, n, q, form):
    skc.assert_case_reaches_the_fallback(killer, n, q)
    key = skc.killer_key(killer, n, q)
    if form == "wide":
        key = key * (1 << 19)          # the same comparisons, a span of 2^20 or more: block_std_sort_desc takes the wide form
        assert key.dtype == np.int32 and int(key.max()) - int(key.min()) >= 1 << 20 and int(key.min()) > -(1 << 31)
    else:
        assert int(key.max()) - int(key.min()) < 1 << 20
    got = skc.perm_of_positions(ctx.debug_pileup_order(key))
    assert np.array_equal(got, skc.oracle_perm(oracle_lib, key)), (n, q, form)
    if reference is not None:
        assert np.array_equal(got, skc.oracle_perm(reference, key, "ref_sort_perm")), (n, q, form, "reference")
