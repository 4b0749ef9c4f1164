"""hinge_amd/csrc/stdsort_emul.h (the host/device replay of libstdc++ std::sort the HIP kernels use)
compiled for the host and compared with the real std::sort (through the oracle library)."""
import numpy as np
import pytest

from sort_killer_common import P

import sort_killer_common as skc


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return skc.harness(tmp_path_factory)


def _check(emul, oracle_lib, key):
    key = np.ascontiguousarray(key, np.int32)
    n = len(key)
    for mode_o, desc in ((0, 1), (1, 0)):
        a = np.zeros(max(n, 1), np.int32)
        b = np.zeros(max(n, 1), np.int32)
        oracle_lib.oracle_sort_perm(n, P(key), mode_o, P(a))
        emul.emul_sort_perm(n, P(key), desc, P(b))
        assert np.array_equal(a, b), (n, desc)


def test_replay_matches_std_sort(emul, oracle_lib):
    rng = np.random.default_rng(0)
    for trial in range(1500):
        n = int(rng.choice([0, 1, 2, 3, 15, 16, 17, 18, 31, 33, 64, 100, 257, 1000, 5000, int(rng.integers(1, 3000))]))
        key = [rng.integers(0, 4, size=n), rng.integers(0, max(1, n // 8) + 1, size=n), np.sort(rng.integers(0, 50, size=n)),
               np.sort(rng.integers(0, 50, size=n))[::-1], rng.integers(0, 1 << 20, size=n)][trial % 5]
        _check(emul, oracle_lib, key)


def test_replay_matches_std_sort_in_heapsort_fallback(emul, oracle_lib):
    """Adversarial keys push introsort past its depth limit: the heap part must match too."""
    for n in (200, 1000, 4096, 20000):
        k = np.zeros(n, np.int32)
        emul.killer_keys(n, P(k))
        _check(emul, oracle_lib, k)            # ascending comparator = the adversary's own
        _check(emul, oracle_lib, -k)


@pytest.mark.parametrize("n,q", skc.CASES)
def test_replay_matches_std_sort_in_heapsort_fallback_with_ties(emul, oracle_lib, n, q):
    """Killer keys with ties (key = -(val // q), descending): the case reaches the depth limit where sort_killer_common says it
    does, for q >= 2 the heap part's tie order shows in the result, and hinge_sort::std_sort leaves the order of std::sort."""
    skc.assert_case_reaches_the_fallback(emul, n, q)
    key = skc.killer_key(emul, n, q)
    got = np.zeros(n, np.int32)
    emul.emul_sort_perm(n, P(key), 1, P(got))
    assert np.array_equal(got, skc.oracle_perm(oracle_lib, key)), (n, q)
    wide = key * (1 << 19)                      # what the GPU test feeds the wide form: the same comparisons
    assert wide.dtype == np.int32 and int(wide.max()) - int(wide.min()) >= 1 << 20
    assert np.array_equal(skc.oracle_perm(oracle_lib, wide), got), (n, q, "wide")
