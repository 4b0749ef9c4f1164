"""Every instance of the device replay of std::sort (hinge_amd/csrc/pileup_order.h) that k_hinge_call can run - the work spaces of
4096, 2048 and 1024 elements, each through block_std_sort_desc (a key array; packed or wide form by the keys' span) and through
block_std_sort_desc_keys (the LEAN layout: keys from a functor, staged in the stopper scratch, packed form only) - by way of
hinge_debug_pileup_order_in.  One workgroup per call."""
import numpy as np
import pytest

import sort_killer_common as skc

pytestmark = pytest.mark.gpu

CAPS = [4096, 2048, 1024]
INSTANCES = [(cap, lean) for cap in CAPS for lean in (False, True)]


@pytest.fixture(scope="module")
def killer(tmp_path_factory):
    return skc.harness(tmp_path_factory)


@pytest.fixture(scope="module")
def ctx():
    from hinge_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _check(ctx, oracle_lib, cap, lean, key, what):
    key = np.ascontiguousarray(key, np.int32)
    ok, pos = ctx.debug_pileup_order_in(cap, lean, key)
    assert ok, (cap, lean, what)
    assert np.array_equal(skc.perm_of_positions(pos), skc.oracle_perm(oracle_lib, key)), (cap, lean, what)


@pytest.mark.parametrize("cap,lean", INSTANCES)
def test_instance_matches_std_sort_in_heapsort_fallback(killer, ctx, oracle_lib, cap, lean):
    """The killer cases that fit the instance: as they are (packed form), and for the key-array entry times 2^19 (wide form)."""
    cases = [(n, q) for n, q in skc.CASES if n <= cap]
    assert any(n == cap for n, _ in cases) and any(n <= 65 for n, _ in cases)
    for n, q in cases:
        skc.assert_case_reaches_the_fallback(killer, n, q)
        key = skc.killer_key(killer, n, q)
        _check(ctx, oracle_lib, cap, lean, key, (n, q, "packed"))
        if not lean:
            _check(ctx, oracle_lib, cap, lean, key * (1 << 19), (n, q, "wide"))


def _keys_of_kind(rng, n, kind):
    """The key kinds of test_filter_gpu.py::test_pileup_order_replays_std_sort (6: keys that span 2^20 or more)."""
    if kind == 0:
        return rng.integers(0, 4, size=n)
    if kind == 1:
        return rng.integers(0, max(1, n // 8) + 1, size=n)
    if kind == 2:
        return np.sort(rng.integers(0, 50, size=n))
    if kind == 3:
        return np.sort(rng.integers(0, 50, size=n))[::-1]
    if kind == 4:
        return rng.integers(0, 1 << 20, size=n)
    if kind == 5:
        return np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]])
    if kind == 6:
        return rng.integers(-(1 << 30), 1 << 30, size=n) // (1 if n % 2 else 1 << 12) * (1 if n % 2 else 1 << 12)
    return rng.integers(-70000, -69000 + n // 8, size=n)


@pytest.mark.parametrize("cap,lean", INSTANCES)
def test_instance_replays_std_sort(ctx, oracle_lib, cap, lean):
    rng = np.random.default_rng(5)
    sizes = [n for n in (0, 1, 2, 15, 16, 17, 18, 33, 64, 65, 100, 257, 1000, 2048, 4095, 4096) if n < cap - 1] + [cap - 1, cap]
    sizes += [int(x) for x in rng.integers(17, cap, size=10)]
    for n in sizes:
        for kind in range(8):
            key = np.ascontiguousarray(_keys_of_kind(rng, n, kind), np.int32)
            if lean and n > 0 and int(key.max()) - int(key.min()) >= 1 << 20:
                ok, pos = ctx.debug_pileup_order_in(cap, lean, key)
                assert not ok and (pos == -1).all(), (cap, n, kind)
                continue
            _check(ctx, oracle_lib, cap, lean, key, (n, kind))


@pytest.mark.parametrize("cap,lean", INSTANCES)
def test_instance_at_the_packed_form_s_span_limit(ctx, oracle_lib, cap, lean):
    """Keys spanning exactly 2^20 - 1 sort (the packed form's last span); spanning exactly 2^20 the key-array entry sorts them in
    the wide form, the functor entry reports "not sorted" and leaves the output alone."""
    rng = np.random.default_rng(11)
    for n in (2, 17, 64, 100, cap):
        for base in (0, -(1 << 30), (1 << 31) - (1 << 20) - 1):
            for sp in ((1 << 20) - 1, 1 << 20):
                key = base + rng.integers(0, sp + 1, size=n) // 4096 * 4096      # ties inside the span
                key[int(rng.integers(0, n))] = base
                key[(int(np.argmin(key)) + 1) % n] = base + sp
                key = np.ascontiguousarray(key, np.int32)
                assert int(key.max()) - int(key.min()) == sp
                if lean and sp == 1 << 20:
                    ok, pos = ctx.debug_pileup_order_in(cap, lean, key)
                    assert not ok and (pos == -1).all(), (cap, n, base)
                else:
                    _check(ctx, oracle_lib, cap, lean, key, (n, base, sp))


@pytest.mark.parametrize("cap,lean", INSTANCES)
def test_instance_refuses_more_than_its_capacity(ctx, cap, lean):
    from hinge_amd import capi
    with pytest.raises(capi.HingeError) as ex:
        ctx.debug_pileup_order_in(cap, lean, np.zeros(cap + 1, np.int32))
    assert ex.value.code == capi.HINGE_E_ARG


def test_no_other_instance(ctx):
    from hinge_amd import capi
    with pytest.raises(capi.HingeError) as ex:
        ctx.debug_pileup_order_in(512, False, np.zeros(4, np.int32))
    assert ex.value.code == capi.HINGE_E_ARG
