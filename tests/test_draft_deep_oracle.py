"""Ladders beyond the first draft kernels' envelope on the CPU: oracle/draft_oracle.cpp's restatement of falcon against the
REFERENCE's own falcon code (ref_falcon_ladder) on deep ladders (65 .. 4096 members) and long members (32 767 .. 70 000 bases, and
member + template beyond the old ~61 000-base LDS bound), the generators of tests/draft_deep_common.py - the pin on which the GPU
tests' comparisons with the oracle rest.  No generated ladder may be reference-undefined: the restatement returns >= 0 for all."""
import numpy as np

import draft_common as dc
import draft_deep_common as ddc


def test_deep_and_long_generators_are_reference_defined(oracle_lib):
    lib = dc.bind(oracle_lib)
    rng = np.random.default_rng(11)
    ddc.check_defined(lib, ddc.deep_cases(rng))
    ddc.check_defined(lib, ddc.long_cases(rng))


def test_deep_ladders_restatement_matches_the_reference(oracle_lib, ref_lib):
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    rng = np.random.default_rng(11)
    cases = ddc.deep_cases(rng)
    assert sorted({len(m) for m, _ in cases}) == sorted(set(ddc.DEEP_SIZES) | {136})
    for k, (mem, mx) in enumerate(cases):
        got, want = dc.ladder_call(lib.oracle_falcon_ladder, mem, mx), dc.ladder_call(ref.ref_falcon_ladder, mem, mx)
        assert got[0] >= 0 and got == want, (k, len(mem))


def test_tie_ladder_is_decided_by_the_link_order(oracle_lib, ref_lib):
    """The tie construction does what it claims: trading X's and Y's sequences (same template, same counts) changes the
    reference's consensus - the tie is broken by which link is numbered first - and the restatement agrees on both."""
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    for seed in (1, 2):
        a, b = ddc.tie_ladder(seed), ddc.tie_ladder(seed, swap=True)
        assert a[0][56] == b[0][56] and a[0][0] == b[0][64] and a[0][64] == b[0][0]
        ra, rb = dc.ladder_call(ref.ref_falcon_ladder, *a), dc.ladder_call(ref.ref_falcon_ladder, *b)
        assert ra[0] >= 0 and rb[0] >= 0 and ra[1] != rb[1], seed
        assert dc.ladder_call(lib.oracle_falcon_ladder, *a) == ra and dc.ladder_call(lib.oracle_falcon_ladder, *b) == rb


def test_long_members_restatement_matches_the_reference(oracle_lib, ref_lib):
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    rng = np.random.default_rng(11)
    ddc.deep_cases(rng)                                   # (the same stream as the GPU test's)
    cases = ddc.long_cases(rng)
    assert {len(m[0]) for m, _ in cases} >= set(ddc.LONG_SIZES)
    for k, (mem, mx) in enumerate(cases):
        got, want = dc.ladder_call(lib.oracle_falcon_ladder, mem, mx), dc.ladder_call(ref.ref_falcon_ladder, mem, mx)
        assert got[0] >= 0 and got == want, (k, [len(m) for m in mem])


def test_deep_chain_construction_gives_deep_ladders(oracle_lib, tmp_path):
    """The executable-level construction of test_draft_deep_gpu.py holds on the CPU too: the oracle's `hinge draft` runs through
    it and its largest ladder has more than 64 members."""
    fa, log, sizes = ddc.deep_chain(dc.bind(oracle_lib), str(tmp_path))
    assert len(dc.contigs_of(fa)) >= 2 and sizes
    assert max(sizes) > 64, max(sizes)
