"""`hinge_draft_ladders` beyond the first kernels' envelope: ladders of 65 .. 65535 members (k_draft_cns_deep) and members of
32768+ bases or member + template beyond the aligner's LDS (k_draft_align_long), against the REFERENCE's own falcon
(ref_falcon_ladder, live from oracle/_ref) and the oracle's restatement, byte for byte; one call that mixes every route; the
member-count limit of the reference's 16-bit vote counters.  Generators: tests/draft_deep_common.py."""
import os

import numpy as np
import pytest

import draft_common as dc
import draft_deep_common as ddc
from test_draft_gpu import _db_of_members

pytestmark = pytest.mark.gpu


def _check(lib, ref, cases, got):
    for k, (mem, mx) in enumerate(cases):
        n, want = dc.ladder_call(ref.ref_falcon_ladder, mem, mx)
        assert n >= 0
        assert got[k] == want, (k, len(mem), max(len(m) for m in mem))
        assert dc.ladder_call(lib.oracle_falcon_ladder, mem, mx) == (n, want)


def test_deep_ladders_match_the_reference(oracle_lib, ref_lib, tmp_path):
    """65, 96, 128, 129, 200, 500, 1000 and 4096 members at 0-20 % errors: members that end early, an unrelated member,
    identical members, a shared 40-100-base insertion; links that first appear in member 64+ and tie with one of chunk 0."""
    from hinge_amd import capi
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    cases = ddc.deep_cases(np.random.default_rng(11))
    db, rungs = _db_of_members(str(tmp_path), [m for m, _ in cases])
    ctx = capi.Context(0)
    got = capi.Draft(ctx, db).ladders(rungs, [mx for _, mx in cases])
    ctx.close()
    _check(lib, ref, cases, got)


def test_long_members_match_the_reference(oracle_lib, ref_lib, tmp_path):
    """Members of 32 767, 32 768, 40 000 and 70 000 bases and a ladder whose member + template exceed the old ~61 000-base LDS
    bound; every other member is stored reverse-complemented (strand 1)."""
    from hinge_amd import capi
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    rng = np.random.default_rng(11)
    ddc.deep_cases(rng)
    cases = ddc.long_cases(rng)
    db, rungs = _db_of_members(str(tmp_path), [m for m, _ in cases])
    assert {r[1] for ld in rungs for r in ld} == {0, 1}
    ctx = capi.Context(0)
    got = capi.Draft(ctx, db).ladders(rungs, [mx for _, mx in cases])
    ctx.close()
    _check(lib, ref, cases, got)


def test_what_the_first_kernels_refused(oracle_lib, ref_lib, tmp_path):
    """A 65-member ladder and a 40 000-base member each failed the whole call (HINGE_E_CAPACITY / HINGE_E_RANGE); now each is
    answered with the reference's bytes."""
    from hinge_amd import capi
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    rng = np.random.default_rng(21)
    truth = ddc.rand_seq(rng, 40000)
    for cases in ([ddc.deep_ladder(rng, 65, 500, 0.12)], [([truth, dc.noisy(rng, truth, 0.03)], 1)]):
        wd = str(tmp_path / str(len(cases[0][0])))
        os.makedirs(wd)
        db, rungs = _db_of_members(wd, [m for m, _ in cases])
        ctx = capi.Context(0)
        got = capi.Draft(ctx, db).ladders(rungs, [mx for _, mx in cases])
        ctx.close()
        _check(lib, ref, cases, got)


def test_one_call_mixes_every_route(oracle_lib, ref_lib, tmp_path):
    """2 000 ordinary ladders with the deep and long ones in ONE call: every ladder the reference's, the ordinary ones equal to a
    call without the others (no cross-talk between routes), and again with a 1 GiB scratch budget (several batches)."""
    from hinge_amd import capi
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    rng = np.random.default_rng(31)
    ordinary = [dc.random_ladder(rng, case) for case in range(2000)]
    special = [ddc.deep_ladder(rng, n, 300, 0.1, kind) for n, kind in ((70, ""), (150, "early"), (300, "insertion"), (1000, ""))]
    special += [ddc.tie_ladder(4)]
    truth = ddc.rand_seq(rng, 36000)
    special += [([dc.noisy(rng, truth, 0.03) for _ in range(4)], 2)]
    truth = ddc.rand_seq(rng, 34000)
    special += [([dc.noisy(rng, truth, 0.02) for _ in range(70)], 5)]         # deep AND long
    mixed, ord_ids = [], []
    for k, c in enumerate(ordinary):                       # the special ladders spread through the call
        ord_ids.append(len(mixed))
        mixed.append(c)
        if k % 300 == 150 and special:
            mixed.append(special.pop(0))
    mixed += special
    db, rungs = _db_of_members(str(tmp_path), [m for m, _ in mixed])
    ctx = capi.Context(0)
    dr = capi.Draft(ctx, db)
    got = dr.ladders(rungs, [mx for _, mx in mixed])
    alone = dr.ladders([rungs[i] for i in ord_ids], [mixed[i][1] for i in ord_ids])
    old = os.environ.get("HINGE_DRAFT_SCRATCH_GB")
    os.environ["HINGE_DRAFT_SCRATCH_GB"] = "1"
    try:
        got_small = dr.ladders(rungs, [mx for _, mx in mixed])
    finally:
        if old is None:
            del os.environ["HINGE_DRAFT_SCRATCH_GB"]
        else:
            os.environ["HINGE_DRAFT_SCRATCH_GB"] = old
    ctx.close()
    assert [got[i] for i in ord_ids] == alone
    assert got_small == got
    _check(lib, ref, mixed, got)


def test_member_count_limit(oracle_lib, ref_lib, tmp_path):
    """1 .. 65535 members (the reference's link_count / count / n_link are uint16_t): a 65 535-member ladder is answered as the
    reference answers it, 65 536 members give HINGE_E_CAPACITY."""
    from hinge_amd import capi
    lib, ref = dc.bind(oracle_lib), dc.bind_ref(ref_lib)
    rng = np.random.default_rng(41)
    truth = ddc.rand_seq(rng, 24)
    mem = [dc.noisy(rng, truth, 0.05) or "a" for _ in range(65535)]
    db, rungs = _db_of_members(str(tmp_path), [mem])
    ctx = capi.Context(0)
    dr = capi.Draft(ctx, db)
    got = dr.ladders(rungs, [7])
    _check(lib, ref, [(mem, 7)], got)
    with pytest.raises(capi.HingeError) as e:
        dr.ladders([rungs[0] + [rungs[0][0]]], [7])
    assert e.value.code == capi.HINGE_E_CAPACITY
    ctx.close()


def test_draft_executable_with_deep_ladders(oracle_lib, tmp_path):
    """`draft_assembly` on a path through every read of a 100x data set (tests/draft_deep_common.deep_chain): FASTA and stdout
    are the oracle's byte for byte, and the oracle's printed lanes show a ladder of more than 64 members (the construction must
    give one: this fails, not skips, when it does not)."""
    lib = dc.bind(oracle_lib)
    wd = str(tmp_path)
    want_fa, want_log, sizes = ddc.deep_chain(lib, wd)
    assert max(sizes) > 64, max(sizes)
    got_fa, got_log = dc.run_product(wd)
    assert got_fa == want_fa, "FASTA differs from the oracle's"
    assert got_log == want_log, "stdout differs from the oracle's"
