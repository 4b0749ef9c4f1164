"""`hinge consensus` on the GPU at the edges no other test reaches on purpose: the global-atomics vote (k_cns_vote) on pinned data, a
tile of CNS_TILE_MAX positions and the first trace spacing beyond it, and the 16-bit tile counters at their limit.

The two tspace cases past the tile limit are UNPINNED: they are compared with the oracle restatement (oracle/consensus_oracle.cpp),
not with the reference's program.  From a trace spacing of about 1 700 on the reference can give up with "Out of memory (Enlarging DP
vector)" - it sizes its wave vector in int arithmetic from a value it reads one behind the trace (consensus_common.run_reference) -
and at 2 600 and at 4 096 it did so in 20 runs of 20; the restatement is pinned to it on every smaller set."""
import os

import numpy as np
import pytest

import cns_model
import consensus_common as cc

pytestmark = pytest.mark.gpu

NOISY = dict(p_sub=0.05, p_ins=0.09, p_del=0.05)


def _widest_lane_bytes(las):
    """A lower bound of one k_cns_realign lane's wave storage (consensus_kernels.h cns_cells / cns_row_width with |m - n| = 0)."""
    tb = 1 if las.tspace <= 125 else 2
    tr = las.trace.astype(np.int64) if tb == 1 else np.ascontiguousarray(las.trace).view("<u2").astype(np.int64)
    dcap = int(tr[0::2].max())
    return 4 * (dcap + 3) * (2 * ((dcap + 1) // 2) + 3)


def test_tile_of_the_largest_size_and_a_halved_launch(oracle_lib, tmp_path):
    """tspace 4096 = CNS_TILE_MAX: one tile per 4096 positions, 81 940 B of LDS counters (hipFuncSetAttribute), on the 9000-base contig
    of cns_edge_t2458 with noisy reads - and HINGE_CNS_SCRATCH_GB=1, which two workgroups' wave storage exceeds: k_cns_realign's grid is
    halved and its lanes stride over the segments.  Unpinned (module docstring): against the oracle."""
    from hinge_amd import formats
    wd = str(tmp_path)
    cc.make("cns_edge_t2458", wd, tspace=4096, coverage=80.0, **NOISY)
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    n_seg = int((las.rec["tlen"] // 2).sum())
    assert len(las.rec) < 400 and n_seg > 256 and 2 * 256 * _widest_lane_bytes(las) > (1 << 30) > 256 * _widest_lane_bytes(las) * 1.3
    want = cc.run_oracle(oracle_lib, wd)
    got = cc.run_product(wd, env={"HINGE_CNS_SCRATCH_GB": "1"})
    assert got[0] == want[0] and got[1] == want[1]
    assert any(c.isupper() for c in got[0].decode().split("\n")[1])


def test_trace_spacing_beyond_the_largest_tile(oracle_lib, tmp_path):
    """tspace 4097: cns_tile_len(tspace) > CNS_TILE_MAX, the global-atomics vote by itself.  Unpinned: against the oracle."""
    wd = str(tmp_path)
    cc.make("cns_edge_t2458", wd, tspace=4097)
    want = cc.run_oracle(oracle_lib, wd)
    got = cc.run_product(wd)
    assert got[0] == want[0] and got[1] == want[1]
    assert any(c.isupper() for c in got[0].decode().split("\n")[1])


@pytest.mark.parametrize("name", ["cns_noisy", "cns_twobyte", "cns_edge_t64", "cns_edge_t2048"])
def test_global_vote_on_pinned_data(oracle_lib, tmp_path, name):
    """HINGE_CNS_VOTE_GLOBAL=1: k_cns_vote instead of the LDS tiles.  FASTA and stdout are the reference program's."""
    wd = str(tmp_path)
    cc.make(name, wd)
    fasta, out = cc.run_product(wd, env={"HINGE_CNS_VOTE_GLOBAL": "1"})
    ref = cc.run_reference(wd) or cc.run_oracle(oracle_lib, wd)
    assert fasta == ref[0] and out == ref[1]
    assert cc.sha(fasta) == cc.GOLDEN[name]["fasta_sha256"] and cc.sha(out) == cc.GOLDEN[name]["stdout_sha256"]


@pytest.fixture(scope="module")
def repeated(tmp_path_factory):
    """cns_tiny and one alignment k of it: 600-900 aligned bases, two inserted bases in a row, both the same base, among its voted
    columns (found from cns.indels() and the read).  The contig of k after picks = [k] * N for every N the tests use, and the model's
    count planes of ONE vote of k."""
    from hinge_amd import capi, formats
    wd = str(tmp_path_factory.mktemp("cns_repeat"))
    d = cc.make("cns_tiny", wd)
    ctx = capi.Context(0)
    cns = capi.Consensus(ctx, os.path.join(wd, "draft"), os.path.join(wd, "reads"))
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    cns.run(las, list(range(len(las.rec))))
    found = None
    for k, r in enumerate(las.rec):
        if not 600 <= int(r["aepos"] - r["abpos"]) <= 900:
            continue
        read = d.reads[int(r["bread"])]
        bseq = (3 - read[::-1]) if int(r["flags"]) & 1 else read
        kind, apos, base = cns_model.columns(int(r["abpos"]), int(r["aepos"]), int(r["bbpos"]), cns.indels(k), bseq)
        start, end, _ = cns_model.chop_end(kind)
        if any(kind[c] == 1 and kind[c + 1] == 1 and base[c] == base[c + 1] and apos[c] == apos[c + 1] for c in range(start, end - 1)):
            found = k
            break
    assert found is not None, "no alignment of 600-900 bases with two equal inserted bases in a row"
    k, contig = found, int(las.rec[found]["aread"])
    draft = d.contigs[contig]
    one = np.zeros((9, len(draft)), np.int64)
    cns_model.vote(one, 0, len(draft), kind, apos, base, start, end)
    assert one[5:].max() >= 2
    runs = {}
    for n in (1, 3, 40_000, 65_535, 65_536):
        cns.run(las, [k] * n)
        runs[n] = cns.contig(contig)
    ctx.close()
    return {"runs": runs, "draft": draft, "one": one}


def test_three_votes_give_the_model_s_string(repeated):
    """N = 3 is the expected answer of the larger runs: every rule of consensus.cpp:228-270 is a proportion and depth >= 3 holds.  It is
    itself the model's string (cns_model.call on three times the planes of one vote), the twice-inserted base in it."""
    text, st = repeated["runs"][3]
    want = cns_model.call(3 * repeated["one"], repeated["draft"])
    assert text.decode() == want
    assert st.insertions >= 1 and st.good_bases > 300 and st.consensus_length == sum(c.isupper() for c in want)


@pytest.mark.parametrize("n", [40_000, 65_535, 65_536])
def test_counters_hold_one_alignment_n_times(repeated, n):
    """One alignment N times: the contig string must equal N = 3's and the statistics scale.  65 536 runs on k_cns_vote's int32 counters
    (the host's limit); 65 535 holds the aligned 16-bit counters at 0xffff; at 40 000 the twice-inserted base's counter would pass
    0xffff (80 000 mod 65 536 = 14 464 < depth / 2: the insertion was lost) - k_cns_vote_tiles flags it (CNS_ST_VOTE16) and the
    host votes again with k_cns_vote."""
    text3, st3 = repeated["runs"][3]
    text1, st1 = repeated["runs"][1]
    text, st = repeated["runs"][n]
    assert text == text3
    assert st.sum_coverage == n * st1.sum_coverage and st1.sum_coverage > 300
    assert (st.good_bases, st.insertions, st.deletions, st.low_coverage_bases, st.consensus_length) == \
           (st3.good_bases, st3.insertions, st3.deletions, st3.low_coverage_bases, st3.consensus_length)
