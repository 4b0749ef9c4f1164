"""The numpy model of `hinge seed` (tests/seed_common.py) against what it is for: the recall rule on the generator's data sets, no
placement for unrelated reads, and the order of a repeat's two copies.  No GPU, no library."""
import numpy as np
import pytest

import seed_common as sm
from hinge_amd import synth_consensus as sc


@pytest.mark.parametrize("name", ["cns_tiny", "cns_twobyte", "cns_noisy", "cns_small"])
def test_recall_rule(name):
    """Every generator record of >= 400 aligned contig bases (of a read with several, its longest) gets its contig, its strand and a
    diagonal within window + 5 % of its length, at the defaults.  Only records under 400 bases are left out."""
    d = sc.generate(sc.CONFIGS[name])
    index = sm.Index(d.contigs)
    res = sm.model_seed(d.contigs, d.reads, index=index)
    checked, missed, left_out = sm.recall(d, res, index)
    assert missed == []
    assert checked >= 40 and all(ln < 400 for ln in left_out)
    longest = {}
    for q in d.rec:
        longest[int(q["bread"])] = max(longest.get(int(q["bread"]), 0), int(q["aepos"]) - int(q["abpos"]))
    assert checked + len(left_out) == len(longest) and len(left_out) == sum(v < 400 for v in longest.values())
    assert all(n <= 1 for n in res[3]) and len(res[0]) == sum(res[3]) == len(res[1]) == len(res[2])


def test_unrelated_reads_get_nothing():
    rng = np.random.default_rng(8)
    d = sc.generate(sc.CONFIGS["cns_small"])
    reads = [rng.integers(0, 4, size=1000, dtype=np.uint8) for _ in range(40)]
    pl, count, diag, n_placed, status = sm.model_seed(d.contigs, reads)
    assert pl == [] and n_placed == [0] * 40 and status == [(sm.NONE, sm.NONE)] * 40


def test_repeat_copies_and_their_order():
    contigs, reads = sm.repeat_case()
    one = sm.model_seed(contigs, reads, max_placements=1)
    assert one[3] == [1] and one[0][0][:3] == (0, 0, 0) and one[0][0][3:5] == (1050, 1550) and one[0][0][5:] == (0, 500) and one[2] == [1050]
    two = sm.model_seed(contigs, reads, max_placements=2)
    assert two[3] == [2] and two[0][0] == one[0][0] and two[0][1][3:5] == (4050, 4550) and two[2] == [1050, 4050]
    assert two[1][0] == two[1][1] == (500 - sm.K) // sm.STEP + 1                     # every sampled k-mer, on either copy
    assert sm.model_seed(contigs, reads, max_placements=8)[:4] == two[:4]
    # the complemented read: the same two, as strand 1
    rc = sm.model_seed(contigs, [sm.revcomp(reads[0])], max_placements=2)
    assert [p[2:] for p in rc[0]] == [p[2:3] + p[3:] for p in [(0, 0, 1, 1050, 1550, 0, 500), (0, 0, 1, 4050, 4550, 0, 500)]] and rc[4] == [(sm.NONE, sm.OK)]


def test_stride_and_overflow():
    assert sm.stride(15, 15, 2, 64) == 2 and sm.stride(15 + 127, 15, 2, 64) == 2 and sm.stride(15 + 128, 15, 2, 64) == 4 and sm.stride(20000, 15, 2, 64) == 314
    assert (20000 - 15) // 314 + 1 <= 64 < (20000 - 15) // 312 + 1
    seen = {}
    for label, contigs, reads, kw, host_only in sm.edge_calls():
        seen[label] = sm.model_seed(contigs, reads, **kw)
    assert seen["fill64"][4] == [(sm.OK, sm.NONE)] and seen["over65"][4] == [(sm.OVERFLOW, sm.NONE), (sm.NONE, sm.OVERFLOW)]
    assert seen["max_occ"][3] == [4, 0, 4] and set(seen["max_occ"][1]) == {1}
    assert seen["contig_ends"][3] == [1, 1, 1, 1, 0]
    assert [p[3:] for p in seen["contig_ends"][0]] == [(0, 15, 0, 15), (485, 500, 0, 15), (0, 15, 0, 15), (685, 700, 0, 15)]
    assert [p[:3] + p[3:] for p in seen["overhang"][0]] == [(1, 0, 0, 0, 400, 100, 500), (1, 1, 0, 1600, 2000, 0, 400), (1, 2, 1, 0, 400, 100, 500), (1, 3, 1, 1600, 2000, 0, 400)]
    assert seen["lengths"][3] == [0, 1, 1]
