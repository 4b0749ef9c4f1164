"""The hand-built parts of tests/hinge_edges_common.py on the CPU: every named case is what its name says (facts from the model's own
supporter lists), the threshold pairs give the two answers stated for them, the drawn parts crowd the thresholds, and the model's
tables are the oracle program's output files on the written parts.  These tables are what tests/test_hinge_edges_gpu.py holds
every route of the hinge kernels to."""
import os

import numpy as np
import pytest

from conftest import run_in

import hinge_edges_common as he


@pytest.fixture(scope="module")
def parts(oracle_lib, tmp_path_factory):
    """(part, model result) by name: built and modelled once."""
    cache = {}

    def get(name):
        if name not in cache:
            part = he.make_part(name, str(tmp_path_factory.mktemp(name)))
            cache[name] = (part, he.model(part, part.fp, oracle_lib, with_facts=not name.startswith("overflow")))
        return cache[name]

    return get


def _check_partners(part, m, min_cov):
    NP = part.n_partners
    assert m["min_cov"] == min_cov
    assert (m["mask"][:NP] == [he.MLO, he.MHI]).all() and (m["mask"][-1] == [he.MLO, he.MHI]).all()
    assert all(not m["annos"][i] for i in list(range(NP)) + [part.r1])


@pytest.mark.parametrize("name", ["named", "tiny"])
def test_every_named_case_is_what_it_is_for(parts, name):
    part, m = parts(name)
    _check_partners(part, m, 9 if name == "named" else 1)
    for cname, f in m["facts"].items():
        exp = part.cases[cname].expect
        assert tuple(m["mask"][part.read_of[cname]]) == (he.MLO, he.MHI), cname
        assert not f["gated"], cname
        assert len(f["annos"]) == exp.get("annos", 1), (cname, f["annos"])
        a0 = f["a"][0]
        for k in ("support", "near_end", "span", "order_matters", "undecided", "len_tie", "hinge", "at"):
            if k in exp:
                assert a0[k] == exp[k], (cname, k, a0[k], exp[k])
        if "n" in exp:
            assert f["n"] == exp["n"], cname
        if "open" in exp:
            assert sum(a["undecided"] for a in f["a"]) == exp["open"], cname
        assert [(p, t) for (p, t), a in zip(f["annos"], f["a"]) if a["hinge"]] == list(m["hinges"][part.read_of[cname]])


def test_threshold_pairs_flip_the_answer(parts):
    """One step across a threshold, two answers - for every variant (type +1, complemented supporters) of every pair."""
    part, m = parts("named")
    hinge = {c: [a["hinge"] for a in f["a"]] for c, f in m["facts"].items()}
    for tag in ("", "_plus", "_comp", "_plus_comp"):
        for none, yes in (("support_7", "support_8"), ("support_6", "support_8"), ("overhang_300", "overhang_301"), ("window_-100", "window_-99"),
                          ("window_+100", "window_+99"), ("window_scan_+100", "window_scan_+99"), ("near_end_6", "near_end_7"), ("seventh_at_200", "seventh_at_199"),
                          ("unbridged_c7_at_200", "unbridged_c7_at_201"), ("unbridged_c6_at_201", "unbridged_c7_at_201"), ("unbridged_c6_at_200", "unbridged_c7_at_201"),
                          ("bridged_7_followers", "bridged_6_followers"), ("bridged_follower_at_199", "bridged_follower_at_200"),
                          ("bridged_own_group_8", "bridged_own_group_7"), ("cat0_followers_7", "cat0_followers_6"),
                          ("cat0_not_considered_6", "cat0_not_considered_7"), ("bmust", "umust"), ("order_first_3", "order_first_2")):
            assert hinge[none + tag] == [False] and hinge[yes + tag] == [True], (none, yes, tag)
    # the tie order decides, and std::sort left both outcomes: among the supporter lists beyond 16 (introsort) and up to 16
    om = [(c, f) for c, f in m["facts"].items() if f["a"][0]["order_matters"] and len(f["a"]) == 1]
    for big in (False, True):
        got = {f["a"][0]["hinge"] for c, f in om if (f["a"][0]["support"] > 16) == big}
        assert got == {False, True}, (big, got)
    assert len(om) >= 3 and all(f["n"] > 16 for c, f in om)       # (pile-ups of at most 16 overlaps: the tiny part)
    # exactly the cases that claim it are order_matters
    for c, f in m["facts"].items():
        if "order_matters" in part.cases[c].expect or len(f["a"]) != 1:
            continue
        assert not f["a"][0]["order_matters"], c
    # the dense list's step up is an annotation of the other type
    for tag in ("", "_plus", "_comp"):
        assert [t for _, t in m["facts"]["light_dense_other_type" + tag]["annos"]] == [1, -1]
    # the light kernel bins what has at most LIGHT_CAP = 1023 supporters: the cases for its 10-bit counts must not exceed it
    for c, f in m["facts"].items():
        if c.startswith(("light_bin_", "light_dense_")):
            assert all(a["support"] <= 1023 for a in f["a"]) and max(a["support"] for a in f["a"]) == 1023, c


def test_tiny_pileups_let_the_las_order_decide(parts):
    part, m = parts("tiny")
    for c, f in m["facts"].items():
        if f["n"] == 16:      # n <= 16 and 14 supporters: both sorts are stable insertion sorts (at n = 17 the pile-up sort is an introsort)
            assert f["a"][0]["hinge"] == ("first_2" in c), c
        elif "_tie" not in c:      # without a length tie the pair's order is its length order whatever the sort
            assert f["a"][0]["hinge"] == ("first_2" in c), c
    assert {f["n"] for f in m["facts"].values()} == {16, 17}


@pytest.mark.parametrize("name", [p for p in he.PARTS if p.startswith("drawn")])
def test_drawn_parts_crowd_the_thresholds(parts, name):
    part, m = parts(name)
    _check_partners(part, m, 9)
    allf = [a for f in m["facts"].values() for a in f["a"]]
    assert not any(f["gated"] for f in m["facts"].values())
    assert len(allf) >= 300
    hinges = sum(a["hinge"] for a in allf)
    assert 5 * hinges >= len(allf) and 5 * (len(allf) - hinges) >= len(allf), (hinges, len(allf))
    assert sum(a["order_matters"] for a in allf) >= 20
    assert sum(a["undecided"] for a in allf) >= 30


def _pairs(path):
    out = {}
    for line in open(path):
        tok = line.split()
        out[int(tok[0])] = [(int(tok[j]), int(tok[j + 1])) for j in range(1, len(tok) - 1, 2)]
    return out


@pytest.mark.parametrize("name", list(he.PARTS) + ["overflow", "overflow_queue"])
def test_model_is_the_oracle_program(parts, oracle_lib, name):
    part, m = parts(name)
    if name.startswith("overflow"):
        _check_partners(part, m, 9)
        row_ptr = part.cols[1]
        n = np.diff(row_ptr)[part.n_partners:part.r1]
        assert len(n) == he.OVERFLOW_READS > 4096
        if name == "overflow":
            assert (n == he.OVERFLOW_PILE).all() and 5 * int(n.sum()) > 1 << 22        # the queue and the arena overflow
        else:
            assert 5 * int(n.sum()) <= 1 << 22                                             # the queue alone
        assert sum(1 for i in range(part.n_partners, part.r1) if len(m["annos"][i]) == 1 and not m["gated"][i]) == he.OVERFLOW_READS
        assert all(len(c.sites[0].sups) > part.fp.hinge_min_support for c in part.cases.values())      # every one is scanned: queued under force_exact(1)
    assert run_in(part.dir, oracle_lib.oracle_filter, b"G", b"G.las", 0, b"G", b"nominal.ini", b"") == 0
    want_mask = {int(a): (int(b), int(c)) for a, b, c in np.loadtxt(os.path.join(part.dir, "G.mas"), dtype=np.int64).reshape(-1, 3)}
    want_rep, want_hg = _pairs(os.path.join(part.dir, "G.repeat.txt")), _pairs(os.path.join(part.dir, "G.hinges.txt"))
    n_h = 0
    for i in range(part.r0, part.r1 + 1):
        assert tuple(m["mask"][i]) == want_mask[i], ("mask", i)
        assert m["annos"][i] == want_rep[i], ("annotations", i)
        if i < part.r1:                      # .hinges.txt stops before the part's last read
            assert m["hinges"][i] == want_hg[i], ("hinges", i)
            n_h += len(want_hg[i])
    assert n_h > 0
