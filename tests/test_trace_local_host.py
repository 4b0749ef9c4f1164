"""k_trace_fill_local and k_trace_walk_local without a GPU: hinge_amd/csrc/trace_kernels.h compiled for the host (tests/trace_host:
stand-ins for the HIP runtime header and the base fetch, 64 threads in lock step for the fill's wavefront, 64 slots between two
barriers for its cross-lane reduction) under AddressSanitizer and UBSan, as a stand-alone program with guard words around the
directions, the best cell, the trace, the kept cells and the score - value for value against the numpy model
(tests/trace_local_common.py).  What this cannot show: anything the GPU's memory system or compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_common as tc
import trace_local_common as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "trace_host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("trace_local_host"))
    shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", "trace_kernels.h"), wd)       # the kernel source itself
    shutil.copy(os.path.join(HOST, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver_local")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", HOST, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver_local.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _run(driver, contigs, reads, pl, tspace, W, extend=50, match=1, diff=2, min_score=lc.MIN_SCORE):
    """One round at W of the placements' widened boxes: the driver's lines against local_round's answers."""
    boxes = [lc.widen(p, len(contigs[p[0]]), len(reads[p[1]]), extend) for p in pl]
    boxes = [b for b in boxes if abs((b[6] - b[5]) - (b[4] - b[3])) <= W]
    lines = ["%d %d %d %d %d %d" % (len(boxes), W, tspace, match, diff, min_score)]
    for b in boxes:
        lines.append("%d %d %d %s %s %d %d" % (b[3], b[2], b[5], "".join(map(str, contigs[b[0]].tolist())), "".join(map(str, reads[b[1]].tolist())), b[4], b[6]))
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    want = lc.local_round([tc.stretches(contigs, reads, b) for b in boxes], [b[3] for b in boxes], tspace, W, match, diff, min_score)
    got = r.stdout.decode().splitlines()
    assert len(got) == len(want)
    seen = set()
    for ln, (st, cells, tr, df, sc), b in zip(got, want, boxes):
        v = [int(t) for t in ln.split()]
        assert v[0] == st, (b, W, v, st)
        if st == tc.OK:
            assert v[1] == df and v[2] == sc and tuple(v[3:7]) == cells and v[7:] == tr, (b, W, v, cells, tr, df, sc)
        seen.add(st)
    return seen


def test_hand_cases_on_the_host(driver):
    contigs, reads, pl, calls = lc.hand_cases()
    seen = set()
    for label, names, kw in calls:
        kw = dict(kw)
        band, band_max, ts = kw.pop("band"), kw.pop("band_max"), kw.pop("tspace")
        for W in sorted({band, band_max}):                                             # the first round's band and the last one's
            seen |= _run(driver, contigs, reads, [pl[n] for n in names], ts, W, **kw)
    assert {tc.OK, tc.TOUCHED, lc.EMPTY} <= seen


def test_many_perturbed_on_the_host(driver):
    contigs, reads, pl = lc.perturbed_many()
    assert tc.OK in _run(driver, contigs, reads, pl, 100, 128)


def test_random_pairs_on_the_host(driver):
    """60 short stretches of two letters with any length ratio the band admits: steep and falling centre lines, both strands, flanks
    for the widening to use; small scores and two letters so that equal maxima and ties inside a cell are common."""
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(60):
        alen, blen, ab, fl, comp = int(rng.integers(1, 121)), int(rng.integers(1, 121)), int(rng.integers(0, 150)), int(rng.integers(0, 9)), int(rng.integers(0, 2))
        contig = rng.integers(0, 2, size=ab + alen + int(rng.integers(0, 9)), dtype=np.uint8)
        whole = np.concatenate([rng.integers(0, 4, size=fl, dtype=np.uint8), rng.integers(0, 2, size=blen, dtype=np.uint8), rng.integers(0, 4, size=int(rng.integers(0, 9)), dtype=np.uint8)]).astype(np.uint8)
        read = tc.revcomp(whole) if comp else whole
        m, x = [(1, 2), (1, 1), (2, 3), (15, 1)][int(rng.integers(0, 4))]
        seen |= _run(driver, [contig], [read], [(0, 0, comp, ab, ab + alen, fl, fl + blen)], int(rng.choice([7, 100, 200])), int(rng.choice([8, 24, 128])), extend=int(rng.integers(0, 7)),
                     match=m, diff=x, min_score=int(rng.choice([1, 6, 40 * m])))
    assert {tc.OK, tc.TOUCHED, lc.EMPTY} <= seen
