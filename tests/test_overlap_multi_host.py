"""k_overlap_vote_multi without a GPU: hinge_amd/csrc/overlap_multi_kernels.h (with overlap_kernels.h, seed_kernels.h and
seed_index.h) compiled for the host (tests/overlap_multi_host/driver.cpp, the stand-ins of tests/trace_host for the HIP runtime
header and the base fetch; 64 threads in lock step for the wavefront, 64 slots between two barriers for its ballots) under
AddressSanitizer and UBSan, as a stand-alone program with guard words around the output and behind the LDS in use (16 bytes and one
dead bit per slot) - value for value against the numpy model (tests/overlap_multi_common.py).  Hand-made hit lists reach the kernel
through a hand-made index: one entry per hit of the query's k-mer at p, placed in target b on diagonal d.  Not covered here: the
real base fetch of hinge_amd/csrc/consensus_kernels.h, nor anything the GPU's memory system or compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlap_common as oc
import overlap_multi_common as om
import seed_common as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "overlap_multi_host")
SHIM = os.path.join(ROOT, "tests", "trace_host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("overlap_multi_host"))
    for name in ("overlap_multi_kernels.h", "overlap_kernels.h", "seed_kernels.h", "seed_index.h"):      # the kernel source itself
        shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", name), wd)
    shutil.copy(os.path.join(SHIM, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", SHIM, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _digits(a):
    return "".join(map(str, np.asarray(a).tolist()))


def _call(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return r.stdout.decode().splitlines()


def _want_line(st, nh, rounds):
    want = [st, sum(len(c) for c in rounds), nh] + [len(c) for c in rounds]
    for cands in rounds:
        for c in cands:
            want += list(c)
    return want


def _run(driver, reads, stretches, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
         block_bases=oc.BLOCK_BASES):
    """Every (read, strand, block) as a job: the driver's lines against job_candidates_multi.  Returns (statuses seen, most rounds with a candidate)."""
    rlen = [len(r) for r in reads]
    bl = oc.blocks(rlen, block_bases)
    lines = ["reads %d %d %d %d %d %d %d %d" % (k, step, window, max_occ, list_, max_partners, min_hits, stretches), str(len(reads))] + [_digits(r) for r in reads]
    lines.append(str(len(bl)))
    lines += ["%d %d" % b for b in bl]
    got = _call(driver, lines)
    assert len(got) == len(bl) * (1 + 2 * len(reads))
    seen, deepest, at = set(), 0, 0
    for first, end in bl:
        index = sm.Index(reads[first:end], k, max_occ)
        assert got[at].split() == ["index", str(len(index.codes)), str(index.dropped_codes)]
        at += 1
        for a in range(len(reads)):
            for comp in (0, 1):
                Q = oc.revcomp(reads[a]) if comp else np.asarray(reads[a], np.uint8)
                st, nh, rounds = om.job_candidates_multi(index, first, a, Q, step, window, list_, max_partners, min_hits, stretches)
                v = [int(t) for t in got[at].split()]
                assert v == _want_line(st, nh, rounds), (first, a, comp, v[:24], _want_line(st, nh, rounds)[:24])
                at += 1
                seen.add(st)
                deepest = max(deepest, sum(1 for c in rounds if c))
    return seen, deepest


def _run_hits(driver, groups, stretches, window, min_hits, list_=64, max_partners=8, seed=3):
    """Hand-made hits [(b, d, n)]: n hits of target b on diagonal d, one sampled position each.  Returns the rounds."""
    k, alen = oc.K, oc.K + 63                                            # 64 sampled positions at stride 1, list 64
    assert sm.stride(alen, k, 1, list_) == 1 and sum(n for _, _, n in groups) <= alen - k + 1
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 4, size=alen, dtype=np.uint8)
    codes = sm.kmer_codes(q, k)
    assert len(set(codes.tolist())) == len(codes)                        # every k-mer of the query once: a hit list is what is planted
    b, d, p = [], [], []
    for bb, dd, n in groups:
        b += [bb] * n; d += [dd] * n; p += list(range(len(p), len(p) + n))
    n_targets = max(b) + 1
    lines = ["hits %d 1 %d 4 %d %d %d %d" % (k, window, list_, max_partners, min_hits, stretches), _digits(q), str(n_targets)] + ["100000"] * n_targets
    lines += [str(len(b))] + ["%d %d %d" % (x, y + alen, z) for x, y, z in zip(b, d, p)]          # (d + alen: every hit inside its target)
    got = _call(driver, lines)
    rounds = om.pick_rounds(b, [v + alen for v in d], p, window, min_hits, stretches)
    rounds = [[(x + 1, c, y, z) for x, c, y, z in cands] for cands in rounds]                     # (the targets are reads 1 ..)
    trunc = any(len(c) > max_partners for c in rounds)
    rounds = [c[:max_partners] for c in rounds]
    st = (om.TRUNCATED if trunc else 0) if any(rounds) else om.NONE
    assert [int(t) for t in got[0].split()] == _want_line(st, len(b), rounds), (groups, got[0])
    return [[(x - 1, c, y - alen, z) for x, c, y, z in cands] for cands in rounds]


def test_hand_made_hit_lists_on_the_host(driver):
    """The cases of test_overlap_multi_model.py through the kernel itself."""
    W = 16
    for lo, hi, later in ((84, 116, 2), (85, 116, 1), (84, 115, 1), (85, 115, 0)):                 # the suppression bounds
        rounds = _run_hits(driver, [(7, lo, 1), (7, 100, 5), (7, 110, 5), (7, hi, 2)], 4, W, 1)
        assert sum(len(r) for r in rounds[1:]) == later
    # a dead representative
    assert _run_hits(driver, [(0, 84, 1), (0, 93, 4), (0, 100, 6), (0, 110, 6)], 3, W, 3) == [[(0, 12, 110, 11)], [(0, 5, 93, 2)], []]
    # a group of fewer elements than rounds; a second pick of exactly min_hits and of min_hits - 1
    assert _run_hits(driver, [(1, 50, 1), (1, 500, 1)], 4, W, 1) == [[(1, 1, 50, 0)], [(1, 1, 500, 1)], [], []]
    assert [len(r) for r in _run_hits(driver, [(1, 50, 5), (1, 500, 3), (2, 70, 3)], 3, W, 3)] == [2, 1, 0]
    assert [len(r) for r in _run_hits(driver, [(1, 50, 5), (1, 500, 2), (2, 70, 3)], 3, W, 3)] == [2, 0, 0]
    # eight rounds, eight stretches of one partner; more candidates per round than partners: TRUNCATED, the first b kept in each
    assert [len(r) for r in _run_hits(driver, [(0, 100 * x, 2) for x in range(1, 9)] + [(1, 40, 2)], 8, W, 2)] == [2] + [1] * 7
    rounds = _run_hits(driver, [(0, 100, 3), (0, 300, 2), (1, 40, 3), (1, 400, 2)], 2, W, 2, max_partners=1)
    assert [[c[0] for c in r] for r in rounds] == [[0], [0]]
    # a full list of 64: no padding, the dead bits' two words both in use
    assert [len(r) for r in _run_hits(driver, [(0, 100, 40), (0, 900, 24)], 2, W, 6)] == [1, 1]


def test_planted_reads_on_the_host(driver):
    """The planted pairs and six reads of the edge set; max_occ 16: the 64 threads' barriers make the ballot rounds the slow part."""
    edge, en = oc.edge_reads()
    planted, names = om.planted_reads()
    reads = planted + edge[:4] + [edge[en["tandem"]], edge[en["short"]]]
    rlen = [len(r) for r in reads]
    seen, deepest = _run(driver, reads, 3, max_occ=16)
    assert {0, oc.NONE} <= seen and deepest == 3                         # rep0 / rep1: a main diagonal and two cross ones
    two = next(bb for bb in range(max(rlen), sum(rlen)) if len(oc.blocks(rlen, bb)) == 2)
    seen, deepest = _run(driver, reads, 2, max_occ=16, block_bases=two, max_partners=1, list_=64, min_hits=2)
    assert oc.OVERFLOW | oc.TRUNCATED in seen


def test_largest_list_on_the_host(driver):
    """list 8192 at 8 rounds: 128 KiB of keys and values and the whole KiB of dead bits, a hit count beyond 4 096 (N = 8 192) -
    noise-free reads at step 1, every read holding a stretch twice."""
    rng = np.random.default_rng(12)
    g = rng.integers(0, 4, size=1500, dtype=np.uint8)
    reads = [np.concatenate([g[a:a + 900], g[a + 300:a + 500]]).astype(np.uint8) for a in (0, 30, 60, 90, 120, 150, 180)] + [oc.revcomp(g[90:990])]
    index = sm.Index(reads, oc.K, 16)
    nh = max(om.job_candidates_multi(index, 0, a, reads[a], 1, oc.WINDOW, 8192, oc.MAX_PARTNERS, oc.MIN_HITS, 8)[1] for a in range(len(reads)))
    assert 4096 < nh <= 8192
    seen, deepest = _run(driver, reads, 8, step=1, list_=8192, max_occ=16)
    assert 0 in seen and deepest >= 2
