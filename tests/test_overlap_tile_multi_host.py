"""k_overlap_vote_tile_multi and k_overlap_tile_reduce_multi without a GPU: hinge_amd/csrc/overlap_tile_multi_kernels.h (with the
kernel headers it includes and seed_index.h) compiled for the host (tests/overlap_tile_multi_host/driver.cpp, the stand-ins of
tests/trace_host for the HIP runtime header and the base fetch; 64 threads in lock step for the wavefront, 64 slots between two
barriers for its ballots and lane exchanges) under AddressSanitizer and UBSan, as a stand-alone program with guard words around
every tile row, the reduced row and the largest-tile word, and behind the LDS in use - value for value against the numpy model
(tests/overlap_tile_multi_common.py), job by job and block by block.  Not covered here: the real base fetch of
hinge_amd/csrc/consensus_kernels.h (the stand-in replaces it), nor anything the GPU's memory system or compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlap_common as oc
import overlap_multi_common as omc
import overlap_tile_common as otc
import overlap_tile_multi_common as otm
import seed_common as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "overlap_tile_multi_host")
SHIM = os.path.join(ROOT, "tests", "trace_host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("overlap_tile_multi_host"))
    for name in ("overlap_tile_multi_kernels.h", "overlap_tile_kernels.h", "overlap_multi_kernels.h", "overlap_kernels.h", "seed_kernels.h", "seed_index.h"):      # the kernel source itself
        shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", name), wd)
    shutil.copy(os.path.join(SHIM, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", SHIM, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _digits(a):
    return "".join(map(str, np.asarray(a).tolist()))


def _run(driver, reads, tile, stretches, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
         block_bases=oc.BLOCK_BASES):
    """Every (read, strand, block) as a job: the driver's lines against job_tiles_multi, reduce_tiles_multi and project.  Returns
    (the statuses seen, the largest tile count, the most rounds with a candidate, the largest tile's hits)."""
    rlen = [len(r) for r in reads]
    bl = otc.blocks(rlen, block_bases)
    lines = ["%d %d %d %d %d %d %d %d %d" % (k, step, window, max_occ, list_, max_partners, min_hits, tile, stretches), str(len(reads))] + [_digits(r) for r in reads]
    lines.append(str(len(bl)))
    lines += ["%d %d" % b for b in bl]
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    got = r.stdout.decode().splitlines()
    assert len(got) == len(bl) * (1 + 2 * len(reads))
    seen, at, most, deepest, top = set(), 0, 0, 0, 0
    for first, end in bl:
        index = sm.Index(reads[first:end], k, max_occ)
        assert got[at].split() == ["index", str(len(index.codes)), str(index.dropped_codes)]
        at += 1
        for a in range(len(reads)):
            for comp in (0, 1):
                Q = oc.revcomp(reads[a]) if comp else np.asarray(reads[a], np.uint8)
                tiles = otm.job_tiles_multi(index, first, a, Q, tile, step, window, list_, max_partners, min_hits, stretches)
                st, nh, rounds = otm.reduce_tiles_multi(tiles, window, max_partners, stretches)
                want = [len(tiles), max(t[1] for t in tiles), st, sum(len(c) for c in rounds), nh] + [len(c) for c in rounds]
                for cands in rounds:
                    for b, c, d, p in cands:
                        dg = oc.diag_of(rlen[a], rlen[b], comp, d)
                        want += [b, c, d, p] + list(oc.project(rlen[a], rlen[b], dg, k)) + [dg]
                v = [int(t) for t in got[at].split()]
                assert v == want, (first, a, comp, v[:24], want[:24])
                at += 1
                seen.add(st)
                most = max(most, len(tiles))
                deepest = max(deepest, sum(1 for c in rounds if c))
                top = max(top, max(t[1] for t in tiles))
    return seen, most, deepest, top


def test_multi_reads_on_the_host_at_tile_256(driver):
    """overlap_multi_common.multi_reads() at tile 256 and 3 rounds (rep0 / rep1: three diagonals, in different tiles); max_occ 8:
    the 64 threads' barriers make the ballot rounds the slow part here."""
    reads, names = omc.multi_reads()
    seen, most, deepest, top = _run(driver, reads, 256, 3, max_occ=8)
    assert {0, oc.NONE} <= seen and deepest == 3 and most == otc.tile_count(1500, oc.K, 256) == 11


def test_short_list_on_the_host_at_tile_128(driver):
    """list 64 at tile 128 (the largest tile its list * step allows): OVERFLOW in single tiles; max_partners 1: TRUNCATED per round;
    three blocks."""
    edge, en = oc.edge_reads()
    planted, names = omc.planted_reads()
    reads = planted[:6] + edge[:2] + [edge[en["tandem"]], edge[en["short"]]]
    rlen = [len(r) for r in reads]
    seen, most, deepest, top = _run(driver, reads, 128, 3, list_=64, min_hits=1, max_occ=16)
    assert oc.OVERFLOW in seen and oc.NONE in seen and top == 64 and deepest >= 2
    three = next(bb for bb in range(max(rlen), sum(rlen)) if len(oc.blocks(rlen, bb)) == 3)
    seen, most, deepest, top = _run(driver, reads, 256, 2, max_partners=1, max_occ=16, block_bases=three)
    assert oc.TRUNCATED in seen and deepest == 2


def test_random_parameters_on_the_host(driver):
    """Two-letter sequences, so that codes repeat and groups tie: small k, every step, tiles of 64 and 128, short lists that
    overflow in single tiles, few partners, small windows (several rounds), blocks."""
    rng = np.random.default_rng(5)
    seen, deep = set(), 0
    for _ in range(6):
        g = rng.integers(0, 2, size=int(rng.integers(100, 400)), dtype=np.uint8)
        reads = []
        for _ in range(int(rng.integers(2, 5))):
            a = int(rng.integers(0, len(g) - 20))
            a2 = int(rng.integers(0, len(g) - 20))                                                   # two pieces of g: two diagonals per pair
            r = np.concatenate([rng.integers(0, 4, size=int(rng.integers(0, 9)), dtype=np.uint8), g[a:a + int(rng.integers(1, 200))], g[a2:a2 + int(rng.integers(1, 120))]]).astype(np.uint8)
            reads.append(oc.revcomp(r) if rng.integers(0, 2) else r)
        step, list_ = int(rng.integers(1, 5)), int(rng.choice([64, 128, 2048]))
        tile = min(int(rng.choice([64, 128])), 128 if list_ * step >= 128 else 64)                   # (a tile is at most list * step bases)
        s, most, deepest, top = _run(driver, reads, tile, int(rng.integers(1, 9)), k=int(rng.choice([8, 9, 12, 16])), step=step, window=int(rng.choice([16, 64, 256])),
                                     max_occ=int(rng.choice([1, 3, 16])), list_=list_, max_partners=int(rng.choice([1, 2, 8])), min_hits=int(rng.integers(1, 6)),
                                     block_bases=int(rng.choice([150, 300, 1 << 20])))
        seen |= s
        deep = max(deep, deepest)
    assert {0, oc.NONE} <= seen and deep >= 2


def test_largest_list_on_the_host(driver):
    """list 8192 at 8 rounds and tile 8 192: all 132 096 bytes of LDS - 128 KiB of keys and values and the whole KiB of dead bits -,
    a tile of more than 4 096 hits (N = 8 192): noise-free reads at step 1, every read holding a stretch twice."""
    rng = np.random.default_rng(12)
    g = rng.integers(0, 4, size=1500, dtype=np.uint8)
    reads = [np.concatenate([g[a:a + 900], g[a + 300:a + 500]]).astype(np.uint8) for a in (0, 30, 60, 90, 120, 150, 180)] + [oc.revcomp(g[90:990])]
    seen, most, deepest, top = _run(driver, reads, 8192, 8, step=1, list_=8192, max_occ=16)
    assert 4096 < top <= 8192 and most == 1
    assert 0 in seen and deepest >= 2
