"""k_overlap_vote_tile and k_overlap_tile_reduce without a GPU: hinge_amd/csrc/overlap_tile_kernels.h (with overlap_kernels.h,
seed_kernels.h and seed_index.h) compiled for the host (tests/overlap_tile_host/driver.cpp, the stand-ins of tests/trace_host for the
HIP runtime header and the base fetch; 64 threads in lock step for the wavefront, 64 slots between two barriers for its ballots
and lane exchanges) under AddressSanitizer and UBSan, as a stand-alone program with guard words around every output row and behind
the LDS - value for value against the numpy model (tests/overlap_tile_common.py), job by job and block by block.  Not covered
here: the real base fetch of hinge_amd/csrc/consensus_kernels.h (the stand-in replaces it), nor anything the GPU's memory system or
compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlap_common as oc
import overlap_tile_common as otc
import seed_common as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "overlap_tile_host")
SHIM = os.path.join(ROOT, "tests", "trace_host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("overlap_tile_host"))
    for name in ("overlap_tile_kernels.h", "overlap_kernels.h", "seed_kernels.h", "seed_index.h"):              # the kernel source itself
        shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", name), wd)
    shutil.copy(os.path.join(SHIM, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", SHIM, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _digits(a):
    return "".join(map(str, np.asarray(a).tolist()))


def _run(driver, reads, tile, k=oc.K, step=oc.STEP, window=oc.WINDOW, max_occ=oc.MAX_OCC, list_=oc.LIST, max_partners=oc.MAX_PARTNERS, min_hits=oc.MIN_HITS,
         block_bases=oc.BLOCK_BASES):
    """Every (read, strand, block) as a job: the driver's lines against job_tiles, reduce_tiles and project.  Returns (the statuses
    seen, the largest tile count)."""
    rlen = [len(r) for r in reads]
    bl = otc.blocks(rlen, block_bases)
    lines = ["%d %d %d %d %d %d %d %d" % (k, step, window, max_occ, list_, max_partners, min_hits, tile), str(len(reads))] + [_digits(r) for r in reads]
    lines.append(str(len(bl)))
    lines += ["%d %d" % b for b in bl]
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    got = r.stdout.decode().splitlines()
    assert len(got) == len(bl) * (1 + 2 * len(reads))
    seen, at, most = set(), 0, 0
    for first, end in bl:
        index = sm.Index(reads[first:end], k, max_occ)
        assert got[at].split() == ["index", str(len(index.codes)), str(index.dropped_codes)]
        at += 1
        for a in range(len(reads)):
            for comp in (0, 1):
                Q = oc.revcomp(reads[a]) if comp else np.asarray(reads[a], np.uint8)
                tiles = otc.job_tiles(index, first, a, Q, tile, step, window, list_, max_partners, min_hits)
                st, nh, cands = otc.reduce_tiles(tiles, max_partners)
                want = [len(tiles), max(t[1] for t in tiles), st, len(cands), nh]
                for b, c, d, p in cands:
                    dg = oc.diag_of(rlen[a], rlen[b], comp, d)
                    want += [b, c, d, p] + list(oc.project(rlen[a], rlen[b], dg, k)) + [dg]
                v = [int(t) for t in got[at].split()]
                assert v == want, (first, a, comp, v[:20], want[:20])
                at += 1
                seen.add(st)
                most = max(most, len(tiles))
    return seen, most


def test_edge_set_on_the_host_at_tile_256(driver):
    """The special reads of the shared edge set and four ordinary ones at tile 256 (up to eleven tiles per read; list 64 at tile 128,
    the largest its list * step allows), max_occ 8 where
    the call does not set it: the 64 threads' barriers make the ballot rounds the slow part here."""
    reads, names = oc.edge_reads()
    reads = reads[:4] + reads[30:]
    rlen = [len(r) for r in reads]
    three = next(bb for bb in range(max(rlen), sum(rlen)) if len(oc.blocks(rlen, bb)) == 3 and any(e - f == 1 for f, e in oc.blocks(rlen, bb)))
    seen = {}
    for label, kw in (("list64_min_hits1", dict(list_=64, min_hits=1, max_occ=16)), ("partners1", dict(max_partners=1)), ("three_blocks", dict(block_bases=three, max_partners=2)),
                      ("step3", dict(step=3, window=16, min_hits=2))):
        tile = 128 if kw.get("list_") == 64 else 256                    # (a tile is at most list * step bases)
        seen[label], most = _run(driver, reads, tile, **dict(dict(max_occ=8), **kw))
        assert most == otc.tile_count(1500, oc.K, tile) == (11 if tile == 256 else 23)
    assert oc.OVERFLOW in seen["list64_min_hits1"] and oc.NONE in seen["list64_min_hits1"]
    assert oc.TRUNCATED in seen["partners1"] and 0 in seen["partners1"]


def test_random_parameters_on_the_host(driver):
    """Two-letter sequences, so that codes repeat and groups tie: small k, every step, tiles of 64 and 128, short lists that
    overflow in single tiles, few partners, blocks."""
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(6):
        g = rng.integers(0, 2, size=int(rng.integers(100, 400)), dtype=np.uint8)
        reads = []
        for _ in range(int(rng.integers(2, 5))):
            a = int(rng.integers(0, len(g) - 20))
            r = np.concatenate([rng.integers(0, 4, size=int(rng.integers(0, 9)), dtype=np.uint8), g[a:a + int(rng.integers(1, 200))]]).astype(np.uint8)
            reads.append(oc.revcomp(r) if rng.integers(0, 2) else r)
        step, list_ = int(rng.integers(1, 5)), int(rng.choice([64, 128, 2048]))
        tile = min(int(rng.choice([64, 128])), 128 if list_ * step >= 128 else 64)                   # (a tile is at most list * step bases)
        s, most = _run(driver, reads, tile, k=int(rng.choice([8, 9, 12, 16])), step=step, window=int(rng.choice([16, 64, 256])), max_occ=int(rng.choice([1, 3, 16])),
                       list_=list_, max_partners=int(rng.choice([1, 2, 8])), min_hits=int(rng.integers(1, 6)), block_bases=int(rng.choice([150, 300, 1 << 20])))
        seen |= s
    assert {0, oc.NONE} <= seen
