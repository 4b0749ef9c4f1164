"""The device build of the k-mer index without a GPU: hinge_amd/csrc/index_kernels.h itself (with seed_kernels.h and seed_index.h)
compiled for the host (tests/index_host/driver.cpp, the stand-ins of tests/trace_host for the HIP runtime header and the base
fetch; 64 threads in lock step for the wavefront, 64 slots between two barriers for its ballots, a launch's workgroups one after
the other) under AddressSanitizer and UBSan, as a stand-alone program with guard words around every output and scratch array and
behind the LDS - value for value against seed_build_index inside the program and against the numpy model (seed_common.Index) here.
Not covered here: the real base fetch of hinge_amd/csrc/consensus_kernels.h (the stand-in replaces it), the launches of
index_capi.inc (the driver restates their order), nor anything the GPU's memory system or compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import index_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "index_host")
SHIM = os.path.join(ROOT, "tests", "trace_host")
T = ic.tile_from_source()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("index_host"))
    for name in ("index_kernels.h", "seed_kernels.h", "seed_index.h"):                # the kernel source itself
        shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", name), wd)
    shutil.copy(os.path.join(SHIM, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", SHIM, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _run(driver, reads, k, max_occ, ranges=None, label=""):
    """The driver's build of every range against the model; returns [(codes, gpos, off, dropped, entries, passes)] per range."""
    ranges = ranges or [(0, len(reads))]
    lines = ["%d %d" % (k, max_occ), str(len(reads))] + ["".join(map(str, np.asarray(r).tolist())) or "-" for r in reads]
    lines += [str(len(ranges))] + ["%d %d" % r for r in ranges]
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (label, r.returncode, r.stdout[-300:], r.stderr[-3000:])
    got = r.stdout.decode().split("\n")
    out = []
    for x, (first, end) in enumerate(ranges):
        head = got[4 * x].split()
        assert head[0] == "index"
        n, kept, dropped, passes = (int(v) for v in head[1:])
        codes, gpos, off = (np.asarray([int(v) for v in got[4 * x + q].split()], np.int64) for q in (1, 2, 3))
        assert n == ic.entries(reads[first:end], k) and kept == len(codes) and passes == (2 * k + 7) // 8
        ic.check((codes, gpos, off, dropped), reads[first:end], k, max_occ, (label, first, end))
        out.append((codes, gpos, off, dropped, n, passes))
    return out


def test_tile_boundaries_on_the_host(driver):
    """Entry counts around the scatter's tile, 0 and 1 entries; max_occ 1 with a run of two across the first tile boundary."""
    rng = np.random.default_rng(21)
    for n in (T - 1, T, T + 1):
        assert _run(driver, ic.one_read_of(rng, n, 9), 9, 4, label="n%d" % n)[0][4] == n
    assert _run(driver, ic.rand_reads(rng, [3, 7, 1]), 8, 16, label="none")[0][4] == 0
    assert _run(driver, ic.rand_reads(rng, [8]), 8, 16, label="one")[0][4] == 1
    reads = ic.straddle(T)
    got = _run(driver, reads, 8, 1, label="straddle")[0]
    c = ic.sorted_codes(reads, 8)
    assert c[T] not in got[0].tolist() and got[3] >= 1


def test_stability_on_the_host(driver):
    """Two-letter reads (codes with many entries: gpos must ascend inside each), a homopolymer across several tiles, and the same
    code at exactly max_occ = 256 and at 257 entries."""
    rng = np.random.default_rng(22)
    reads = ic.rand_reads(rng, [700, 11, 650, 900, 1], letters=2)
    codes, gpos, _, dropped, n, _ = _run(driver, reads, 8, 256, label="two_letter")[0]
    assert n > T and dropped == 0 and np.bincount(codes.astype(np.int64)).max() > 16 and ic.gpos_ascends_within_codes(codes, gpos)
    homo = [rng.integers(0, 4, size=150, dtype=np.uint8), np.zeros(2 * T + 500, np.uint8), rng.integers(0, 4, size=90, dtype=np.uint8)]
    codes, gpos, _, dropped, n, _ = _run(driver, homo, 12, 256, label="homopolymer")[0]
    assert n > 2 * T and dropped == 1 and 0 not in codes.tolist()
    at256, at257 = ic.homopolymer_sets(10)
    codes, gpos, _, dropped, _, _ = _run(driver, at256, 10, 256, label="at256")[0]
    assert int((codes == 0).sum()) == 256 and ic.gpos_ascends_within_codes(codes, gpos)
    codes, gpos, _, dropped, _, _ = _run(driver, at257, 10, 256, label="at257")[0]
    assert int((codes == 0).sum()) == 0 and dropped >= 1


def test_k16_and_k_values_on_the_host(driver):
    """k = 16: all 32 bits of the code, four full digits, codes with the top bit set; k = 8, 12, 15: two, three, four passes."""
    rng = np.random.default_rng(23)
    reads = ic.rand_reads(rng, [1203, 15, 1101, 16])
    codes = _run(driver, reads, 16, 16, label="k16")[0][0]
    assert (codes >= 2 ** 31).any() and (codes < 2 ** 31).any()
    for k in (8, 12, 15):
        assert _run(driver, reads[:2] + [reads[2][:517]], k, 3, label="k%d" % k)[0][5] == (2 * k + 7) // 8


def test_scan_depth_on_the_host(driver):
    """The scan alone (the driver's "scan" input: the real k_index_scan_sums / k_index_scan_apply and the recursion over the one
    sums array) at one, two and three levels and at the seams between them - n + 1 == C * C is a second level of exactly one full
    chunk, C * C + 1 a second level of C + 1 elements and a third of 2, C * C + C + 1 a third of 3 - over flags (0 / 1) and over tile
    counts (0 .. 300), against a serial exclusive scan inside the program."""
    C = ic.scan_chunk_from_source()
    for x, n in enumerate((1, C - 1, C, C + 1, C * C - 1, C * C, C * C + 1, C * C + C + 1)):
        for max_value in (1, 300):
            r = subprocess.run([driver], input=("scan %d %d %d\n" % (n, 100 + x, max_value)).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 0, (n, max_value, r.returncode, r.stdout[-300:], r.stderr[-3000:])
            head = r.stdout.decode().split()
            assert head[0] == "scan" and int(head[1]) == n and int(head[2]) == ic.scan_levels(n, C) == (1 if n <= C else 2 if n <= C * C else 3)
            nb1 = -(-n // C)
            nb2 = -(-nb1 // C)
            assert int(head[3]) == (0 if n <= C else nb1 if nb1 <= C else nb1 + nb2) and (0 < int(head[4]) < 2 ** 31 or n == 1)
            assert r.stderr == b""


def test_short_reads_and_ranges_on_the_host(driver):
    """Reads shorter than k between longer ones (off and the entry offsets differ); ranges with first > 0, a single-read range and
    a range of short reads only: gpos is relative to the range."""
    rng = np.random.default_rng(24)
    reads = ic.rand_reads(rng, [5, 333, 14, 1, 402, 15, 7, 129, 3])
    got = _run(driver, reads, 15, 16, ranges=[(0, 9), (1, 5), (4, 5), (5, 7), (2, 9)], label="ranges")
    assert got[1][2].tolist() == [0, 333, 347, 348, 750] and got[2][1].max() == 402 - 15 and got[3][4] == 1 and got[0][4] == 319 + 388 + 1 + 115
