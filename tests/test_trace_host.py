"""The kernels of `hinge paf2las` without a GPU: hinge_amd/csrc/trace_kernels.h compiled for the host (tests/trace_host: stand-ins
for the HIP runtime header and the base fetch, 64 threads in lock step for a wavefront) under AddressSanitizer and UBSan, value for
value against the numpy model.  What this cannot show: anything the GPU's memory system or compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "trace_host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("trace_host"))
    shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", "trace_kernels.h"), wd)       # the kernel source itself
    shutil.copy(os.path.join(HOST, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", HOST, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _run(driver, contigs, reads, pl, tspace, W):
    pl = [p for p in pl if abs((p[6] - p[5]) - (p[4] - p[3])) <= W]
    lines = ["%d %d %d" % (len(pl), W, tspace)]
    for p in pl:
        lines.append("%d %d %d %s %s %d %d" % (p[3], p[2], p[5], "".join(map(str, contigs[p[0]].tolist())), "".join(map(str, reads[p[1]].tolist())), p[4], p[6]))
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    want = tc.align_round([tc.stretches(contigs, reads, p) for p in pl], [p[3] for p in pl], tspace, W)
    got = r.stdout.decode().splitlines()
    assert len(got) == len(want)
    for ln, (st, tr, df), p in zip(got, want, pl):
        v = [int(t) for t in ln.split()]
        assert v[0] == st and (st != tc.OK or (v[1] == df and v[2:] == tr)), (p, W, v, st, tr, df)
    return len(pl)


def test_hand_cases_on_the_host(driver):
    contigs, reads, cases = tc.hand_cases()
    pl = [p for _, p, _ in cases]
    for W, ts in ((8, 100), (128, 100), (128, 200), (1024, 100), (2048, 100)):      # the smallest, the default and the two widest bands
        assert _run(driver, contigs, reads, pl, ts, W) == len(pl)


def test_indel_cases_on_the_host(driver):
    contigs, reads, pl = tc.indel_cases()
    for W, ts in ((16, 100), (32, 100), (64, 100), (512, 100), (512, 200)):
        assert _run(driver, contigs, reads, pl, ts, W) >= 2


def test_random_pairs_on_the_host(driver):
    """Short stretches of two letters with any length ratio the band admits: steep and falling centre lines, both strands, flanks."""
    rng = np.random.default_rng(2)
    n = 0
    for _ in range(30):
        alen, blen, ab, fl, comp = int(rng.integers(1, 120)), int(rng.integers(1, 120)), int(rng.integers(0, 150)), int(rng.integers(0, 5)), int(rng.integers(0, 2))
        contig = rng.integers(0, 2, size=ab + alen + 3, dtype=np.uint8)
        whole = np.concatenate([rng.integers(0, 4, size=fl, dtype=np.uint8), rng.integers(0, 2, size=blen, dtype=np.uint8), rng.integers(0, 4, size=2, dtype=np.uint8)]).astype(np.uint8)
        read = tc.revcomp(whole) if comp else whole
        for W in (8, 24, 48):
            n += _run(driver, [contig], [read], [(0, 0, comp, ab, ab + alen, fl, fl + blen)], int(rng.choice([7, 100])), W)
    assert n > 30
