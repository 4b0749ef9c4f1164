"""k_seed_vote without a GPU: hinge_amd/csrc/seed_kernels.h and seed_index.h compiled for the host (tests/seed_host/driver.cpp, the
stand-ins of tests/trace_host for the HIP runtime header and the base fetch; 64 threads in lock step for the wavefront, 64 slots
between two barriers for its ballots and its cross-lane reduction) under AddressSanitizer and UBSan, as a stand-alone program with
guard words around the output and behind the LDS - value for value against the numpy model (tests/seed_common.py), job by job.
Not covered here: the real base fetch of hinge_amd/csrc/consensus_kernels.h - CnsPair::B, the complemented strand included - is replaced
by the stand-in tests/trace_host/consensus_kernels.h (the real header needs a device compiler), so only the GPU tests exercise it; nor
anything the GPU's memory system or compiler does differently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import seed_common as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "seed_host")
SHIM = os.path.join(ROOT, "tests", "trace_host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("seed_host"))
    for name in ("seed_kernels.h", "seed_index.h"):                                   # the kernel source itself
        shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", name), wd)
    shutil.copy(os.path.join(SHIM, "consensus_kernels.h"), wd)
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", SHIM, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _digits(a):
    return "".join(map(str, np.asarray(a).tolist()))


def _run(driver, contigs, reads, k=sm.K, step=sm.STEP, window=sm.WINDOW, max_occ=sm.MAX_OCC, list_=sm.LIST, max_placements=1, min_hits=sm.MIN_HITS):
    """Both strands of every read as jobs: the driver's lines against job_picks and project.  Returns the statuses seen."""
    index = sm.Index(contigs, k, max_occ)
    lines = ["%d %d %d %d %d %d %d" % (k, step, window, max_occ, list_, max_placements, min_hits), str(len(contigs))] + [_digits(c) for c in contigs]
    jobs = [(b, comp) for b in range(len(reads)) for comp in (0, 1)]
    lines.append(str(len(jobs)))
    lines += ["%d %s" % (comp, _digits(reads[b])) for b, comp in jobs]
    r = subprocess.run([driver], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    got = r.stdout.decode().splitlines()
    assert got[0].split() == ["index", str(len(index.codes)), str(index.dropped_codes)]
    assert len(got) == 1 + len(jobs)
    seen = []
    for ln, (b, comp) in zip(got[1:], jobs):
        read = np.asarray(reads[b], np.uint8)
        st, nh, picks = sm.job_picks(index, sm.revcomp(read) if comp else read, step, window, list_, max_placements, min_hits)
        want = [st, len(picks), nh]
        for pk in picks:
            q = sm.project(index, len(read), comp, b, pk)
            want += list(pk) + ([1, q[0]] + list(q[3:7]) if q else [0])
        v = [int(t) for t in ln.split()]
        assert v == want, (b, comp, v, want)
        seen.append(st)
    return seen


def test_edge_list_on_the_host(driver):
    seen = {}
    for label, contigs, reads, kw, host_only in sm.edge_calls():
        seen[label] = _run(driver, contigs, reads, **kw)
    assert seen["lengths"][0:2] == [sm.NONE, sm.NONE] and sm.OK in seen["lengths"][2:4] and sm.OK in seen["lengths"][4:6]
    assert sm.OVERFLOW in seen["over65"] and sm.OVERFLOW not in seen["fill64"] and sm.OK in seen["fill64"]
    assert seen["long_read"][0] == sm.OK


def test_cns_tiny_on_the_host(driver):
    from hinge_amd import synth_consensus as sc
    d = sc.generate(sc.CONFIGS["cns_tiny"])
    seen = _run(driver, d.contigs, d.reads[:24], max_placements=2)
    assert sm.OK in seen and sm.NONE in seen


def test_random_parameters_on_the_host(driver):
    """Two-letter sequences, so that codes repeat and windows tie: small k, every step, short lists that overflow, N up to 8."""
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(12):
        contigs = [rng.integers(0, 2, size=int(rng.integers(20, 400)), dtype=np.uint8) for _ in range(int(rng.integers(1, 4)))]
        reads = []
        for _ in range(3):
            c = contigs[int(rng.integers(0, len(contigs)))]
            a = int(rng.integers(0, len(c)))
            r = np.concatenate([rng.integers(0, 4, size=int(rng.integers(0, 9)), dtype=np.uint8), c[a:a + int(rng.integers(1, 200))]]).astype(np.uint8)
            reads.append(sm.revcomp(r) if rng.integers(0, 2) else r)
        seen |= set(_run(driver, contigs, reads, k=int(rng.choice([8, 9, 12, 16])), step=int(rng.integers(1, 5)), window=int(rng.choice([16, 64, 256])),
                         max_occ=int(rng.choice([1, 3, 16, 40])), list_=int(rng.choice([64, 64, 128, 2048])), max_placements=int(rng.choice([1, 2, 8])), min_hits=int(rng.integers(1, 6))))
    assert seen == {sm.OK, sm.NONE, sm.OVERFLOW}
