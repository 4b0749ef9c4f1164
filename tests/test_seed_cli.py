"""`hinge seed` without a GPU: usage and error exits, and the PAF text of hand-made placements (--self-test-paf: the writer alone, not in the usage text) -
names, strand and coordinates as `hinge paf2las` reads them back: its parser takes every line (it gets as far as asking for the
GPU), and refuses the same text with a wrong length."""
import os
import subprocess

import numpy as np

from hinge_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")


def _run(cmd, wd):
    return subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _dbs(wd):
    rng = np.random.default_rng(2)
    contigs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (900, 1200)]
    reads = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (500, 640, 333)]
    formats.write_db(os.path.join(wd, "draft"), np.asarray([len(c) for c in contigs], np.int32), bases=contigs)
    formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return contigs, reads


def test_usage_and_error_exits(tmp_path):
    wd = str(tmp_path)
    _dbs(wd)
    r = _run([HINGE, "seed"], wd)
    assert r.returncode == 1 and b"usage: seed <draft db> <read db> <out.paf>" in r.stderr and b"--max-placements" in r.stderr and b"self-test" not in r.stderr
    for extra, text in ((["--bogus"], b"unknown option --bogus"), (["--k"], b"--k needs a value"), (["--window", "0"], b"--window needs a positive number"), (["extra"], b"usage:")):
        r = _run([HINGE, "seed", "draft", "reads", "x.paf"] + extra, wd)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stderr)
    r = _run([HINGE, "seed", "nodraft", "reads", "x.paf"], wd)
    assert r.returncode == 1 and b"Could not open database" in r.stderr
    r = _run([HINGE, "paf2las"], wd)
    assert r.returncode == 1 and b"hinge seed" in r.stderr                          # paf2las names its producer
    assert not os.path.exists(os.path.join(wd, "x.paf"))


def test_paf_text_of_hand_made_placements(tmp_path):
    wd = str(tmp_path)
    _dbs(wd)
    # read comp contig abpos aepos bbpos bepos count diag
    rows = [(0, 0, 0, 100, 600, 0, 500, 41, 100), (1, 1, 1, 0, 400, 240, 640, 17, 660), (2, 1, 0, 700, 900, 0, 200, 9, 700), (2, 0, 1, 5, 338, 0, 333, 3, 905)]
    open(os.path.join(wd, "pl.txt"), "w").write("".join(" ".join(map(str, r)) + "\n" for r in rows))
    r = _run([HINGE, "seed", "draft", "reads", "x.paf", "--self-test-paf", "pl.txt"], wd)
    assert r.returncode == 0, r.stderr
    want = ["read/1/0_500\t500\t0\t500\t+\tcontig/1/0_900\t900\t100\t600\t41\t500\t255\tsd:i:100\tsc:i:41",
            "read/2/0_640\t640\t0\t400\t-\tcontig/2/0_1200\t1200\t0\t400\t17\t400\t255\tsd:i:660\tsc:i:17",        # `-`: [240, 640) of the complement = [0, 400) of the stored read
            "read/3/0_333\t333\t133\t333\t-\tcontig/1/0_900\t900\t700\t900\t9\t200\t255\tsd:i:700\tsc:i:9",
            "read/3/0_333\t333\t0\t333\t+\tcontig/2/0_1200\t1200\t5\t338\t3\t333\t255\tsd:i:905\tsc:i:3"]
    assert open(os.path.join(wd, "x.paf")).read().splitlines() == want
    # the conversion back, as paf2las_main.cpp does it: bbpos = qlen - qe, bepos = qlen - qs on a `-` line; ids between the slashes
    for ln, row in zip(want, rows):
        f = ln.split("\t")
        b, a, qlen, qs, qe = int(f[0].split("/")[1]) - 1, int(f[5].split("/")[1]) - 1, int(f[1]), int(f[2]), int(f[3])
        comp = int(f[4] == "-")
        assert (b, comp, a, int(f[7]), int(f[8]), qlen - qe if comp else qs, qlen - qs if comp else qe) == row[:7]
    # paf2las's own parser takes every line: it gets as far as the GPU (exit 0 with one, 2 "no usable GPU" without), never a line error
    r = _run([HINGE, "paf2las", "draft", "reads", "x.paf", "x.las", "--ends", "local"], wd)
    assert r.returncode in (0, 2) and b" line " not in r.stderr, r.stderr
    assert r.returncode == 0 or b"no usable GPU" in r.stderr
    # ... and refuses the same text once a length is wrong
    open(os.path.join(wd, "bad.paf"), "w").write(want[0].replace("\t500\t0\t500\t+", "\t501\t0\t500\t+") + "\n")
    r = _run([HINGE, "paf2las", "draft", "reads", "bad.paf", "y.las", "--ends", "local"], wd)
    assert r.returncode == 1 and b"line 1: the query length is not the read's length" in r.stderr
    r = _run([HINGE, "seed", "draft", "reads", "x.paf", "--self-test-paf", "none.txt"], wd)
    assert r.returncode == 1 and b"cannot read none.txt" in r.stderr
    open(os.path.join(wd, "far.txt"), "w").write("7 0 0 1 2 3 4 5 6\n")
    r = _run([HINGE, "seed", "draft", "reads", "x.paf", "--self-test-paf", "far.txt"], wd)
    assert r.returncode == 1 and b"an id outside its DB" in r.stderr
