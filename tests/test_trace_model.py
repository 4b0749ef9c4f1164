"""`hinge paf2las` without a GPU: the numpy model of the banded alignment (tests/trace_common.py) against the properties the trace
of a .las must have, `hinge correct-head`, the PAF strand arithmetic, and the command lines' usage / error exits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import trace_common as tc
from hinge_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")
TSPACE = 100


@pytest.fixture(scope="module")
def hand():
    contigs, reads, cases = tc.hand_cases()
    res = tc.model_run(contigs, reads, [p for _, p, _ in cases], TSPACE)
    return contigs, reads, cases, res


def _segments(p, trace, tspace):
    """[(a0, a1, b0, b1)] of a placement's trace."""
    ab, ae, bb = int(p[3]), int(p[4]), int(p[5])
    out, a0, b0 = [], ab, bb
    for s in range(len(trace) // 2):
        a1 = min((ab // tspace + s + 1) * tspace, ae)
        out.append((a0, a1, b0, b0 + trace[2 * s + 1]))
        a0, b0 = a1, b0 + trace[2 * s + 1]
    return out


def test_band_centre_formula():
    # integer form of round(i (blen - alen) / alen), halves up, for both signs of blen - alen
    for alen, blen in ((10, 13), (10, 7), (7, 7), (1, 9), (300, 299), (33, 100)):
        for i in range(alen + 1):
            assert tc.centre(i, alen, blen) == int(np.floor(i * (blen - alen) / alen + 0.5 + 1e-12))
        assert tc.centre(0, alen, blen) == 0 and tc.centre(alen, alen, blen) == blen - alen


def test_hand_cases_trace_properties(hand):
    contigs, reads, cases, res = hand
    for (name, p, expect), (st, w, trace, diffs) in zip(cases, res):
        A, B = tc.stretches(contigs, reads, p)
        assert st == tc.OK and w == 128, name
        if expect is not None:
            assert st == expect
        assert len(trace) == 2 * tc.n_segments(p[3], p[4], TSPACE), name
        assert sum(trace[1::2]) == len(B), name
        assert sum(trace[0::2]) == diffs == tc.levenshtein(A, B), name       # OK and untouched: the band held an optimal path
        for a0, a1, b0, b1 in _segments(p, trace, TSPACE):
            seg_a, seg_b = contigs[p[0]][a0:a1], (tc.revcomp(reads[p[1]]) if p[2] else reads[p[1]])[b0:b1]
            d = trace[2 * ((a0 // TSPACE) - (p[3] // TSPACE))]
            assert d >= tc.levenshtein(seg_a, seg_b), name                     # hinge_consensus_run sizes its waves from the recorded diffs
    names = [c[0] for c in cases]
    assert res[names.index("identical")][3] == 0 and res[names.index("alen_1")][2] == [0, 1]
    assert res[names.index("one_block")][2][1] == cases[names.index("one_block")][1][6] - cases[names.index("one_block")][1][5]


def test_indel_cases_widen_and_drop():
    contigs, reads, pl = tc.indel_cases()
    res = tc.model_run(contigs, reads, pl, TSPACE, band=16, band_max=1024)
    for x in (0, 1):
        st, w, trace, diffs = res[x]
        assert st == tc.OK and w in (32, 64) and diffs == 30
        assert sum(trace[1::2]) == len(reads[pl[x][1]])
    assert res[2][:2] == (tc.OK, 16) and res[4][:2] == (tc.OK, 16)
    assert res[3][:3] == (tc.NO_PATH, 1024, None)                 # |blen - alen| = 1300 > W_MAX
    assert res[5][0] == tc.WIDE and res[5][1] == 512 and res[5][2] is None
    # the same placements from the default W: the answers of a round do not depend on where the rounds started
    res128 = tc.model_run(contigs, reads, pl, TSPACE)
    assert [r[0] for r in res128] == [r[0] for r in res] and res128[5][1] == 512 and res128[0][1] == 128


def test_two_byte_traces_hold_wide_segments():
    contigs, reads, pl = tc.indel_cases()
    st, w, trace, diffs = tc.model_run(contigs, reads, [pl[5]], 200)[0]
    assert st == tc.OK and w == 512 and max(trace) > 255 and sum(trace[1::2]) == len(reads[pl[5][1]])


def test_paf_strand_arithmetic(tmp_path):
    """A `-` line's query coordinates are on the read's forward strand: bbpos = qlen - qend, bepos = qlen - qstart, and the
    stretch they name in the complemented frame is the reverse complement of the forward stretch."""
    rng = np.random.default_rng(3)
    read = rng.integers(0, 4, size=500, dtype=np.uint8)
    qs, qe = 40, 460
    bb, be = len(read) - qe, len(read) - qs
    assert np.array_equal(tc.revcomp(read)[bb:be], tc.revcomp(read[qs:qe]))
    # write_paf with a target table of its own: query = read, target = contig
    p = str(tmp_path / "x.paf")
    formats.write_paf(p, np.asarray([500]), [0], [1], [1], [qs], [qe], [10], [430], rlen_b=np.asarray([900, 1000]))
    f = open(p).read().split("\t")
    assert f[0] == "synth/1/0_500" and f[1:5] == ["500", "40", "460", "-"] and f[5] == "synth/2/0_1000" and f[6:9] == ["1000", "10", "430"]


def test_correct_head_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    seqs = ["".join("ACGT"[v] for v in rng.integers(0, 4, size=n)) for n in (200, 12, 75, 30, 29)]
    src = tmp_path / "in.fasta"
    with open(src, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">contig%d some words\n" % i)
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + "\n")
    r = subprocess.run([HINGE, "correct-head", str(src), str(tmp_path / "out.fasta"), str(tmp_path / "map.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    lines = open(tmp_path / "map.txt").read().splitlines()
    assert lines == ["contig0 some words\tm000_000/1/0_200", "contig1 some words\tDeleted", "contig2 some words\tm000_000/3/0_75",
                     "contig3 some words\tm000_000/4/0_30", "contig4 some words\tDeleted"]
    out = open(tmp_path / "out.fasta").read().splitlines()
    heads = [l for l in out if l.startswith(">")]
    assert heads == [">m000_000/1/0_200", ">m000_000/3/0_75", ">m000_000/4/0_30"]
    assert all(len(l) <= 60 for l in out if not l.startswith(">"))
    bases = formats.read_fasta_bases(str(tmp_path / "out.fasta"))
    assert ["".join("ACGT"[v] for v in b) for b in bases] == [seqs[0], seqs[2], seqs[3]]
    # and the DB made of it keeps them
    assert formats.fasta2db(str(tmp_path / "out.fasta"), str(tmp_path / "d")) == 3


def test_correct_head_usage_and_errors(tmp_path):
    r = subprocess.run([HINGE, "correct-head", "only_one"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"usage: hinge correct-head" in r.stderr
    r = subprocess.run([HINGE, "correct-head", str(tmp_path / "missing.fasta"), str(tmp_path / "o.fasta"), str(tmp_path / "m.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"Traceback" not in r.stderr


def _tiny_dbs(wd):
    rng = np.random.default_rng(8)
    contig = rng.integers(0, 4, size=400, dtype=np.uint8)
    read = contig[50:350].copy()
    formats.write_db(os.path.join(wd, "draft"), np.asarray([400], np.int32), bases=[contig])
    formats.write_db(os.path.join(wd, "reads"), np.asarray([300], np.int32), bases=[read])


def _paf2las(wd, paf_text, *opts, env=None):
    with open(os.path.join(wd, "x.paf"), "w") as f:
        f.write(paf_text)
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([HINGE, "paf2las", "draft", "reads", "x.paf", "out.las"] + list(opts), cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


GOOD = "synth/1/0_300\t300\t0\t300\t+\tsynth/1/0_400\t400\t50\t350\t300\t300\t255\n"


def test_paf2las_usage_and_input_errors(tmp_path):
    wd = str(tmp_path)
    _tiny_dbs(wd)
    r = subprocess.run([HINGE, "paf2las", "draft", "reads"], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"usage: paf2las" in r.stderr
    r = _paf2las(wd, GOOD, "--no-such-option")
    assert r.returncode == 1 and b"unknown option" in r.stderr
    r = subprocess.run([HINGE, "paf2las", "nodb", "reads", "x.paf", "out.las"], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"Could not open database" in r.stderr
    # input errors name the line (all of them are found before the GPU is needed)
    for text, what in ((GOOD + GOOD.replace("synth/1/0_400", "synth/7/0_400"), b"line 2: unknown contig"),
                       (GOOD.replace("synth/1/0_300", "nobody"), b"line 1: unknown read"),
                       (GOOD.replace("\t300\t0\t300\t", "\t301\t0\t300\t"), b"line 1: the query length"),
                       (GOOD.replace("\t400\t50\t350\t", "\t400\t50\t450\t"), b"line 1: coordinates outside"),
                       ("a\tb\tc\n", b"line 1: fewer than 9 columns")):
        r = _paf2las(wd, text)
        assert r.returncode == 1 and what in r.stderr, r.stderr
    # names through a FASTA's record order: an unknown name there is an error too
    with open(os.path.join(wd, "names.fasta"), "w") as f:
        f.write(">ctgA extra\nACGT\n")
    r = _paf2las(wd, GOOD, "--draft-names", "names.fasta")
    assert r.returncode == 1 and b"line 1: unknown contig" in r.stderr


def test_paf2las_without_gpu_fails_like_the_other_executables(tmp_path):
    wd = str(tmp_path)
    _tiny_dbs(wd)
    r = _paf2las(wd, GOOD, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert r.returncode == 2 and b"paf2las: no usable GPU" in r.stderr
