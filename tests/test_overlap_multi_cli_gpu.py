"""`hinge overlap --max-stretches S` end to end: the executable on the synth_draft sets of tests/test_overlap_multi_model.py, its .las
read back through formats.read_las and held to the generator's ground truth.

Plasmid set (8 kb circular, noise-free; --step 16 --list 8192): with --max-stretches 2 the record set and every end point equal the
generator's 308; with no option the .las holds 272 of them, one per key.
NOISY set of test_overlap_model.py (no second stretch anywhere): --max-stretches 3 writes the bytes no option writes.
Repeat set (a 1 200-base copy 3 kb away, 10 % errors per read; --max-stretches 3 --min-len 800): every expected stretch - the
cross alignments of the two copies and the main overlaps beside them - has a record of its key on the expected copy, its end points
within END_TOL of the generator's copy position.
Downstream: filter, maximal and layout on the plasmid .las against the CPU oracle, byte for byte."""
import filecmp
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlap_multi_common as om
from conftest import write_ini
from hinge_amd import formats
from hinge_amd import synth_draft as sd
from test_cli_gpu import FILES, _cli, _oracle
from test_overlap_model import NOISY
from test_overlap_multi_model import ON_TOL, PLASMID, REPEAT, rec_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")
# |end point - the expected one| over all four end points of the repeat set's 272 expected stretches (position in the read = genome
# offset scaled by read length over interval length): see DESIGN.md 3.13 for the distribution; the 99th percentile plus half, the rule
# of test_overlap_cli_gpu.py
END_P99 = 30                # measured on an MI355X over 1 088 end points (146 cross stretches, 126 main ones): median 6, 90th percentile 17, 99th 30, largest 53, mean 8.09
END_TOL = END_P99 + END_P99 // 2


def _overlap(wd, d, *args, min_len="1000"):
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "G"), d.rlen, bases=d.reads)
    r = subprocess.run([HINGE, "overlap", "G", "out.las", "--min-len", min_len] + list(args), cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    return formats.read_las(os.path.join(wd, "out.las")), r.stdout.decode(), r.stderr.decode()


def _recs(las):
    return [(int(q["aread"]), int(q["bread"]), int(q["flags"]) & 1, int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in las.rec]


def _check_order_and_pairs(las, d):
    """The stated order; every stretch with both records, which cover the same bases."""
    recs = _recs(las)
    keys = [(r[0], r[1], r[2], r[3], r[5]) for r in recs]
    assert keys == sorted(keys) and len(recs) > 0
    have = {}
    for r in recs:
        have[r] = have.get(r, 0) + 1
    for r in recs:
        assert have.get(om.mirror_record(r, d.rlen), 0) == have[r], r                               # the mirror: the same stretch from read b
    for r in recs:
        assert 0 <= r[3] < r[4] <= d.rlen[r[0]] and 0 <= r[5] < r[6] <= d.rlen[r[1]]


@pytest.fixture(scope="module")
def plasmid(tmp_path_factory):
    d = sd.generate(PLASMID)
    wd = str(tmp_path_factory.mktemp("ovl_plasmid"))
    return (d, wd) + _overlap(wd, d, "--step", "16", "--list", "8192", "--max-stretches", "2")


def test_plasmid_set_equals_the_generator(plasmid, tmp_path):
    d, wd, las, out, err = plasmid
    print(out.strip())
    want = rec_set(d)
    assert len(want) == 308
    _check_order_and_pairs(las, d)
    assert sorted(_recs(las)) == want
    assert int(las.rec["diffs"].sum()) == 0
    assert "--max-stretches 2:" in out and "308 written" in out and "0 duplicates dropped" in out
    one, out1, err1 = _overlap(str(tmp_path), d, "--step", "16", "--list", "8192")
    got1 = _recs(one)
    assert len(got1) == 272 and set(got1) <= set(want) and len({r[:3] for r in got1}) == 272 and "--max-stretches" not in out1


def test_noisy_set_is_byte_identical_without_a_second_stretch(tmp_path):
    d = sd.generate(NOISY)
    _overlap(str(tmp_path / "three"), d, "--max-stretches", "3")
    _overlap(str(tmp_path / "none"), d)
    assert filecmp.cmp(str(tmp_path / "three" / "out.las"), str(tmp_path / "none" / "out.las"), shallow=False)
    assert os.path.getsize(str(tmp_path / "none" / "out.las")) > 100_000


def test_stretches_from_the_environment(plasmid, tmp_path):
    d, wd, las, out, err = plasmid
    formats.write_db(os.path.join(str(tmp_path), "G"), d.rlen, bases=d.reads)
    r = subprocess.run([HINGE, "overlap", "G", "out.las", "--step", "16", "--list", "8192"], cwd=str(tmp_path), env=dict(os.environ, HINGE_OVERLAP_MAX_STRETCHES="2"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and filecmp.cmp(os.path.join(str(tmp_path), "out.las"), os.path.join(wd, "out.las"), shallow=False)


def test_repeat_set_every_expected_stretch_has_its_record(tmp_path):
    d = sd.generate(REPEAT)
    las, out, err = _overlap(str(tmp_path), d, "--max-stretches", "3", min_len="800")
    print(out.strip()); print(err.strip())
    _check_order_and_pairs(las, d)
    by_key = {}
    for r in _recs(las):
        by_key.setdefault(r[:3], []).append(r[3:])
    want = om.expected_stretches(d)
    assert len(want) == 272
    missing, dev = [], []
    for w in want:
        on = [q for q in by_key.get(w[:3], []) if abs((q[2] - q[0]) - (w[6] - w[4])) < ON_TOL and min(q[1], w[5]) - max(q[0], w[4]) > 0]
        if not on:
            missing.append(w)
            continue
        best = min(on, key=lambda q: sum(abs(g - t) for g, t in zip(q, w[4:])))
        dev += [abs(g - t) for g, t in zip(best, w[4:])]
    dev = np.asarray(dev)
    pct = {p: float(np.percentile(dev, p)) for p in (50, 90, 99, 100)}
    kinds = {k: sum(1 for w in want if w[3] == k) for k in ("cross", "main")}
    print("expected stretches %s, missing %d %s; end point deviation over %d end points: %s, mean %.2f" % (kinds, len(missing), missing[:5], len(dev), pct, float(dev.mean())))
    assert not missing
    assert pct[99] <= END_TOL


def test_downstream_stages_match_the_oracle(plasmid, oracle_lib, tmp_path):
    d, wd, las, out, err = plasmid
    dirs = []
    for side in ("oracle", "hip"):
        dst = str(tmp_path / side)
        os.makedirs(dst)
        formats.write_db(os.path.join(dst, "G"), d.rlen, bases=d.reads)
        shutil.copy(os.path.join(wd, "out.las"), os.path.join(dst, "G.las"))
        write_ini(os.path.join(dst, "v.ini"))
        dirs.append(dst)
    assert _oracle(oracle_lib, dirs[0], False, "v.ini") == [0, 0, 0]
    assert _cli(dirs[1], False, "v.ini") == [0, 0, 0]
    bad = [f for f in FILES if not filecmp.cmp(os.path.join(dirs[0], f), os.path.join(dirs[1], f), shallow=False)]
    assert not bad, "differs from the oracle: %s" % bad


def test_bad_stretches_print_the_usage():
    for v in ("0", "9", "x"):
        r = subprocess.run([HINGE, "overlap", "G", "out.las", "--max-stretches", v], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"usage: overlap" in r.stderr and b"--max-stretches" in r.stderr, v
