"""`hinge overlap --tile T --tile-stretches S` end to end: the executable on a set of long reads with a two-copy repeat (LONGREP of
tests/test_overlap_tile_multi_model.py: 66 reads of 30 .. 60 kb, 10 % errors per read, a 1 500-base copy 20 kb away), its .las read
back through formats.read_las and held to the generator's ground truth, beside the two options it joins.

Three runs, all with --min-len 800: `--tile 8192 --tile-stretches 3`, `--tile 8192` and `--max-stretches 3`.  Every one of the 334
expected stretches - 188 cross alignments of the two copies, 146 main overlaps beside them - has a record of its key on the expected
copy in the first run (the criterion of tests/test_overlap_multi_cli_gpu.py); the cross stretches' end points lie as close to the
generator's as those of the `--max-stretches 3` run on the stretches it finds, within 15 bases.
Equivalent runs: `--tile-stretches 1` writes `--tile`'s bytes; on reads of one tile `--tile 8192 --tile-stretches 3` writes
`--max-stretches 3`'s.  Downstream: filter, maximal and layout on the combined .las against the CPU oracle, byte for byte."""
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
from test_overlap_multi_cli_gpu import HINGE, _check_order_and_pairs, _overlap, _recs
from test_overlap_multi_model import ON_TOL
from test_overlap_tile_multi_model import LONGREP

pytestmark = pytest.mark.gpu

END_MARGIN = 15             # bases over the `--max-stretches 3` run's own 99th percentile (the margin of DESIGN.md 3.11)


def _on_expected(las, want):
    """Per expected stretch the deviations of its best record's four end points, or None without a record on it."""
    by_key = {}
    for r in _recs(las):
        by_key.setdefault(r[:3], []).append(r[3:])
    out = []
    for w in want:
        on = [q for q in by_key.get(w[:3], []) if abs((q[2] - q[0]) - (w[6] - w[4])) < ON_TOL and min(q[1], w[5]) - max(q[0], w[4]) > 0]
        if not on:
            out.append(None)
            continue
        best = min(on, key=lambda q: sum(abs(g - t) for g, t in zip(q, w[4:])))
        out.append([abs(g - t) for g, t in zip(best, w[4:])])
    return out


@pytest.fixture(scope="module")
def longrep(tmp_path_factory):
    d = sd.generate(LONGREP)
    wd = str(tmp_path_factory.mktemp("ovl_longrep"))
    runs = {}
    for name, args in (("both", ("--tile", "8192", "--tile-stretches", "3")), ("tile", ("--tile", "8192")), ("whole", ("--max-stretches", "3"))):
        runs[name] = _overlap(os.path.join(wd, name), d, *args, min_len="800")
    return d, wd, runs, om.expected_stretches(d)


def test_every_expected_stretch_has_its_record(longrep):
    d, wd, runs, want = longrep
    assert len(want) == 334 and sum(1 for w in want if w[3] == "cross") == 188
    found = {}
    for name, (las, out, err) in runs.items():
        print(name, out.strip()); print(name, err.strip())
        _check_order_and_pairs(las, d)
        found[name] = _on_expected(las, want)
        missing = [w for w, f in zip(want, found[name]) if f is None]
        print("%s: %d records; expected stretches without a record: %d (%d cross) %s" % (name, len(las.rec), len(missing), sum(1 for w in missing if w[3] == "cross"), missing[:3]))
    assert "--tile-stretches 3:" in runs["both"][1] and "--tile 8192:" in runs["both"][1]           # both summary lines
    assert not [w for w, f in zip(want, found["both"]) if f is None]
    # the end points of the cross stretches, against the whole-read run's own on the ones it finds
    pct = {}
    for name in runs:
        dev = np.asarray([v for w, f in zip(want, found[name]) if f is not None and w[3] == "cross" for v in f] or [0])
        pct[name] = {p: float(np.percentile(dev, p)) for p in (50, 90, 99, 100)}
        print("%s: cross stretches' end point deviation over %d end points: %s" % (name, len(dev), pct[name]))
    assert pct["both"][99] <= pct["whole"][99] + END_MARGIN


def test_one_round_writes_the_tiled_bytes(tmp_path):
    d = sd.generate(NOISY)
    _overlap(str(tmp_path / "one"), d, "--tile", "1024", "--tile-stretches", "1")
    _overlap(str(tmp_path / "tile"), d, "--tile", "1024")
    assert filecmp.cmp(str(tmp_path / "one" / "out.las"), str(tmp_path / "tile" / "out.las"), shallow=False)
    assert os.path.getsize(str(tmp_path / "tile" / "out.las")) > 100_000


def test_one_tile_reads_write_the_whole_read_bytes(tmp_path):
    d = sd.generate(NOISY)
    assert max(d.rlen) <= 8192
    las, out, err = _overlap(str(tmp_path / "both"), d, "--tile", "8192", "--tile-stretches", "3")
    _overlap(str(tmp_path / "whole"), d, "--max-stretches", "3")
    assert filecmp.cmp(str(tmp_path / "both" / "out.las"), str(tmp_path / "whole" / "out.las"), shallow=False)
    assert "--tile-stretches 3:" in out
    # both defaults from the environment
    wd = str(tmp_path / "env")
    os.makedirs(wd)
    formats.write_db(os.path.join(wd, "G"), d.rlen, bases=d.reads)
    r = subprocess.run([HINGE, "overlap", "G", "out.las"], cwd=wd, env=dict(os.environ, HINGE_OVERLAP_TILE="8192", HINGE_OVERLAP_TILE_STRETCHES="3"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and filecmp.cmp(os.path.join(wd, "out.las"), str(tmp_path / "both" / "out.las"), shallow=False)


def test_bad_combinations_print_the_usage():
    for args in (("--tile-stretches", "2"), ("--tile-stretches", "1"), ("--tile", "8192", "--tile-stretches", "2", "--max-stretches", "2"), ("--tile", "8192", "--tile-stretches", "0"),
                 ("--tile", "8192", "--tile-stretches", "9"), ("--tile", "8192", "--tile-stretches", "x"), ("--tile", "8192", "--max-stretches", "2")):
        r = subprocess.run([HINGE, "overlap", "G", "out.las"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"usage: overlap" in r.stderr and b"--tile-stretches" in r.stderr, args


def test_downstream_stages_match_the_oracle(longrep, oracle_lib, tmp_path):
    d, wd, runs, want = longrep
    dirs = []
    for side in ("oracle", "hip"):
        dst = str(tmp_path / side)
        os.makedirs(dst)
        formats.write_db(os.path.join(dst, "G"), d.rlen, bases=d.reads)
        shutil.copy(os.path.join(wd, "both", "out.las"), os.path.join(dst, "G.las"))
        write_ini(os.path.join(dst, "v.ini"))
        dirs.append(dst)
    assert _oracle(oracle_lib, dirs[0], False, "v.ini") == [0, 0, 0]
    assert _cli(dirs[1], False, "v.ini") == [0, 0, 0]
    bad = [f for f in FILES if not filecmp.cmp(os.path.join(dirs[0], f), os.path.join(dirs[1], f), shallow=False)]
    assert not bad, "differs from the oracle: %s" % bad
