"""`hinge overlap --tile` end to end: the executable with and without the option, its .las read back through formats.read_las.

NOISY (reads of 2 .. 4 kb, one tile of 8 192 bases each): --tile 8192 writes the bytes the command writes without it.
LONG (reads of 30 .. 100 kb at 10 % errors per read, tests/test_overlap_tile_model.py): with --tile 8192 the .las holds at least as
many of the 3 152 pairs sharing >= 2 000 genome bases as without, loses at most 5 % of them to the alignment and the filters (the
tiled model finds all of them: the reference point), holds nothing from disjoint intervals, and its end points lie as close to the
generator's as the un-tiled run's (99th percentile, plus the 13 bases the un-tiled test adds to its own).
Measured on an MI355X: see DESIGN.md 3.14."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import overlap_common as oc
from hinge_amd import formats
from hinge_amd import synth_draft as sd
from test_overlap_model import NOISY
from test_overlap_tile_model import LONG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")
END_MARGIN = 13             # what tests/test_overlap_cli_gpu.py adds to its measured 99th percentile (END_P99 // 2)


def _overlap(wd, d, out, *args):
    os.makedirs(wd, exist_ok=True)
    if not os.path.exists(os.path.join(wd, "G.db")):
        formats.write_db(os.path.join(wd, "G"), d.rlen, bases=d.reads)
    r = subprocess.run([HINGE, "overlap", "G", out, "--min-len", "1000"] + list(args), cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    return formats.read_las(os.path.join(wd, out)), r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def long_runs(tmp_path_factory):
    d = sd.generate(LONG)
    wd = str(tmp_path_factory.mktemp("ovl_tile_long"))
    return d, _overlap(wd, d, "tiled.las", "--tile", "8192"), _overlap(wd, d, "plain.las")


def _rows(las):
    return {(int(q["aread"]), int(q["bread"]), int(q["flags"]) & 1): (int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in las.rec}


def _check_las(las, d, tspace=100):
    """What every .las of the command holds, whatever the data (the checks of tests/test_overlap_cli_gpu.py)."""
    rec = las.rec
    assert las.tspace == tspace and len(rec) > 0
    keys = [(int(q["aread"]), int(q["bread"]), int(q["flags"]) & 1, int(q["abpos"])) for q in rec]
    assert keys == sorted(keys) and len(set(k[:3] for k in keys)) == len(keys)                     # LAsort order, one record per (a, b, comp)
    have = set(k[:3] for k in keys)
    assert all((b, a, c) in have for a, b, c in have)                                              # (a, b, comp) iff (b, a, comp)
    tb = 1 if tspace <= 125 else 2
    rlen = d.rlen
    for i, q in enumerate(rec):
        t = np.asarray(las.trace[las.trace_off[i]:las.trace_off[i + 1]])
        assert len(t) == int(q["tlen"]) * tb
        v = t.astype(np.int64) if tb == 1 else t.view("<u2").astype(np.int64)
        ab, ae, bb, be = int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])
        assert 0 <= ab < ae <= rlen[int(q["aread"])] and 0 <= bb < be <= rlen[int(q["bread"])]
        assert int(v[1::2].sum()) == be - bb                                                       # the B advances
        assert len(v) // 2 == (ae - 1) // tspace - ab // tspace + 1                                # the segments of [abpos, aepos)
        assert int(v[0::2].sum()) == int(q["diffs"])


def _p99(d, got):
    truth = oc.rec_rows(d)
    dev = np.asarray([abs(g - t) for x in got if x in truth for g, t in zip(got[x], truth[x])], np.int64)
    return dev, {p: int(np.percentile(dev, p)) for p in (50, 90, 99, 100)}


def test_one_tile_reads_give_the_same_bytes(tmp_path):
    d = sd.generate(NOISY)
    wd = str(tmp_path)
    las, out, err = _overlap(wd, d, "plain.las")
    tlas, tout, terr = _overlap(wd, d, "tiled.las", "--tile", "8192")
    assert len(las.rec) > 1000
    assert filecmp.cmp(os.path.join(wd, "plain.las"), os.path.join(wd, "tiled.las"), shallow=False)
    assert "--tile 8192: %d tile(s), 0 job(s) of more than one" % (2 * len(d.reads)) in tout and "--tile" not in out
    env = dict(os.environ, HINGE_OVERLAP_TILE="8192")                                                # the default from the environment
    r = subprocess.run([HINGE, "overlap", "G", "env.las", "--min-len", "1000"], cwd=wd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"--tile 8192:" in r.stdout
    assert filecmp.cmp(os.path.join(wd, "plain.las"), os.path.join(wd, "env.las"), shallow=False)


def test_long_reads_recall_and_end_points(long_runs):
    """Measured on an MI355X: with --tile 8192 3 242 candidates, 3 202 records, 3 152 of the 3 152 pairs (without: 3 161 candidates and
    15 mirrored, 3 170 records, 3 148 pairs); nothing lost, nothing from disjoint intervals.  End points over 12 800 / 12 680 of them:
    median 1 / 5, 90th percentile 6 / 56, 99th 16 / 121 - 1 457 of the tiled run's records were extended by their second run (the box
    along a candidate's diagonal cuts an end whose own diagonal lies on its far side).  Before that second run the
    tiled figures were 5 / 60 / 142."""
    d, (tlas, tout, terr), (plas, pout, perr) = long_runs
    print(tout.strip()); print(terr.strip()); print(pout.strip()); print(perr.strip())
    _check_las(tlas, d)
    got, plain = _rows(tlas), _rows(plas)
    want = oc.truth_pairs(d, 2_000)
    assert len(want) == 3152
    lost = sorted(want - set(got))                                                                  # (the tiled model finds all of `want`)
    print("pairs >= 2000: %d; .las with --tile: %d of them, without: %d; lost to the alignment or the filters: %d %s" % (
        len(want), len(want & set(got)), len(want & set(plain)), len(lost), lost[:20]))
    assert len(want & set(got)) >= len(want & set(plain))
    assert len(lost) <= 0.05 * len(want)
    assert not [x for x in got if oc.shared_bases(d, x[0], x[1]) <= 0]
    dev, pct = _p99(d, got)
    pdev, ppct = _p99(d, plain)
    print("end point deviation with --tile over %d end points: %s, mean %.2f; without over %d: %s, mean %.2f" % (len(dev), pct, float(dev.mean()), len(pdev), ppct, float(pdev.mean())))
    assert len(dev) >= 4 * 1000
    assert "--tile 8192: " in tout and " %d job(s) of more than one" % (2 * len(d.reads)) in tout
    assert pct[99] <= ppct[99] + END_MARGIN


def test_bad_tiles_print_the_usage():
    for args in (["--tile", "100"], ["--tile", "16384"], ["--tile", "8192", "--max-stretches", "2"], ["--tile", "0"], ["--tile"]):
        r = subprocess.run([HINGE, "overlap", "G", "out.las"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"usage: overlap" in r.stderr and b"--tile T" in r.stderr, args
