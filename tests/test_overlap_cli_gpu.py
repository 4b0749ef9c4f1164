"""`hinge overlap` end to end: the executable on the two synth_draft sets of tests/test_overlap_model.py, its .las read back through
formats.read_las and held to the generator's ground truth.

Clean set (--step 16 --list 8192, see test_overlap_model.py): record set and end points equal the generator's.
Noisy set (the defaults): recall of the pairs sharing >= 2 000 genome bases against the model's, less the pairs hinge_trace_local
clipped out or the filters dropped (counted, printed, capped at 5 %); end points against the generator's within END_TOL."""
import os
import subprocess

import numpy as np
import pytest

import overlap_common as oc
from hinge_amd import formats
from hinge_amd import synth_draft as sd
from test_overlap_model import CLEAN, NOISY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")
# |end point - the generator's| over all four end points of the noisy set's records: see DESIGN.md 3.11 for the distribution; the
# 99th percentile plus half, the rule that gave `paf2las --ends local` its constants
END_P99 = 26                # measured on an MI355X over 5 136 end points: median 3, 90th percentile 14, 99th 26, largest 51, mean 5.35
END_TOL = END_P99 + END_P99 // 2


def _overlap(wd, d, *args):
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "G"), d.rlen, bases=d.reads)
    r = subprocess.run([HINGE, "overlap", "G", "out.las", "--min-len", "1000"] + list(args), cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    return formats.read_las(os.path.join(wd, "out.las")), r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    d = sd.generate(CLEAN)
    return (d,) + _overlap(str(tmp_path_factory.mktemp("ovl_clean")), d, "--step", "16", "--list", "8192")


@pytest.fixture(scope="module")
def noisy(tmp_path_factory):
    d = sd.generate(NOISY)
    return (d,) + _overlap(str(tmp_path_factory.mktemp("ovl_noisy")), d)


def _rows(las):
    return {(int(q["aread"]), int(q["bread"]), int(q["flags"]) & 1): (int(q["abpos"]), int(q["aepos"]), int(q["bbpos"]), int(q["bepos"])) for q in las.rec}


def _check_las(las, d, tspace=100):
    """What every .las of the command holds, whatever the data."""
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


def test_clean_set_equals_the_generator(clean):
    d, las, out, err = clean
    _check_las(las, d)
    got, want = _rows(las), oc.rec_rows(d)
    assert set(got) == set(want)
    assert all(got[x] == want[x] for x in want)
    assert int(las.rec["diffs"].sum()) == 0
    assert "%d written" % len(want) in out and "0 dropped for asymmetry" in out and "OVERFLOW" in err


def test_noisy_set_recall_and_end_points(noisy):
    d, las, out, err = noisy
    _check_las(las, d)
    print(out.strip()); print(err.strip())
    got = _rows(las)
    want = oc.truth_pairs(d, 2_000)
    rows, cnt, dg, rep, status, hits, st = oc.model_overlap(d.reads)
    sym, sdg, added = oc.symmetrise(rows, dg, d.rlen)
    model = {tuple(r[:3]) for r in sym}
    model_recall = len(want & model) / len(want)
    recall = len(want & set(got)) / len(want)
    lost = sorted((want & model) - set(got))                                                       # candidates of the model the .las does not hold
    print("pairs >= 2000: %d; model recall %.4f; .las recall %.4f; lost to the alignment or the filters: %d %s" % (len(want), model_recall, recall, len(lost), lost[:20]))
    assert len(lost) <= 0.05 * len(want)
    assert recall >= model_recall - len(lost) / len(want) - 1e-12
    # no record of pairs whose genome intervals are disjoint
    assert not [x for x in got if oc.shared_bases(d, x[0], x[1]) <= 0]
    # end points against the generator's
    truth = oc.rec_rows(d)
    dev = np.asarray([abs(g - t) for x in got if x in truth for g, t in zip(got[x], truth[x])], np.int64)
    pct = {p: int(np.percentile(dev, p)) for p in (50, 90, 99, 100)}
    print("end point deviation over %d end points: %s, mean %.2f" % (len(dev), pct, float(dev.mean())))
    assert len(dev) >= 4 * 1000
    assert pct[99] <= END_TOL


def test_tspace_200_gives_two_byte_traces(noisy, tmp_path):
    d = noisy[0]
    las, out, err = _overlap(str(tmp_path), d, "--tspace", "200")
    _check_las(las, d, 200)
    assert set(_rows(las)) == set(_rows(noisy[1]))


def test_bad_arguments_print_the_usage():
    for args in ([], ["G"], ["G", "out.las", "extra"], ["G", "out.las", "--k"], ["G", "out.las", "--step", "0"], ["G", "out.las", "--nope", "1"], ["G", "out.las", "--max-err", "2"]):
        r = subprocess.run([HINGE, "overlap"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"usage: overlap" in r.stderr, args
