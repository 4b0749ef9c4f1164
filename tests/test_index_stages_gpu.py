"""`hinge overlap` and `hinge seed` on the device-built index against the host-built one: hinge_overlap_run on
overlap_common.edge_reads() and hinge_seed_run on cns_tiny, each in a fresh child process per setting of HINGE_INDEX_DEVICE (the
switch is read from the environment; tests/index_stage_child.py) - every output array and every stats slot except the
microseconds is equal, and hinge_index_last_stats names the path that built every block's index."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _stage(stage, tmp_path):
    got = {}
    for dev in ("1", "0"):
        out = os.path.join(str(tmp_path), "%s_%s.npz" % (stage, dev))
        env = dict(os.environ, HINGE_INDEX_DEVICE=dev)
        for name in ("HINGE_INDEX_SCRATCH_MB", "HINGE_INDEX_SCRATCH_BYTES"):
            env.pop(name, None)
        r = subprocess.run([sys.executable, os.path.join(HERE, "index_stage_child.py"), stage, os.path.join(str(tmp_path), stage + dev), out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        z = np.load(out)
        got[dev] = ({k: z[k] for k in z.files if k != "stats"}, json.loads(str(z["stats"])))
    (a, sa), (b, sb) = got["1"], got["0"]
    assert sorted(a) == sorted(b) and len(a) >= 10
    for name in a:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
    assert sorted(sa) == sorted(sb)
    for label in sa:
        for x in (0, 1):
            for slot in sa[label][x]:
                if slot not in ("index_us", "device_builds", "host_builds", "passes", "scratch_bytes"):
                    assert sa[label][x][slot] == sb[label][x][slot], (label, slot)
    return sa, sb


def test_overlap_run_is_the_same_on_both_indexes(tmp_path):
    sa, sb = _stage("overlap", tmp_path)
    assert sa["three_blocks"][0]["blocks"] == 3
    assert (sa["three_blocks"][1]["device_builds"], sa["three_blocks"][1]["host_builds"]) == (3, 0)
    assert (sb["three_blocks"][1]["device_builds"], sb["three_blocks"][1]["host_builds"]) == (0, 3)
    assert (sa["defaults"][1]["device_builds"], sb["defaults"][1]["host_builds"]) == (1, 1)
    assert sa["max_occ2"][1]["dropped_codes"] == sa["max_occ2"][0]["dropped_codes"] > 0
    for s in (sa, sb):
        assert s["three_blocks"][1]["kept"] == s["three_blocks"][0]["entries"] and s["three_blocks"][1]["entries"] >= s["three_blocks"][1]["kept"] > 0


def test_seed_run_is_the_same_on_both_indexes(tmp_path):
    sa, sb = _stage("seed", tmp_path)
    for label in sa:
        assert (sa[label][1]["device_builds"], sa[label][1]["host_builds"]) == (1, 0)
        assert (sb[label][1]["device_builds"], sb[label][1]["host_builds"]) == (0, 1)
        assert sa[label][1]["kept"] == sa[label][0]["entries"] > 0 and sa[label][1]["dropped_codes"] == sa[label][0]["dropped_codes"]
    assert sa["n2_k10_occ1"][0]["dropped_codes"] > 0
