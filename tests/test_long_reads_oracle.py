"""The `ultra_long` data set (reads up to 1.3 Mb) on the CPU oracle: `hinge filter` answers it, and it is a data set on which
the long-read tier of the HIP path (hinge_amd/csrc/filter_long_kernels.h) has something to do - reads whose coverage profile
does not fit the mask/annotate kernel's LDS slot, some longer than a whole workgroup's LDS, with annotations and hinges on them."""
import os

import numpy as np

from conftest import clone_dataset, run_in

RESO, CUT_OFF, KCAP_LDS_MAX = 40, 300, 5120   # the shipped reso, nominal.ini's cut_off, bins of a wavefront's LDS slot


def long_read_ids(rlen):
    """Reads whose bins exceed the LDS slot of k_mask_annotate (what hinge_capi.hip lists for the long-read tier)."""
    rlen = np.asarray(rlen, np.int64)
    return np.nonzero((rlen + CUT_OFF) // RESO + 4 > KCAP_LDS_MAX)[0]


def entries_on(path, ids):
    """(position, type) pairs that a .repeat.txt / .hinges.txt file holds for the reads in `ids`."""
    ids = set(int(i) for i in ids)
    n = 0
    for l in open(path):
        t = l.split()
        if t and int(t[0]) in ids:
            n += (len(t) - 1) // 2
    return n


def test_ultra_long_config_is_answered_by_the_oracle_and_not_vacuous(datasets, oracle_lib, tmp_path):
    from hinge_amd import formats, synth
    assert "ultra_long" in synth.CONFIGS
    src, d = datasets("ultra_long")
    wd = clone_dataset(src, str(tmp_path / "oracle"))
    assert run_in(wd, oracle_lib.oracle_filter, b"G", b"G.las", 0, b"G", b"nominal.ini", b"") == 0
    rlen = formats.read_db_index(os.path.join(wd, "G"))["rlen"]
    ids = long_read_ids(rlen)
    assert len(ids) >= 20, "reads beyond the LDS slot: %d" % len(ids)
    assert int(np.sum(np.asarray(rlen) > 819200)) >= 2, "reads beyond a whole workgroup's LDS"
    assert entries_on(os.path.join(wd, "G.repeat.txt"), ids) >= 1
    assert entries_on(os.path.join(wd, "G.hinges.txt"), ids) >= 1
    recs = formats.read_las(os.path.join(wd, "G.las"))
    pile = formats.pileups_from_las(recs, rlen)
    assert int(np.max(np.diff(pile.row_ptr))) < 65536
