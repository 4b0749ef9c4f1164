"""A hand-made part whose hinge decision needs sort keys that span 2^20 or more, shared by tests/test_wide_keys.py (the model's
answer, on the CPU) and tests/test_wide_keys_gpu.py (the kernels').  TEST INFRASTRUCTURE.

The replay of std::sort behind k_hinge_call packs key and element into one 32-bit word and therefore takes keys that span less
than 2^20; the LEAN instance has no other form and hands such an annotation to the serial exact kernel.  Pile-up keys are sums of
two span lengths, supporter keys positions on the read: both get there on a read of 1.1 Mb or more.

The part (positions exceed 65 535: it goes through set_reads / set_pileups, the unpacked route):
  read 0             2 400 000 bases; reads 1..S 20 000 bases each
  read 0's pile-up   30 overlaps over [0, 2 400 000]                         the floor of its coverage
                     15 more over [0, 60 000 + 977 k], k = 0..14             the gate sees 15 more at the head than at the tail
                     S supporters [start_k, 2 000 020] against read k, uncomplemented: distinct multiples of 40 in
                     [200 000, 1 900 000), the smallest 200 000, the largest 1 814 400 - the coverage drops by S at 2 000 020
  reads k >= 1       30 overlaps over their whole length
Shape "hinge": the supporters' B spans are [0, 15 000] - no left overhang, the scan stops "unbridged" at its seventh element: a
hinge.  Shape "bridged": B spans [1000, 15 000] - a left overhang of 680 > theta, every supporter takes the scan's third branch,
which never finds 8 other ends inside 200 bases (they are 40 apart and distinct), so the scan runs to its end: bridged, NO hinge.
A route that drops the annotation leaves 0 on the first shape, one that writes 1 blindly fails the second."""
import ctypes

import numpy as np

import spec_model

RLEN0, RLEN = 2400000, 20000
ANNO = (2000000, -1)
START_LO, START_HI = 200000, 1814400      # the supporter sort spans 1 614 400 >= 2^20
SHAPES = ("hinge", "bridged")
ip = ctypes.POINTER(ctypes.c_int)


def supporter_starts(S):
    """S distinct multiples of 40 in [200 000, 1 900 000), in no particular order by supporter."""
    rng = np.random.default_rng(2024 + S)
    inner = rng.choice(np.arange(START_LO // 40 + 1, START_HI // 40), size=S - 2, replace=False) * 40
    st = np.concatenate([[START_LO, START_HI], inner]).astype(np.int64)
    rng.shuffle(st)
    assert len(set(st.tolist())) == S and st.min() == START_LO and st.max() == START_HI and not (st % 40).any()
    return st


def make_part(S, shape):
    """(rlen, row_ptr, a_span, b_span, b_flag) of reads 0..S, every pile-up in the order of its B reads."""
    assert shape in SHAPES
    rlen = np.array([RLEN0] + [RLEN] * S, np.int32)
    start = supporter_starts(S)
    rows = []           # (aread, bread, ab, ae, bb, be)
    for j in range(30):
        rows.append((0, 1 + j % S, 0, RLEN0, 0, RLEN))
    for k in range(15):
        rows.append((0, 1 + (7 * k) % S, 0, 60000 + 977 * k, 0, RLEN))
    for k in range(1, S + 1):
        rows.append((0, k, int(start[k - 1]), ANNO[0] + 20, 0 if shape == "hinge" else 1000, 15000))
    for k in range(1, S + 1):
        for j in range(30):
            rows.append((k, 1 + (k + j) % S, 0, RLEN, 0, RLEN))
    rows.sort(key=lambda r: (r[0], r[1]))      # stable: a .las file's order (A read, then B read)
    rows = np.array(rows, np.int64)
    assert not (rows[:, 0] == rows[:, 1]).any()
    row_ptr = np.searchsorted(rows[:, 0], np.arange(S + 2)).astype(np.int64)
    a_span = np.ascontiguousarray(rows[:, 2:4], np.int32)
    b_span = np.ascontiguousarray(rows[:, 4:6], np.int32)
    b_flag = np.ascontiguousarray(rows[:, 1], np.uint32)      # bread | comp << 31: uncomplemented
    return rlen, row_ptr, a_span, b_span, b_flag


def model_params(fp):
    return dict(CUT=fp.cut_off, EC=fp.est_cov, TH=fp.theta, CF=fp.coverage_fraction, MINRA=fp.min_repeat_annotation, MAXRA=fp.max_repeat_annotation,
                GAP=fp.repeat_annotation_gap, NHR=fp.no_hinge_region, SUP=fp.hinge_min_support, PIL=fp.hinge_bin_pileup, UNB=fp.hinge_unbridged,
                TOL=fp.hinge_tolerance, BIN=2 * fp.hinge_tolerance, USE_QV=fp.use_qv_mask, USE_COV=fp.use_coverage_mask)


def model(part, fp, oracle_lib):
    """tests/spec_model.py on the part, std::sort's order from the oracle library (as in tests/test_spec_model.py).  Returns a dict:
    min_cov, mask / cmask [n, 2], annotations and hinges per read, gated per read, and the keys of every sort the hinge calling ran:
    sorts = [keys] in call order - a read's pile-up (length sums), then the supporters of each of its scanned annotations."""
    rlen, row_ptr, a_span, b_span, b_flag = part
    n = len(rlen)
    sorts = []

    def sort_perm(keys, descending):
        keys = np.ascontiguousarray(keys, np.int32)
        sorts.append(keys.copy())
        perm = np.zeros(max(len(keys), 1), np.int32)
        oracle_lib.oracle_sort_perm(len(keys), keys.ctypes.data_as(ip), 0 if descending else 1, perm.ctypes.data_as(ip))
        return perm[:len(keys)].tolist()

    P = model_params(fp)
    maskvec = {i: (0, 0) for i in range(n)}
    min_cov, cmask, annos, hinges, cov0 = spec_model.filter_part(rlen, None, row_ptr, a_span, b_span, b_flag, 0, n - 1, maskvec, fp.min_cov, P, sort_perm)
    gated = {i: bool(annos[i]) and spec_model.gate_skips(cov0[i], maskvec[i], P) for i in range(n)}
    return dict(min_cov=min_cov, mask=np.array([maskvec[i] for i in range(n)], np.int32), cmask=np.array([cmask[i] for i in range(n)], np.int32),
                annos=annos, hinges=hinges, gated=gated, sorts=sorts)


def span(keys):
    return int(keys.max()) - int(keys.min())
