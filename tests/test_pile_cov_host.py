"""The ingest's per-read coverage sums without a GPU: capi.pile_cov (numpy) and LasPart::finish_facts (C++), and the estimate
hinge_set_pile_cov works out from them on the host (hinge_amd/csrc/pile_cov_host.h), against a brute-force coverage profile per
read (histogram of begin and end events, prefix sum, sum) and against the CPU oracle's median.  The C++ side runs as a
stand-alone program (tests/pile_cov_host/driver.cpp) built under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RESO = 40


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("pile_cov_host") / "driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(HERE, "pile_cov_host", "driver.cpp"), "-lz"])
    return exe


def run_driver(exe, tmp_path, rlen, row_ptr, a_span, r_begin=0, r_end=None):
    n = len(rlen)
    r_end = n - 1 if r_end is None else r_end
    a_span = np.ascontiguousarray(a_span, dtype=np.int32).reshape(-1, 2)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([n, r_begin, r_end, len(a_span)], np.int64).tofile(f)
        np.ascontiguousarray(rlen, dtype=np.int32).tofile(f)
        np.ascontiguousarray(row_ptr, dtype=np.int64).tofile(f)
        a_span.tofile(f)
    r = subprocess.run([exe, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    raw = open(dst, "rb").read()
    head = np.frombuffer(raw[:48], np.int64)
    nr = int(head[0])
    bins = np.frombuffer(raw[48:48 + 4 * nr], np.int32)
    sums = np.frombuffer(raw[48 + 4 * nr:48 + 8 * nr], np.int32)
    return dict(eligible=bool(head[1]), cov_est=int(head[2]), n_long=int(head[3]), total_cov=int(head[4]), num_slot=int(head[5])), bins, sums


def brute_profile_sum(spans, reso=RESO):
    """profileCoverage of one pile-up with cut_off 0 (LAInterface.cpp:4298-4320): an overlap covers bin k from the first k with
    abpos < k * reso to the last with aepos >= k * reso; the profile has max coordinate / reso + 2 bins.  Returns (bins, sum)."""
    if len(spans) == 0:
        return 0, 0
    K = int(np.max(spans)) // reso + 2
    ev = np.zeros(K + 1, np.int64)
    for ab, ae in spans:
        ev[int(ab) // reso + 1] += 1          # first bin k with ab < k * reso
        ev[int(ae) // reso + 1] -= 1          # first bin k with ae < k * reso: no longer covered
    prof = np.cumsum(ev)[:K]
    return K, int(prof.sum())


def brute(rlen, row_ptr, a_span):
    a_span = np.asarray(a_span, np.int64).reshape(-1, 2)
    nr = len(row_ptr) - 1
    bins, sums = np.zeros(nr, np.int64), np.zeros(nr, np.int64)
    for i in range(nr):
        sp = a_span[row_ptr[i]:row_ptr[i + 1]]
        ok = len(sp) < 65536 and (len(sp) == 0 or (sp.min() >= 0 and sp.max() <= rlen[i]))
        if not ok:
            bins[i] = -1
            continue
        bins[i], sums[i] = brute_profile_sum(sp)
    return bins, sums


def brute_estimate(rlen, bins, sums):
    """filter.cpp:642-678 on the per-read numbers: mean = sum / max(1, bins) for reads >= 5000 bp, the element of rank n / 2."""
    sel = np.asarray(rlen) >= 5000
    means = np.sort(sums[sel] // np.maximum(1, bins[sel]))          # (sums >= 0 here: floor == C division)
    n = len(means)
    return dict(eligible=bool(np.all(bins >= 0)), cov_est=int(means[n // 2]) if n else 0, n_long=n,
                total_cov=int(sums[sel].sum()), num_slot=int(bins[sel].sum()))


def random_part(rng, n_reads, mean_pile, rlen_lo=1000, rlen_hi=20000):
    rlen = rng.integers(rlen_lo, rlen_hi, n_reads).astype(np.int32)
    counts = rng.poisson(mean_pile, n_reads)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    a_of = np.repeat(np.arange(n_reads), counts)
    ab = (rng.random(len(a_of)) * rlen[a_of]).astype(np.int32)
    ae = ab + (rng.random(len(a_of)) * (rlen[a_of] - ab + 1)).astype(np.int32)
    return rlen, row_ptr, np.stack([ab, np.minimum(ae, rlen[a_of])], axis=1).astype(np.int32)


def check(driver, tmp_path, rlen, row_ptr, a_span):
    from hinge_amd import capi
    want_bins, want_sums = brute(rlen, row_ptr, a_span)
    got_py = capi.pile_cov(row_ptr, a_span, rlen, RESO)
    assert got_py.dtype == np.int32
    assert np.array_equal(capi.pile_bins(row_ptr, a_span, rlen, RESO), want_bins)
    assert np.array_equal(got_py, want_sums)
    est, bins, sums = run_driver(driver, tmp_path, rlen, row_ptr, a_span)
    assert np.array_equal(bins, want_bins) and np.array_equal(sums, want_sums)
    if np.all(want_bins >= 0):
        assert est == brute_estimate(rlen, want_bins, want_sums)
    else:
        assert not est["eligible"]          # (the estimate of such a part is not used: the general kernel defines that read's mean)
    return est


@pytest.mark.parametrize("seed,n_reads,mean_pile", [(1, 300, 30), (2, 1500, 3), (3, 40, 400)])
def test_sums_on_random_spans(driver, tmp_path, seed, n_reads, mean_pile):
    rlen, row_ptr, a_span = random_part(np.random.default_rng(seed), n_reads, mean_pile)
    est = check(driver, tmp_path, rlen, row_ptr, a_span)
    assert est["eligible"] and est["n_long"] > 0 and est["total_cov"] > 0


def test_sums_on_the_edge_shapes(driver, tmp_path):
    # read 0: empty pile-up (K = 0); 1: 4 999 bp; 2: 5 000 bp; 3: an overlap with ab == ae, coordinates at 0 and at rlen, ends on bin borders
    rlen = np.array([7000, 4999, 5000, 8000], np.int32)
    piles = [[], [(0, 4999), (10, 4000)], [(0, 5000), (40, 80), (39, 41)], [(8000, 8000), (0, 0), (0, 8000), (120, 120), (7960, 8000), (79, 80)]]
    row_ptr = np.concatenate([[0], np.cumsum([len(p) for p in piles])]).astype(np.int64)
    a_span = np.array([s for p in piles for s in p], np.int32).reshape(-1, 2)
    est = check(driver, tmp_path, rlen, row_ptr, a_span)
    assert est["eligible"] and est["n_long"] == 3          # the 4 999 bp read is not in the median, the empty 7 000 bp one is (mean 0)
    # ... and a read with nbins = -1 (a coordinate behind its end; another one with a negative coordinate): sum 0, part not eligible
    for bad in [(100, 8001), (-1, 500)]:
        a2 = a_span.copy()
        a2[-1] = bad
        est = check(driver, tmp_path, rlen, row_ptr, a2)
        assert not est["eligible"]
        _, bins, sums = run_driver(driver, tmp_path, rlen, row_ptr, a2)
        assert bins[3] == -1 and sums[3] == 0 and bins[2] > 0


def test_part_without_a_long_read_and_part_inside_a_larger_table(driver, tmp_path):
    rlen, row_ptr, a_span = random_part(np.random.default_rng(5), 50, 20, rlen_lo=1000, rlen_hi=4999)
    est = check(driver, tmp_path, rlen, row_ptr, a_span)
    assert est["n_long"] == 0 and est["cov_est"] == 0 and est["eligible"]
    # a part that is a slice [r_begin, r_end] of the read table: the facts cover exactly its reads
    rlen, row_ptr, a_span = random_part(np.random.default_rng(6), 90, 25)
    lo, hi = 20, 69
    rp = np.clip(row_ptr, row_ptr[lo], row_ptr[hi + 1]) - row_ptr[lo]
    sp = a_span[row_ptr[lo]:row_ptr[hi + 1]]
    est, bins, sums = run_driver(driver, tmp_path, rlen, rp, sp, lo, hi)
    want_bins, want_sums = brute(rlen[lo:hi + 1], rp[lo:hi + 2], sp)
    assert np.array_equal(bins, want_bins) and np.array_equal(sums, want_sums)
    assert est == brute_estimate(rlen[lo:hi + 1], want_bins, want_sums)


@pytest.mark.parametrize("name", ["tiny", "chimera", "long_reads"])
def test_host_median_is_the_oracles(driver, datasets, oracle_lib, tmp_path, name):
    """The CPU oracle's own filter run on a data set (filter.cpp:642-678 restated): its median and its means are what the host
    derives from the ingest's sums."""
    import ctypes
    from conftest import clone_dataset, run_in
    from hinge_amd import formats
    src, _ = datasets(name)
    wd = clone_dataset(src, str(tmp_path / "oracle"))
    assert run_in(wd, oracle_lib.oracle_filter, b"G", b"G.las", 0, b"G", b"nominal.ini", b"") == 0
    oracle_lib.oracle_probe_means.restype = ctypes.c_long
    oracle_lib.oracle_probe_means.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_int)]
    cov_est = ctypes.c_int(0)
    cap = 1 << 20
    buf = np.zeros(cap, np.int32)
    n = int(oracle_lib.oracle_probe_means(buf.ctypes.data, cap, ctypes.byref(cov_est)))
    assert 0 < n <= cap
    rlen = formats.read_db_index(os.path.join(src, "G"))["rlen"]
    recs = formats.read_las(os.path.join(src, "G.las"))
    pile = formats.pileups_from_las(recs, rlen)
    r0, r1 = int(recs.rec["aread"][0]), int(recs.rec["aread"][-1])
    est, bins, sums = run_driver(driver, tmp_path, rlen, pile.row_ptr, pile.a_span, r0, r1)
    assert est["eligible"]
    assert est["n_long"] == n and est["cov_est"] == cov_est.value
    sel = np.asarray(rlen[r0:r1 + 1]) >= 5000
    assert np.array_equal(np.sort(sums[sel] // np.maximum(1, bins[sel])), np.sort(buf[:n]))
