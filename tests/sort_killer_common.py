"""Keys that drive libstdc++'s std::sort into its depth limit - the heap sort fallback - WITH ties, shared by the CPU test of
hinge_amd/csrc/stdsort_emul.h (tests/test_stdsort_emul.py) and the GPU tests of its device replay (tests/test_sort_fallback_gpu.py,
tests/test_sort_instances_gpu.py).  TEST INFRASTRUCTURE: a g++ harness around stdsort_emul.h and the real std::sort.

McIlroy's adversary ("A killer adversary for quicksort", 1999) run against this libstdc++'s std::sort gives n distinct values
val[0..n) that push the median-of-3 introsort past its 2 * floor(log2 n) levels.  The sort key is -(val // q), sorted DESCENDING
like compare_overlap: with q = 1 the comparisons are the adversary's own; with q >= 2 neighbouring values fall together, the walk
still runs out of depth, and where the heap part leaves the equal keys shows in the result - the only thing a replay of an
unstable sort is there for."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ip = ctypes.POINTER(ctypes.c_int)
P = lambda a: a.ctypes.data_as(ip)  # noqa: E731

HARNESS = r'''
#include <algorithm>
#include <vector>
#include "stdsort_emul.h"
extern "C" void emul_sort_perm(int n, const int* key, int desc, int* perm) {
    for (int i = 0; i < n; i++) perm[i] = i;
    hinge_sort::std_sort(perm, n, key, desc);
}
// McIlroy's "antiquicksort" adversary run against std::sort: produces keys that drive the
// median-of-3 introsort into its depth limit (the heapsort fallback).
static std::vector<int> val; static int nsolid, candidate, gas;
static bool adv_cmp(int x, int y) {
    if (val[x] == gas && val[y] == gas) { if (x == candidate) val[x] = nsolid++; else val[y] = nsolid++; }
    if (val[x] == gas) candidate = x; else if (val[y] == gas) candidate = y;
    return val[x] < val[y];
}
extern "C" void killer_keys(int n, int* out) {
    val.assign(n, 0); gas = n - 1; nsolid = 0; candidate = 0;
    std::vector<int> idx(n);
    for (int i = 0; i < n; i++) { idx[i] = i; val[i] = gas; }
    std::sort(idx.begin(), idx.end(), adv_cmp);
    for (int i = 0; i < n; i++) out[i] = val[i];
}
// The introsort loop of std::sort(idx, idx + n, key[x] > key[y]) walked with the replay's own median and partition; a segment of
// more than 16 elements that arrives with no depth left is what libstdc++ heap-sorts: its size goes to seg[] (at most cap of them
// are stored), the walk does not enter it.  Returns their number.
// *differs = 1 when the real std::sort leaves another order than std::__introsort_loop with the depth limit lifted followed by
// std::__final_insertion_sort: the fallback was reached AND its tie order shows in the result.
extern "C" int fallback_probe(int n, const int* key, int* seg, int cap, int* differs) {
    hinge_sort::KeyCmp c{key, 1};
    std::vector<int> idx(n);
    for (int i = 0; i < n; i++) idx[i] = i;
    int count = 0;
    std::vector<int> sf, sl, sd;
    if (n > 0) { sf.push_back(0); sl.push_back(n); sd.push_back(hinge_sort::floor_log2((unsigned)n) * 2); }
    while (!sf.empty()) {
        int first = sf.back(), last = sl.back(), depth = sd.back();
        sf.pop_back(); sl.pop_back(); sd.pop_back();
        while (last - first > 16) {
            if (depth == 0) { if (count < cap) seg[count] = last - first; ++count; break; }
            --depth;
            const int mid = first + (last - first) / 2;
            hinge_sort::move_median_to_first_(idx.data(), first, first + 1, mid, last - 1, c);
            const int cut = hinge_sort::unguarded_partition_(idx.data(), first + 1, last, first, c);
            sf.push_back(first); sl.push_back(cut); sd.push_back(depth);
            first = cut;
        }
    }
    auto comp = [key](int x, int y) { return key[x] > key[y]; };
    std::vector<int> real(n), deep(n);
    for (int i = 0; i < n; i++) real[i] = deep[i] = i;
    std::sort(real.begin(), real.end(), comp);
    if (n > 1) {
        std::__introsort_loop(deep.begin(), deep.end(), (long)1 << 40, __gnu_cxx::__ops::__iter_comp_iter(comp));
        std::__final_insertion_sort(deep.begin(), deep.end(), __gnu_cxx::__ops::__iter_comp_iter(comp));
    }
    *differs = real != deep;
    return count;
}
'''

# (n, q): every case reaches the fallback; n = 40 .. 65 with ONE segment of 17 .. 64 elements (the replay's in-register path),
# n >= 100 with q <= 2 ONE long segment (the level walk), q = 3 several segments, small ones among them
CASES = [(n, q) for n in (40, 48, 63, 64, 65, 100, 257, 1000, 1024, 2048, 4095, 4096) for q in (1, 2)] + \
        [(1000, 3), (2048, 3), (4095, 3), (4096, 3), (2048, 4), (4095, 4), (4096, 4)]

_lib = None


def harness(tmp_path_factory):
    """The compiled harness, once per session."""
    global _lib
    if _lib is None:
        d = tmp_path_factory.mktemp("sort_killer")
        src = d / "h.cpp"
        src.write_text(HARNESS)
        so = d / "h.so"
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "hinge_amd", "csrc"), "-o", str(so), str(src)])
        lib = ctypes.CDLL(str(so))
        lib.emul_sort_perm.argtypes = [ctypes.c_int, ip, ctypes.c_int, ip]
        lib.killer_keys.argtypes = [ctypes.c_int, ip]
        lib.fallback_probe.argtypes = [ctypes.c_int, ip, ip, ctypes.c_int, ip]
        lib.fallback_probe.restype = ctypes.c_int
        _lib = lib
    return _lib


_keys = {}


def killer_key(lib, n, q):
    """int32 keys of case (n, q), for a descending sort.  Computed once and handed out read-only."""
    if (n, q) not in _keys:
        val = np.zeros(n, np.int32)
        lib.killer_keys(n, P(val))
        key = np.ascontiguousarray(-(val // q), np.int32)
        key.setflags(write=False)
        _keys[(n, q)] = key
    return _keys[(n, q)]


def fallback_segments(lib, key):
    """(sizes of the segments std::sort heap-sorts, whether the result differs from an introsort without depth limit)."""
    key = np.ascontiguousarray(key, np.int32)
    seg = np.zeros(64, np.int32)
    differs = ctypes.c_int(0)
    cnt = lib.fallback_probe(len(key), P(key), P(seg), len(seg), ctypes.cast(ctypes.pointer(differs), ip))
    assert cnt <= len(seg)
    return seg[:cnt].tolist(), bool(differs.value)


def assert_case_reaches_the_fallback(lib, n, q):
    """The non-vacuity conditions of a case, asserted (never skipped): see CASES."""
    segs, differs = fallback_segments(lib, killer_key(lib, n, q))
    assert len(segs) >= 1, ("no segment reaches the depth limit", n, q)
    if q >= 2:
        assert differs, ("the heap part's tie order does not show in the result", n, q)
    if n <= 65:
        assert len(segs) == 1 and 20 <= segs[0] <= 43, (n, q, segs)           # wave_small_sort_*'s dep == 0 branch
    elif q <= 2:
        assert len(segs) == 1 and n - 48 <= segs[0] <= n - 24 and segs[0] > 64, (n, q, segs)   # the level walk's depth == 0 branch
    if (n, q) == (1000, 3):
        assert len(segs) == 2 and max(segs) <= 59, segs                         # small segments that arrive with the budget spent
    if (n, q) == (2048, 3):
        assert sorted(s > 64 for s in segs) == [False, True, True], segs
    if (n, q) == (4096, 3):
        assert len(segs) == 3 and min(segs) > 64, segs
    return segs


def oracle_perm(lib, key, fn="oracle_sort_perm"):
    """perm[p] = element at position p after the oracle's / the reference's std::sort, descending (compare_overlap / pairDescend)."""
    key = np.ascontiguousarray(key, np.int32)
    perm = np.zeros(max(len(key), 1), np.int32)
    getattr(lib, fn)(len(key), P(key), 0, P(perm))
    return perm[:len(key)]


def perm_of_positions(pos):
    """The device hooks return pos[e] = position of element e."""
    perm = np.full(len(pos), -1, np.int32)
    perm[pos] = np.arange(len(pos), dtype=np.int32)
    return perm
