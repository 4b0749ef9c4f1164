"""The kernels of `hinge consensus` without a GPU: hinge_amd/csrc/consensus_kernels.h itself compiled for the host (tests/cns_host: a
stand-in <hip/hip_runtime.h> and a driver with its own main) and run as a child process under AddressSanitizer and UBSan, with every
buffer at the size hinge_amd/csrc/consensus_capi.inc gives it - the .bps copies bps_bytes + CNS_BPS_SPARE.  Compared: the packed
windows against the single-base fetch; the indel lists and chop offsets against the oracle's dump; CnsCols and the nine count planes
of BOTH votes (k_cns_vote's global counters, k_cns_vote_tiles' LDS tiles + halo) against tests/cns_model.py, whose own base calls must
give the oracle's FASTA.  Not run: k_cns_call and
k_cns_emit (cross-lane shuffles; the GPU tests cover them through the FASTA).  What this cannot show: anything the GPU's memory
system or compiler does differently."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cns_model
import consensus_common as cc

ROOT = cc.ROOT
HOST = os.path.join(ROOT, "tests", "cns_host")
CNS_LDS_BASES = 176       # consensus_kernels.h: segments up to this long are staged in LDS by k_cns_realign

# (key, configuration, overrides)
SETS = [("tiny", "cns_tiny", {}), ("noisy", "cns_noisy", {}), ("noisy_noflank", "cns_noisy", {"flank_max": 0}), ("noisy_noflank_noshort", "cns_noisy", {"flank_max": 0, "short_alignments": 0}), ("noisy_last_bytes", "cns_noisy", {"flank_max": 0, "short_alignments": 0, "contig_lens": (9008, 10036)}),
        ("tiny_t176", "cns_tiny", {"tspace": 176}), ("tiny_t177", "cns_tiny", {"tspace": 177})] + \
       [(n, n, {}) for n in ("cns_edge_t64", "cns_edge_t125", "cns_edge_t126", "cns_edge_t176", "cns_edge_t177", "cns_edge_t2048", "cns_edge_t2458")]
KEYS = [s[0] for s in SETS]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("cns_host"))
    shutil.copy(os.path.join(ROOT, "hinge_amd", "csrc", "consensus_kernels.h"), wd)       # the kernel source itself
    exe = os.path.join(wd, "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", wd, "-I", HOST, "-pthread", "-o", exe,
                        os.path.join(HOST, "driver.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return exe


def _read_dump(path):
    raw = open(path, "rb").read()
    want, p = {}, 0
    while p < len(raw):
        contig, pos, off, n = struct.unpack_from("<4i", raw, p)
        p += 16
        want[pos] = (contig, off, np.frombuffer(raw, dtype=np.int32, count=n, offset=p).copy())
        p += 4 * n
    return want


def _run_set(driver, oracle_lib, wd, name, over):
    """One data set through the oracle (dump) and the driver; everything the tests compare."""
    from hinge_amd import formats
    os.makedirs(wd)
    d = cc.make(name, wd, **over)
    fasta, _ = cc.run_oracle(oracle_lib, wd, dump="ora.dump")
    want = _read_dump(os.path.join(wd, "ora.dump"))
    picks = sorted(want)
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    tb = 1 if las.tspace <= 125 else 2
    tr16 = np.ascontiguousarray(las.trace.astype("<u2") if tb == 1 else np.ascontiguousarray(las.trace).view("<u2"))
    rec = las.rec[picks]
    aln = np.zeros((len(picks), 10), np.int32)
    for k, col in enumerate(("aread", "bread", None, "abpos", "aepos", "bbpos", "bepos", "tlen")):
        aln[:, k] = (rec["flags"] & 1) if col is None else rec[col]
    aln[:, 8] = las.trace_off[picks] // tb
    db = []
    for nm in ("draft", "reads"):       # the DBs as capi.Consensus hands them to hinge_consensus_set_db
        idx = formats.read_db_index(os.path.join(wd, nm))
        db.append((np.ascontiguousarray(idx["rlen"], np.int32), np.ascontiguousarray(idx["boff"], np.int64), np.fromfile(formats.db_paths(os.path.join(wd, nm))[2], np.uint8)))
    with open(os.path.join(wd, "in.bin"), "wb") as f:
        f.write(np.asarray([las.tspace, len(db[0][0]), len(db[1][0]), db[0][2].size, db[1][2].size, len(picks), tr16.size, 0], np.int64).tobytes())
        for rlen, boff, bps in db:
            f.write(rlen.tobytes()); f.write(boff.tobytes()); f.write(bps.tobytes())
        f.write(aln.tobytes()); f.write(tr16.tobytes())
    r = subprocess.run([driver, "run", "in.bin", "out.bin"], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (name, over, r.returncode, r.stderr.decode()[-4000:])
    o = np.fromfile(os.path.join(wd, "out.bin"), np.int32)
    n_seg, n_tiles, tile, n_pos, status, tiled = (int(v) for v in o[:6])
    p = [8]

    def take(n, shape=None):
        v = o[p[0]:p[0] + n]
        assert v.size == n
        p[0] += n
        return v.reshape(shape) if shape else v
    res = {"d": d, "fasta": fasta, "want": want, "picks": picks, "aln": aln, "tspace": las.tspace, "tile": tile, "n_tiles": n_tiles, "n_pos": n_pos, "status": status, "tiled": tiled,
           "rlen": (db[0][0], db[1][0]), "boff": (db[0][1], db[1][1]), "bps_bytes": (db[0][2].size, db[1][2].size)}
    res["segs"] = take(7 * n_seg, (n_seg, 7))          # aln, a0, m, b0, n, out_off, out_cap
    res["n_indel"], res["n_ins"], res["col_base"] = take(n_seg), take(n_seg), take(n_seg)
    res["cols"] = take(3 * len(picks), (len(picks), 3))     # start, end, offset
    res["indels"] = take(int(take(1)[0]))
    res["global"] = take(9 * n_pos, (9, n_pos)).astype(np.int64)
    res["tiles"] = take(9 * n_pos, (9, n_pos)).astype(np.int64)
    res["halo"] = take(4 * n_tiles, (n_tiles, 4)).astype(np.int64)
    res["tile_base"] = take(len(db[0][0]) + 1)
    assert p[0] == o.size
    return res


@pytest.fixture(scope="module")
def results(driver, oracle_lib, tmp_path_factory):
    top = str(tmp_path_factory.mktemp("cns_host_sets"))
    return {key: _run_set(driver, oracle_lib, os.path.join(top, key), name, over) for key, name, over in SETS}


def test_windows_equal_the_single_base_fetch(driver):
    """cns_window, CnsPair::winA / winB on both strands, and cns_stage + cns_lds_window / cns_lds_base against cns_base / A / B, base by
    base inside the sequence: sequences of 1, 15, 16, 17, 31, 33 and 64 bases, every start, as the last sequence of a .bps of
    bps_bytes + CNS_BPS_SPARE bytes and with another one behind."""
    r = subprocess.run([driver, "windows"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr.decode()[-4000:])
    w = r.stdout.decode().split()
    assert w[:2] == ["windows", "checked"] and int(w[2]) > 100_000 and int(w[4]) == 0


def _segments_of(res, k):
    s = np.nonzero(res["segs"][:, 0] == k)[0]
    assert s.size and np.array_equal(s, np.arange(s[0], s[0] + s.size))
    return s


@pytest.mark.parametrize("key", KEYS)
def test_segments_and_indel_lists_match_the_oracle(results, key):
    """Per used alignment: the segments tile [ab, ae) x [bb, be) and end on multiples of tspace; their indel lists, one after the
    other, are recoverAlignment's list as the oracle dumps it; n_ins and col_base follow from them; CnsCols.offset is chop_end's."""
    res = results[key]
    assert res["status"] == 0 and len(res["picks"]) >= 10
    ts = res["tspace"]
    for k, pos in enumerate(res["picks"]):
        a = res["aln"][k]
        sg = res["segs"][_segments_of(res, k)]
        assert sg[0, 1] == a[3] and sg[0, 3] == a[5] and sg[:, 2].sum() == a[4] - a[3] and sg[:, 4].sum() == a[6] - a[5]
        assert np.array_equal(sg[1:, 1], sg[:-1, 1] + sg[:-1, 2]) and np.array_equal(sg[1:, 3], sg[:-1, 3] + sg[:-1, 4])
        assert not (sg[1:, 1] % ts).any() and (sg[:, 1] // ts == (sg[:, 1] + sg[:, 2] - 1) // ts).all()
        s_idx = _segments_of(res, k)
        lists = [res["indels"][int(res["segs"][s, 5]):int(res["segs"][s, 5]) + int(res["n_indel"][s])] for s in s_idx]
        assert all(int(res["n_indel"][s]) <= int(res["segs"][s, 6]) for s in s_idx)
        got = np.concatenate(lists)
        assert np.array_equal(got, res["want"][pos][2]), "alignment %d: indel list differs from the oracle's" % pos
        assert [int(res["n_ins"][s]) for s in s_idx] == [int((l < 0).sum()) for l in lists]
        widths = sg[:, 2] + res["n_ins"][s_idx]
        assert np.array_equal(res["col_base"][s_idx], np.cumsum(widths) - widths)
        assert res["cols"][k, 2] == res["want"][pos][1]


@pytest.mark.parametrize("key", KEYS)
def test_columns_and_both_votes_match_the_model(results, key):
    """CnsCols and the nine count planes against tests/cns_model.py, from the ORACLE's indel lists; the tile vote + its halo slots (added
    to the first position of the next tile) against the global-atomics vote, plane by plane."""
    res = results[key]
    d = res["d"]
    first = np.concatenate([[0], np.cumsum(res["rlen"][0])]).astype(np.int64)
    model = np.zeros((9, res["n_pos"]), np.int64)
    for k, pos in enumerate(res["picks"]):
        a = res["aln"][k]
        read = d.reads[a[1]]
        bseq = (3 - read[::-1]) if a[2] else read
        kind, apos, base = cns_model.columns(int(a[3]), int(a[4]), int(a[5]), res["want"][pos][2], bseq)
        start, end, offset = cns_model.chop_end(kind)
        assert tuple(int(v) for v in res["cols"][k]) == (start, end, offset), "alignment %d: CnsCols" % pos
        cns_model.vote(model, int(first[a[0]]), int(res["rlen"][0][a[0]]), kind, apos, base, start, end)
    assert model[:5].sum() > 1000 and model[4].sum() > 0 and model[5:].sum() > 0
    # (the model itself: its base calls are the oracle's FASTA, which is the reference program's on every pinned set)
    text = "".join(">Consensus%d\n%s\n" % (c, cns_model.call(model[:, first[c]:first[c + 1]], d.contigs[c])) for c in range(len(d.contigs)))
    assert text == res["fasta"].decode()
    for b in range(9):
        assert np.array_equal(res["global"][b], model[b]), "k_cns_vote: plane %d" % b
    assert res["tiled"] == 1 and res["tile"] % res["tspace"] == 0
    tiles = res["tiles"].copy()
    for c in range(len(res["rlen"][0])):
        for t in range(int(res["tile_base"][c]), int(res["tile_base"][c + 1])):
            nxt = (t - int(res["tile_base"][c]) + 1) * res["tile"]
            if nxt < res["rlen"][0][c]:       # (behind the contig's last base: dropped, as k_cns_vote drops it)
                tiles[5:, first[c] + nxt] += res["halo"][t]
    for b in range(9):
        assert np.array_equal(tiles[b], model[b]), "k_cns_vote_tiles: plane %d" % b


def test_the_sets_reach_the_branches(results):
    """A data set that stops reaching a branch must fail here rather than pass empty."""
    r177 = results["tiny_t177"]
    staged = (r177["segs"][:, 2] <= CNS_LDS_BASES) & (r177["segs"][:, 4] <= CNS_LDS_BASES)
    assert staged.any() and (~staged).any(), "tspace 177: staged and unstaged segments"
    assert (results["tiny_t176"]["segs"][:, 2] == CNS_LDS_BASES).any() and (r177["segs"][:, 2] == CNS_LDS_BASES + 1).any()
    halo_used = comp_at_end = last_a = last_b = past_spare = 0
    for res in results.values():
        nA, nB = len(res["rlen"][0]), len(res["rlen"][1])
        for c in range(nA):
            for t in range(int(res["tile_base"][c]), int(res["tile_base"][c + 1])):
                if (t - int(res["tile_base"][c]) + 1) * res["tile"] < res["rlen"][0][c]:
                    halo_used += int(res["halo"][t].sum())
        for k in range(len(res["picks"])):
            a = res["aln"][k]
            last = res["segs"][_segments_of(res, k)[-1]]
            comp_at_end += int(a[2] == 1 and a[6] == res["rlen"][1][a[1]])
            last_a += int(a[0] == nA - 1 and a[4] == res["rlen"][0][a[0]] and last[2] % 16 != 0)
            last_b += int(a[1] == nB - 1 and a[2] == 0 and a[6] == res["rlen"][1][a[1]] and last[4] % 16 != 0)
            # the word behind the staged windows, had it been LOADED (two aligned 32-bit words from its first byte on) instead of written as 0
            byte = int(res["boff"][0][a[0]]) + ((int(last[1]) + 16 * ((int(last[2]) + 15) // 16)) >> 2)
            past_spare += int(last[2] <= CNS_LDS_BASES and last[4] <= CNS_LDS_BASES and byte // 4 * 4 + 8 > res["bps_bytes"][0] + 8)
    assert halo_used > 0, "no inserted base in a halo slot"
    assert comp_at_end > 0, "no complemented alignment that ends at its read's end (winB near the read's first bases)"
    assert past_spare > 0, "no staged segment whose spare word starts behind the draft .bps copy's spare bytes"
    assert last_a > 0 and last_b > 0, "no last segment at the end of the last sequence of each DB with a length off 16 (the .bps copy's last bytes)"
    # tile geometry: the tile as a multiple of tspace and as tspace itself, LDS counters past 48 KiB, contigs of whole tiles and one base either side
    assert results["cns_edge_t64"]["tile"] == 2048 and results["cns_edge_t2048"]["tile"] == 2048 and results["cns_edge_t2458"]["tile"] == 2458
    assert 5 * 4 * (results["cns_edge_t2458"]["tile"] + 1) > 48 * 1024
    assert sorted(int(v) - 4096 for v in results["cns_edge_t64"]["rlen"][0]) == [-1, 0, 1]
