#!/usr/bin/env python
"""`hinge overlap` at bench size: the reads of hinge_amd/synth_consensus.py "cns_bench" (4 contigs of ~1.1 Mb at 30x: 18.8 k reads,
E. coli size) against themselves through hinge_overlap_run, then hinge_trace_local on the candidates.  One JSON line; every figure
sits in "figures" as {"value": ..., "measured": "gpu" | "host" | "gpu+host" | "not measured"}:
  index_ms (every block's index; "measured" names the path that built them, from hinge_index_last_stats: the device build of
  index_kernels.h, or - HINGE_INDEX_DEVICE=0, or a block beyond the scratch budget - the host build and its upload; the index
  kernels' own time by HIP events is in index_kernels_ms), k_overlap_vote_ms (HIP events, hinge_profile_*), candidates_per_s (by the
  kernel's time), trace_local_ms and its records on the first --align candidates (0 = all), records_written (the executable, with
  --cli), recall: the generator's pairs sharing >= 2 000 contig bases (from the reads' longest records on the contigs they were cut
  from) that are candidates after the mirror step.
--max-stretches S: everything through hinge_overlap_run_multi with S rounds (k_overlap_vote_multi_ms in place of k_overlap_vote_ms,
candidates_per_round) and `hinge overlap --max-stretches S` with --cli.  --ab N: N interleaved repetitions of hinge_overlap_run and
hinge_overlap_run_multi at 1, 2 and 4 stretches, each kernel's time by HIP events (vote_kernels_ab_ms: every run and the median).
--tile T: everything through hinge_overlap_run_tiled with query tiles of T bases (k_overlap_vote_tile_ms and
k_overlap_tile_reduce_ms in place of k_overlap_vote_ms, tile_stats) and `hinge overlap --tile T` with --cli; with --ab N: N
interleaved repetitions of hinge_overlap_run and hinge_overlap_run_tiled, each kernel's time by HIP events (tile_ab_ms: every run, the
medians and the ratio of the tiled kernels' time to k_overlap_vote's).
--tile T --tile-stretches S: everything through hinge_overlap_run_tiled_multi with S rounds (k_overlap_vote_tile_multi_ms and
k_overlap_tile_reduce_multi_ms, candidates_per_round) and `hinge overlap --tile T --tile-stretches S` with --cli; with --ab N: N
interleaved repetitions of hinge_overlap_run_tiled and hinge_overlap_run_tiled_multi at 1, 2 and 4 rounds, every kernel's time by
HIP events (tile_multi_ab_ms: every run and the medians of the vote kernel, the reduce and their sum).
There is no reference program for this step here (DALIGNER is not part of the reference tree): no speed-up factor is claimed.

    python tools/overlap_bench.py [--config cns_bench] [--steps 2] [--align 200000] [--cli] [--keep DIR] [--max-stretches S] [--ab N] [--tile T] [--tile-stretches S]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def truth_pairs(d, min_shared):
    """{(a, b, comp)} of ordered read pairs whose longest records lie on one contig and share >= min_shared of its bases."""
    import numpy as np
    best = {}
    for q in d.rec:
        b, ln = int(q["bread"]), int(q["aepos"]) - int(q["abpos"])
        if b not in best or ln > best[b][0]:
            best[b] = (ln, int(q["aread"]), int(q["abpos"]), int(q["aepos"]), int(q["flags"]) & 1)
    ids = np.asarray(sorted(best), np.int64)
    c = np.asarray([best[b][1] for b in ids]); s = np.asarray([best[b][2] for b in ids]); e = np.asarray([best[b][3] for b in ids]); st = np.asarray([best[b][4] for b in ids])
    out = set()
    order = np.lexsort((s, c))
    ids, c, s, e, st = ids[order], c[order], s[order], e[order], st[order]
    key = s + (c.astype(np.int64) << 40)
    for i in range(len(ids)):
        j1 = int(np.searchsorted(key, e[i] + (int(c[i]) << 40), side="left"))
        for j in range(i + 1, j1):
            if min(e[i], e[j]) - s[j] >= min_shared:
                comp = int(st[i] != st[j])
                out.add((int(ids[i]), int(ids[j]), comp)); out.add((int(ids[j]), int(ids[i]), comp))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cns_bench")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--align", type=int, default=200000)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--keep", default="")
    ap.add_argument("--max-stretches", type=int, default=0)
    ap.add_argument("--ab", type=int, default=0)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--tile-stretches", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import consensus_common as cc
    import overlap_common as oc
    from hinge_amd import capi
    wd = args.keep or tempfile.mkdtemp(prefix="hinge_overlap_")
    os.makedirs(wd, exist_ok=True)
    d = cc.make(args.config, wd)
    rlen = np.asarray([len(x) for x in d.reads], np.int64)
    fig = {}

    def put(name, value, how):
        fig[name] = {"value": value, "measured": how}
    out = {"config": args.config, "reads": len(d.reads), "read_bases": int(rlen.sum()), "reference_program": None,
           "note": "no reference program for this step on this machine (DALIGNER is an empty submodule of the reference): no speed-up factor", "figures": fig}
    ctx = capi.Context(0)
    capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))
    t = time.time()
    S = args.max_stretches
    T = args.tile
    TS = args.tile_stretches
    assert not (S and T), "--tile and --max-stretches do not go together"
    assert T or not TS, "--tile-stretches needs --tile"
    kernel = "k_overlap_vote_multi" if S else "k_overlap_vote_tile_multi" if TS else "k_overlap_vote_tile" if T else "k_overlap_vote"
    reduce_kernel = "k_overlap_tile_reduce_multi" if TS else "k_overlap_tile_reduce"
    res = ctx.overlap_run(max_stretches=S, tile=T, tile_stretches=TS)                            # warm-up (allocations)
    pl, count, diag, rep, status, hits = res[:6]
    out["first_call_s"] = round(time.time() - t, 3)
    out["stats"] = ctx.overlap_stats()
    out["status"] = {str(s): int(c) for s, c in zip(*np.unique(status, return_counts=True))}
    ctx.profile_enable(4096)
    t = time.time()
    index_us = []
    for _ in range(args.steps):
        res = ctx.overlap_run(max_stretches=S, tile=T, tile_stretches=TS)
        index_us.append(ctx.overlap_stats()["index_us"])
    ist = ctx.index_last_stats()
    out["index_stats"] = ist
    index_path = "gpu" if ist["host_builds"] == 0 else "host" if ist["device_builds"] == 0 else "gpu+host"
    call_ms = (time.time() - t) * 1e3 / max(args.steps, 1)
    prof = ctx.profile_report()
    kernel_ms = prof[kernel][0] / max(args.steps, 1)
    print("overlap_bench: %d timed call(s) done" % args.steps, file=sys.stderr, flush=True)
    put("index_ms", round(float(np.mean(index_us)) / 1e3, 3) if index_us else None, index_path if index_us else "not measured")
    put("index_kernels_ms", {k: round(v[0] / max(args.steps, 1), 3) for k, v in prof.items() if k.startswith("k_index")} if ist["device_builds"] else None, "gpu" if ist["device_builds"] else "not measured")
    put(kernel + "_ms", round(kernel_ms, 3), "gpu")
    if T:
        out["tile"] = T
        out["tile_stats"] = ctx.overlap_tile_stats()
        put(reduce_kernel + "_ms", round(prof[reduce_kernel][0] / max(args.steps, 1), 3), "gpu")
    if S or TS:
        out["tile_stretches" if TS else "max_stretches"] = S or TS
        put("candidates_per_round", [int((res[6] == r).sum()) for r in range(S or TS)], "gpu")
    put("run_call_ms", round(call_ms, 3), "host")
    put("candidates", int(len(pl)), "gpu")
    put("candidates_per_s", round(len(pl) / (kernel_ms * 1e-3)) if kernel_ms else None, "gpu")
    put("largest_hits_kept", int(hits.max()) if hits.size else 0, "gpu")
    # ---- recall, candidate level, after the mirror step ------------------------------------------------------------------------------------
    want = truth_pairs(d, 2000)
    sym, sdg, added = oc.symmetrise([tuple(r) for r in pl.tolist()], diag.tolist(), rlen)
    got = {tuple(r[:3]) for r in sym}
    put("recall_pairs_2000", {"pairs": len(want), "candidates_of_them": len(want & got), "recall": len(want & got) / max(len(want), 1), "mirrored": added}, "gpu")
    # ---- hinge_trace_local on the candidates ----------------------------------------------------------------------------------------------------
    sym = np.asarray(sym, np.int64).reshape(-1, 7)
    part = sym if args.align <= 0 else sym[:args.align]
    ctx.profile_enable(65536)
    t = time.time()
    alns, trace, diffs, st, score = ctx.trace_local(part, 100)
    wall = time.time() - t
    prof = ctx.profile_report()
    put("trace_local_ms", {"kernels_ms": round(sum(v[0] for k, v in prof.items() if k.startswith("k_trace")), 3), "call_s": round(wall, 3), "candidates": int(len(part)),
                           "of": int(len(sym)), "records": int((st[:, 0] == 0).sum())}, "gpu")
    if args.ab and TS:
        names = ["tiled"] + ["tiled_multi S=%d" % x for x in (1, 2, 4)]
        runs = {n: {"vote": [], "reduce": [], "sum": []} for n in names}
        per_round = {}
        for _ in range(args.ab):
            for name in names:
                s_ab = int(name.split("=")[1]) if "=" in name else 0
                ctx.profile_enable(4096)
                res = ctx.overlap_run(tile=T, tile_stretches=s_ab)
                rp = ctx.profile_report()
                v, r = (rp["k_overlap_vote_tile_multi"][0], rp["k_overlap_tile_reduce_multi"][0]) if s_ab else (rp["k_overlap_vote_tile"][0], rp["k_overlap_tile_reduce"][0])
                runs[name]["vote"].append(round(v, 3)); runs[name]["reduce"].append(round(r, 3)); runs[name]["sum"].append(round(v + r, 3))
                if s_ab:
                    per_round[name] = [int((res[6] == x).sum()) for x in range(s_ab)]
            print("overlap_bench: a/b repetition done", file=sys.stderr, flush=True)
        put("tile_multi_ab_ms", {"runs": runs, "median": {n: {k: float(np.median(v)) for k, v in runs[n].items()} for n in names}}, "gpu")
        put("tile_multi_ab_candidates_per_round", per_round, "gpu")
    elif args.ab and T:
        runs = {"k_overlap_vote": [], "k_overlap_vote_tile": [], "k_overlap_tile_reduce": []}
        for _ in range(args.ab):
            ctx.profile_enable(4096)
            ctx.overlap_run()
            runs["k_overlap_vote"].append(round(ctx.profile_report()["k_overlap_vote"][0], 3))
            ctx.profile_enable(4096)
            ctx.overlap_run(tile=T)
            rp = ctx.profile_report()
            runs["k_overlap_vote_tile"].append(round(rp["k_overlap_vote_tile"][0], 3))
            runs["k_overlap_tile_reduce"].append(round(rp["k_overlap_tile_reduce"][0], 3))
            print("overlap_bench: a/b repetition done", file=sys.stderr, flush=True)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        put("tile_ab_ms", {"runs": runs, "median": med, "tiled_over_plain": round((med["k_overlap_vote_tile"] + med["k_overlap_tile_reduce"]) / med["k_overlap_vote"], 3)}, "gpu")
    elif args.ab:
        runs = {"k_overlap_vote": [], "k_overlap_vote_multi S=1": [], "k_overlap_vote_multi S=2": [], "k_overlap_vote_multi S=4": []}
        per_round = {}
        for _ in range(args.ab):
            for name in runs:
                s_ab = int(name.split("=")[1]) if "=" in name else 0
                ctx.profile_enable(4096)
                res = ctx.overlap_run(max_stretches=s_ab)
                runs[name].append(round(ctx.profile_report()[name.split()[0]][0], 3))
                if s_ab:
                    per_round[name] = [int((res[6] == r).sum()) for r in range(s_ab)]
            print("overlap_bench: a/b repetition done", file=sys.stderr, flush=True)
        put("vote_kernels_ab_ms", {k: {"runs": v, "median": float(np.median(v))} for k, v in runs.items()}, "gpu")
        put("vote_kernels_ab_candidates_per_round", per_round, "gpu")
    if args.cli:
        print("overlap_bench: the executable", file=sys.stderr, flush=True)
        t = time.time()
        r = subprocess.run([os.path.join(ROOT, "hinge_amd", "bin", "hinge"), "overlap", "reads", "reads.las"] + (["--max-stretches", str(S)] if S else []) + (["--tile", str(T)] if T else []) + (["--tile-stretches", str(TS)] if TS else []), cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        put("records_written", {"summary": r.stdout.decode().strip(), "stderr": r.stderr.decode().strip().splitlines()[-1:], "wall_s": round(time.time() - t, 3)}, "gpu")
    else:
        put("records_written", None, "not measured")
    print(json.dumps(out))
    if not args.keep:
        shutil.rmtree(wd, ignore_errors=True)


if __name__ == "__main__":
    main()
