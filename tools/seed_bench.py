#!/usr/bin/env python
"""`hinge seed` at bench size: the reads of hinge_amd/synth_consensus.py "cns_bench" (4 contigs of ~1.1 Mb at 30x: 18.8 k reads)
through hinge_seed_run.  One JSON line:
  index_ms with index_path = the path that built it, from hinge_index_last_stats ("gpu": the device build of index_kernels.h, whose
  kernels' time by HIP events is index_kernels_ms; "host": HINGE_INDEX_DEVICE=0 or a draft beyond the scratch budget - the host build
  and its upload), k_seed_vote's time on resident data (HIP events, hinge_profile_*),
  reads/s; the share of the generator's records recovered - per read its longest record, of >= 400 contig bases: contig, strand and a
  diagonal within window + 5 % of its length (tests/seed_common.py recall) -; hinge_trace_local's kernel time on the seeded
  placements beside its time on the generator's own; `hinge consensus` on the .las made from the seeded placements, with the bases
  that differ from consensus on the generator's own .las.
There is no reference program for this step here (DALIGNER is not part of the reference tree): no speed-up factor is claimed.

    python tools/seed_bench.py [--config cns_bench] [--steps 3] [--no-consensus] [--keep DIR]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cns_bench")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-consensus", action="store_true")
    ap.add_argument("--keep", default="")
    args = ap.parse_args()
    import numpy as np
    import consensus_common as cc
    import seed_common as sm
    from hinge_amd import capi, formats
    wd = args.keep or tempfile.mkdtemp(prefix="hinge_seed_")
    os.makedirs(wd, exist_ok=True)
    d = cc.make(args.config, wd)
    r = d.rec
    ts = d.spec.tspace
    gen = np.stack([r["aread"], r["bread"], (r["flags"] & 1).astype(np.int32), r["abpos"], r["aepos"], r["bbpos"], r["bepos"]], axis=1).astype(np.int64)
    out = {"config": args.config, "reads": len(d.reads), "generator_records": int(len(gen)), "draft_bases": int(sum(len(c) for c in d.contigs)),
           "read_bases": int(sum(len(x) for x in d.reads)), "reference_program": None,
           "note": "no reference program for this step on this machine (DALIGNER is an empty submodule of the reference): no speed-up factor"}
    ctx = capi.Context(0)
    capi.Consensus(ctx, os.path.join(wd, "draft"), os.path.join(wd, "reads"))
    pl, count, diag, n_placed, status = ctx.seed_run()                                 # warm-up (allocations)
    out["stats"] = ctx.seed_stats()
    out["status"] = {str(s): int(c) for s, c in zip(*np.unique(status, return_counts=True))}
    ctx.profile_enable(4096)
    t = time.time()
    index_us = []
    for _ in range(args.steps):
        ctx.seed_run()
        index_us.append(ctx.seed_stats()["index_us"])
    call_ms = (time.time() - t) * 1e3 / args.steps
    rep = ctx.profile_report()
    out["run_call_ms"] = round(call_ms, 3)                                             # index + H2D + kernel + D2H + the host's projection
    out["index_ms"] = round(float(np.mean(index_us)) / 1e3, 3)
    ist = ctx.index_last_stats()
    out["index_stats"] = ist
    out["index_path"] = "gpu" if ist["host_builds"] == 0 else "host" if ist["device_builds"] == 0 else "gpu+host"
    out["index_kernels_ms"] = {k: round(v[0] / args.steps, 4) for k, v in rep.items() if k.startswith("k_index")} if ist["device_builds"] else None
    out["kernel_ms"] = round(rep["k_seed_vote"][0] / args.steps, 4)
    out["reads_per_s_kernel"] = len(d.reads) / (out["kernel_ms"] * 1e-3) if out["kernel_ms"] else None
    out["reads_per_s_call"] = len(d.reads) / (call_ms * 1e-3)
    # ---- the recall rule -----------------------------------------------------------------------------------------------------------------
    off = np.concatenate([[0], np.cumsum([len(c) for c in d.contigs])]).astype(np.int64)

    class Off:
        pass
    ix = Off()
    ix.off = off
    checked, missed, left_out = sm.recall(d, ([tuple(x) for x in pl.tolist()], count.tolist(), diag.tolist(), n_placed.tolist(), None), ix)
    out["recall"] = {"records_checked": checked, "missed": len(missed), "share_recovered": (checked - len(missed)) / checked if checked else None, "under_400_left_out": len(left_out),
                     "smallest_count": int(count.min()) if len(count) else None}
    # ---- hinge_trace_local on the seeded placements beside the generator's ---------------------------------------------------------------
    kms = {}
    res = {}
    for name, p in (("generator", gen), ("seeded", pl)):
        ctx.trace_local(p, ts)                                                          # warm-up
        ctx.profile_enable(4096)
        res[name] = ctx.trace_local(p, ts)
        rep = ctx.profile_report()
        st = res[name][3]
        kms[name] = {"kernels_ms": round(sum(v[0] for k, v in rep.items() if k.startswith("k_trace")), 3), "placements": int(len(p)), "records": int((st[:, 0] == 0).sum()),
                     "final_w": {str(w): int(c) for w, c in zip(*np.unique(st[:, 1], return_counts=True))}}
    out["trace_local"] = kms
    if not args.no_consensus:
        walls = {}
        t = time.time()
        gen_fasta, _ = cc.run_product(wd, out="gen.fasta")
        walls["generator_las_s"] = round(time.time() - t, 3)
        wd2 = os.path.join(wd, "ours")
        os.makedirs(wd2, exist_ok=True)
        for f in os.listdir(wd):
            if f.endswith((".db", ".ini")) or f.startswith((".draft.", ".reads.")):
                shutil.copy(os.path.join(wd, f), os.path.join(wd2, f))
        alns, trace, diffs, st, score = res["seeded"]
        ok = st[:, 0] == 0
        rec = np.zeros(int(ok.sum()), dtype=formats.LAS_REC_DTYPE)
        a = alns[ok]
        for name in ("abpos", "aepos", "bbpos", "bepos", "aread", "bread", "tlen"):
            rec[name] = a[name]
        rec["flags"] = a["comp"]
        rec["diffs"] = diffs[ok]
        tb = 1 if ts <= 125 else 2
        tbytes = trace.astype(np.uint8) if tb == 1 else trace.astype("<u2").view(np.uint8)
        toff = np.concatenate([[0], np.cumsum(rec["tlen"].astype(np.int64) * tb)])
        order = np.lexsort((rec["abpos"], rec["bread"], rec["aread"]))
        pieces = [tbytes[toff[k]:toff[k + 1]] for k in order]
        formats.write_las(os.path.join(wd2, "draft.reads.las"), formats.LasRecords(ts, rec[order], np.concatenate(pieces) if pieces else np.zeros(0, np.uint8),
                                                                                    np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)))
        t = time.time()
        our_fasta, _ = cc.run_product(wd2, out="ours.fasta")
        walls["seeded_las_s"] = round(time.time() - t, 3)
        out["consensus_wall"] = walls

        def seqs(b):
            return [s.split(b"\n", 1)[1].replace(b"\n", b"") for s in b.split(b">")[1:]]
        cmp_ = []
        for x, y in zip(seqs(gen_fasta), seqs(our_fasta)):
            e = {"len_generator": len(x), "len_seeded": len(y)}
            if len(x) == len(y):
                e["bases_differing"] = int((np.frombuffer(x.upper(), np.uint8) != np.frombuffer(y.upper(), np.uint8)).sum())
            cmp_.append(e)
        out["consensus_fasta"] = cmp_
    print(json.dumps(out))
    if not args.keep:
        shutil.rmtree(wd, ignore_errors=True)


if __name__ == "__main__":
    main()
