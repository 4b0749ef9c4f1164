#!/usr/bin/env python
"""`hinge paf2las` at bench size: the records of hinge_amd/synth_consensus.py "cns_bench" (4 contigs of ~1.1 Mb at 30x: 18.8 k
placements, 134 M aligned contig bases), stripped of their traces, through hinge_trace_run.  Reports the kernels' time on resident
data (HIP events around every launch, hinge_profile_*), placements/s, aligned bases/s, the direction scratch and the batches, and -
for scale - the wall time of `hinge consensus` on the .las made of the result beside the generator's own .las (the two FASTAs need
not be equal: the generator's path and the banded optimum are different alignments; how many bases differ is reported).
There is no reference program for this step here (DALIGNER is not part of the reference tree): no speed-up factor is claimed.
Prints one JSON line.

--ends refine: after the plain run, the same placements with every end point moved by a seeded -80 .. +80 bases (kept inside its
sequence) through hinge_trace_refine: fill and clip kernel ms, placements/s, and the share of records whose four refined end points
all lie within 10 bases of the generator's, with the miss percentiles.  A second JSON line.
--ends local: the same perturbed placements through hinge_trace_local (k_trace_fill_local, k_trace_walk_local), the same figures;
`--ends refine local` gives both lines from one session.

    python tools/paf2las_bench.py [--config cns_bench] [--steps 3] [--band 128] [--band-max 1024] [--no-consensus] [--ends refine|local ... [--extend E]]
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
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--band-max", type=int, default=0)
    ap.add_argument("--no-consensus", action="store_true")
    ap.add_argument("--keep", default="")
    ap.add_argument("--ends", choices=("given", "refine", "local"), nargs="+", default=["given"])
    ap.add_argument("--extend", type=int, default=-1)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import consensus_common as cc
    from hinge_amd import capi, formats
    wd = args.keep or tempfile.mkdtemp(prefix="hinge_p2l_")
    os.makedirs(wd, exist_ok=True)
    d = cc.make(args.config, wd)
    r = d.rec
    pl = np.stack([r["aread"], r["bread"], (r["flags"] & 1).astype(np.int32), r["abpos"], r["aepos"], r["bbpos"], r["bepos"]], axis=1).astype(np.int64)
    aligned = int((r["aepos"] - r["abpos"]).sum())
    ts = d.spec.tspace
    out = {"config": args.config, "placements": int(len(pl)), "aligned_bases": aligned, "tspace": ts, "reference_program": None,
           "note": "no reference program for this step on this machine (DALIGNER is an empty submodule of the reference): no speed-up factor"}
    ctx = capi.Context(0)
    capi.Consensus(ctx, os.path.join(wd, "draft"), os.path.join(wd, "reads"))
    alns, trace, diffs, status = ctx.trace_run(pl, ts, args.band, args.band_max)        # warm-up (allocations)
    out["stats"] = ctx.trace_stats()
    out["final_w"] = {str(w): int(c) for w, c in zip(*np.unique(status[:, 1], return_counts=True))}
    out["status"] = {str(s): int(c) for s, c in zip(*np.unique(status[:, 0], return_counts=True))}
    ctx.profile_enable(4096)
    t = time.time()
    for _ in range(args.steps):
        ctx.trace_run(pl, ts, args.band, args.band_max)
    call_ms = (time.time() - t) * 1e3 / args.steps
    rep = ctx.profile_report()
    out["run_call_ms"] = round(call_ms, 3)       # host batching + H2D + kernels + D2H, all rounds
    out["kernels_ms"] = {k: round(v[0] / args.steps, 4) for k, v in rep.items() if k.startswith("k_trace") and v[1]}
    out["launches_per_call"] = {k: v[1] // args.steps for k, v in rep.items() if k.startswith("k_trace") and v[1]}
    ksum = sum(out["kernels_ms"].values())
    out["placements_per_s_kernels"] = len(pl) / (ksum * 1e-3) if ksum else None
    out["aligned_bases_per_s_kernels"] = aligned / (ksum * 1e-3) if ksum else None
    out["placements_per_s_call"] = len(pl) / (call_ms * 1e-3)
    out["diffs_vs_generator"] = {"ours": int(diffs.sum()), "generator": int(r["diffs"][status[:, 0] == 0].sum())}
    if not args.no_consensus:
        # `hinge consensus` on the generator's .las and on ours (same DBs)
        walls = {}
        t = time.time()
        gen_fasta, _ = cc.run_product(wd, out="gen.fasta")
        walls["generator_las_s"] = round(time.time() - t, 3)
        wd2 = os.path.join(wd, "ours")
        os.makedirs(wd2, exist_ok=True)
        for f in os.listdir(wd):
            if f.endswith((".db", ".ini")) or f.startswith((".draft.", ".reads.")):
                shutil.copy(os.path.join(wd, f), os.path.join(wd2, f))
        ok = status[:, 0] == 0
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
        walls["our_las_s"] = round(time.time() - t, 3)
        out["consensus_wall"] = walls

        def seqs(b):
            return [s.split(b"\n", 1)[1].replace(b"\n", b"") for s in b.split(b">")[1:]]
        cmp_ = []
        for x, y in zip(seqs(gen_fasta), seqs(our_fasta)):
            e = {"len_generator": len(x), "len_ours": len(y)}
            if len(x) == len(y):
                e["bases_differing"] = int((np.frombuffer(x.upper(), np.uint8) != np.frombuffer(y.upper(), np.uint8)).sum())
            cmp_.append(e)
        out["consensus_fasta"] = cmp_
    print(json.dumps(out))
    for mode in args.ends:
        if mode != "given":
            print(json.dumps(refine_line(args, ctx, d, pl, ts, ksum, mode)))
    if not args.keep:
        shutil.rmtree(wd, ignore_errors=True)


def refine_line(args, ctx, d, pl, ts, plain_kernels_ms, mode):
    import numpy as np
    run = ctx.trace_local if mode == "local" else ctx.trace_refine
    rng = np.random.default_rng(args.seed)
    alen = np.asarray([len(d.contigs[a]) for a in pl[:, 0]], np.int64)
    blen = np.asarray([len(d.reads[b]) for b in pl[:, 1]], np.int64)
    mv = rng.integers(-80, 81, size=(len(pl), 4))
    pp = pl.copy()
    pp[:, 3] = np.clip(pl[:, 3] + mv[:, 0], 0, alen)
    pp[:, 4] = np.clip(pl[:, 4] + mv[:, 1], 0, alen)
    pp[:, 5] = np.clip(pl[:, 5] + mv[:, 2], 0, blen)
    pp[:, 6] = np.clip(pl[:, 6] + mv[:, 3], 0, blen)
    assert (pp[:, 3] < pp[:, 4]).all() and (pp[:, 5] < pp[:, 6]).all()
    alns, trace, diffs, status, score = run(pp, ts, args.band, args.band_max, args.extend)     # warm-up (allocations)
    out = {"config": args.config, "ends": mode, "extend": args.extend, "perturbed_by": 80, "seed": args.seed, "placements": int(len(pp)), "stats": ctx.trace_stats()}
    out["final_w"] = {str(w): int(c) for w, c in zip(*np.unique(status[:, 1], return_counts=True))}
    out["status"] = {str(s): int(c) for s, c in zip(*np.unique(status[:, 0], return_counts=True))}
    ctx.profile_enable(4096)
    t = time.time()
    for _ in range(args.steps):
        run(pp, ts, args.band, args.band_max, args.extend)
    call_ms = (time.time() - t) * 1e3 / args.steps
    rep = ctx.profile_report()
    out["run_call_ms"] = round(call_ms, 3)
    out["kernels_ms"] = {k: round(v[0] / args.steps, 4) for k, v in rep.items() if k.startswith("k_trace") and v[1]}
    out["launches_per_call"] = {k: v[1] // args.steps for k, v in rep.items() if k.startswith("k_trace") and v[1]}
    ksum = sum(out["kernels_ms"].values())
    out["placements_per_s_kernels"] = len(pp) / (ksum * 1e-3) if ksum else None
    out["placements_per_s_call"] = len(pp) / (call_ms * 1e-3)
    out["kernels_ms_over_plain"] = round(ksum / plain_kernels_ms, 3) if plain_kernels_ms else None
    ok = status[:, 0] == 0
    far = np.zeros(len(pp), np.int64)
    for k, name in enumerate(("abpos", "aepos", "bbpos", "bepos")):
        far = np.maximum(far, np.abs(alns[name].astype(np.int64) - pl[:, 3 + k]))
    out["records"] = int(ok.sum())
    out["share_within_10"] = float((far[ok] <= 10).mean()) if ok.any() else None
    out["miss_percentiles_50_90_99_max"] = [int(v) for v in np.percentile(far[ok], [50, 90, 99, 100])] if ok.any() else None
    return out


if __name__ == "__main__":
    main()
