#!/usr/bin/env python
"""`hinge filter` on ultra-long reads: the mask / annotate sweep with its long-read tier (k_mask_annotate_long).

    python tools/long_read_bench.py [--genome 20000000] [--coverage 25] [--steps 5] [--warmup 2] [--no-cpu] [--no-e2e]

The data set is synth.CONFIGS["ultra_long"] (log-normal read lengths up to 1.3 Mb, long repeats) at --genome bases - at least
20 Mb, so that the timed window is not all launch overhead.  Timed: the one-sweep pass of the part (hinge_filter_sweep: prediction,
sweep, median, guard-band reads) with HIP events around the call, warm, median of --steps; every kernel of it by its own event
pair (the long tier's launches - first sweep and MODE_FINAL - summed); `hinge filter` end to end (the executable: ingest, HIP
start-up, kernels, text output; median of three runs).  CPU baseline on the same .las: the REFERENCE'S OWN getOverlap + pile-up sort
+ profileCoverage x2 (`ref_filter_slice` of oracle/_ref/libhinge_ref.so, the baseline of bench.py's reference_slice: a strict
subset of what its filter does) where that library was built, else the oracle's restatement of the whole stage.  Prints one JSON line."""
import argparse
import ctypes
import dataclasses
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_baseline(wd, novl):
    import oracle
    lib = oracle.ref_lib()
    if lib is not None and hasattr(lib, "ref_filter_slice"):
        lib.ref_filter_slice.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]
        lib.ref_filter_slice.restype = ctypes.c_int
        secs = (ctypes.c_double * 3)()
        cnt = (ctypes.c_longlong * 3)()
        rc = lib.ref_filter_slice(os.path.join(wd, "G").encode(), os.path.join(wd, "G.las").encode(), 40, 300, secs, cnt)
        if rc == 0 and cnt[0] == novl:
            return {"kind": "reference", "cores": 1, "what": "getOverlap + pile-up sort + profileCoverage x2 (ref_filter_slice), one thread",
                    "seconds": sum(secs), "seconds_by_phase": {"get_overlap": secs[0], "index_and_sort": secs[1], "profile_coverage": secs[2]}}
        return {"error": "ref_filter_slice rc=%d records=%d (expected %d)" % (rc, cnt[0], novl)}
    cwd = os.getcwd()
    os.chdir(wd)
    try:
        t = time.perf_counter()
        rc = oracle.oracle_lib().oracle_filter(b"G", b"G.las", 0, b"O", b"nominal.ini", b"")
        t = time.perf_counter() - t
    finally:
        os.chdir(cwd)
    assert rc == 0, "oracle_filter rc=%d" % rc
    return {"kind": "port", "cores": 1, "what": "oracle_filter (CPU restatement of the whole stage incl. .las parse and text output), one thread", "seconds": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--coverage", type=float, default=25)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    if args.genome < 20_000_000:
        ap.error("--genome must be at least 20000000: below that the timed window is mostly launch overhead")
    import numpy as np
    from hinge_amd import capi, formats, synth
    from hinge_amd.config import default_filter_params
    wd = tempfile.mkdtemp(prefix="hinge_long_read_bench_")
    try:
        t0 = time.perf_counter()
        d = synth.generate(dataclasses.replace(synth.CONFIGS["ultra_long"], genome_len=args.genome, coverage=args.coverage))
        synth.write_dataset(d, wd, "G")
        with open(os.path.join(wd, "nominal.ini"), "w") as f:
            f.write("[filter]\nlength_threshold = 1000;\naln_threshold = 1000;\nmin_cov = 5;\ncut_off = 300;\ntheta = 300;\n")
        rlen = formats.read_db_index(os.path.join(wd, "G"))["rlen"]
        recs = formats.read_las(os.path.join(wd, "G.las"))
        pile = formats.pileups_from_las(recs, rlen)
        r0, r1 = int(recs.rec["aread"][0]), int(recs.rec["aread"][-1])
        P = default_filter_params()
        n_long = int(np.sum((np.asarray(rlen, np.int64) + P.cut_off) // P.reso + 4 > 5120))
        out = {"workload": "ultra_long at %d bases, coverage %g" % (args.genome, args.coverage), "reads": int(len(rlen)), "overlaps": int(d.novl),
               "las_bytes": os.path.getsize(os.path.join(wd, "G.las")), "longest_read": int(np.max(rlen)), "reads_beyond_lds": n_long,
               "reads_beyond_a_workgroups_lds": int(np.sum(np.asarray(rlen) > 819200)), "largest_pileup": int(np.max(np.diff(pile.row_ptr))),
               "long_read_bases": int(np.sum(np.asarray(rlen, np.int64)[(np.asarray(rlen, np.int64) + P.cut_off) // P.reso + 4 > 5120])),
               "generate_s": round(time.perf_counter() - t0, 2), "steps": args.steps, "warmup": args.warmup}
        ctx = capi.Context(0)
        ctx.set_reads(rlen, None)
        span16, max_pile, in_range = capi.pack_spans(pile.row_ptr, pile.a_span, rlen)
        ctx.set_pileups_packed(r0, r1, pile.row_ptr, pile.a_span, pile.b_span, pile.b_flag, span16, max_pile, in_range)
        ctx.coverage_out(True)
        for _ in range(args.warmup):
            ctx.set_min_cov(P.min_cov)
            ctx.filter_sweep(P)
        assert ctx.long_reads() == n_long
        sweep_ms = []
        ctx.profile_enable(32 * args.steps)
        for _ in range(args.steps):
            ctx.set_min_cov(P.min_cov)
            ctx.timer_start()
            ctx.filter_sweep(P)
            sweep_ms.append(ctx.timer_stop_ms())
        rep = ctx.profile_report()
        out["spec_stats"] = list(ctx.spec_stats())
        ctx.close()
        kernels = {k: round(v[0] / args.steps, 4) for k, v in rep.items() if v[1]}
        long_ms = kernels.get("k_mask_annotate_long", 0.0)
        out["sweep_ms"] = round(sorted(sweep_ms)[len(sweep_ms) // 2], 4)
        out["sweep_ms_runs"] = [round(x, 4) for x in sweep_ms]
        out["kernels_ms_per_sweep"] = kernels
        out["launches_per_sweep"] = {k: v[1] / args.steps for k, v in rep.items() if v[1]}
        out["long_tier_ms"] = long_ms
        out["rest_of_sweep_kernels_ms"] = round(sum(kernels.values()) - long_ms, 4)
        out["long_tier_reads_per_s"] = n_long / (long_ms * 1e-3) if long_ms else None
        out["long_tier_bases_per_s"] = out["long_read_bases"] / (long_ms * 1e-3) if long_ms else None
        if not args.no_e2e:
            hinge = os.path.join(ROOT, "hinge_amd", "bin", "hinge")
            runs = []
            for _ in range(3):
                t = time.perf_counter()
                r = subprocess.run([hinge, "filter", "--db", "G", "--las", "G.las", "-x", "H", "--config", "nominal.ini"], cwd=wd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
                runs.append(time.perf_counter() - t)
                assert r.returncode == 0, r.stderr.decode()[-1000:]
            out["filter_e2e_s"] = round(sorted(runs)[1], 4)
            out["filter_e2e_s_runs"] = [round(x, 4) for x in runs]
        if not args.no_cpu:
            out["cpu"] = cpu_baseline(wd, int(d.novl))
            if "seconds" in out["cpu"]:
                out["cpu_over_sweep"] = round(out["cpu"]["seconds"] / (out["sweep_ms"] * 1e-3), 1)
                if "filter_e2e_s" in out:
                    out["cpu_over_filter_e2e"] = round(out["cpu"]["seconds"] / out["filter_e2e_s"], 2)
        print(json.dumps(out))
    finally:
        shutil.rmtree(wd, ignore_errors=True)


if __name__ == "__main__":
    main()
