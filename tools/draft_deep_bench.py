#!/usr/bin/env python
"""`hinge_draft_ladders` on the ground beyond the first draft kernels: DEEP ladders (65+ members: k_draft_cns_deep)
and LONG ladders (members of 30-80 kb: k_draft_align_long).

    python tools/draft_deep_bench.py [--deep-ladders 1000] [--deep-members 100] [--deep-length 900] [--long-ladders 200]
                                     [--long-min 30000] [--long-max 80000] [--err 0.12] [--steps 2] [--cpu-seconds 20] [--no-cpu]
                                     [--only deep|long]

Deep set: --deep-ladders ladders of Poisson(--deep-members) members (at least 65), one in twenty of 300-600 members, each member a
noisy copy (--err: substitutions, insertions, deletions) of the window's truth of ~--deep-length bases.  Long set: --long-ladders
ladders of 3-10 members of --long-min .. --long-max bases.  Members sit inside longer stored reads on either strand, as in
tools/draft_bench.py (whose ladders stay inside the first kernels' envelope: it clamps members to 64).

Per set: call ms (host tables + H2D + kernels + D2H), kernel ms per k_draft* kernel, ladders/s; CPU baseline = the REFERENCE'S OWN
falcon (`ref_falcon_ladder` over lib/falcon.c + DW_banded.c compiled unmodified, one thread) on the first ladders of the set for
--cpu-seconds, every one byte-checked against the GPU's string (a mismatch fails the run).  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from draft_bench import noisy  # noqa: E402


def make(sizes, lengths, err, seed, wd, name):
    """Ladders of sizes[l] members around a truth of lengths[l] bases: (db, rungs, templates, members)."""
    import numpy as np
    from hinge_amd import formats
    rng = np.random.default_rng(seed)
    reads, rungs, templates, members = [], [], [], []
    k = 0
    for n, L in zip(sizes, lengths):
        truth = rng.integers(0, 4, int(L)).astype(np.uint8)
        rg, ms = [], []
        for m in range(int(n)):
            fwd = noisy(rng, truth, err)
            pad_l, pad_r = int(rng.integers(0, 40)), int(rng.integers(0, 40))
            body = np.concatenate([rng.integers(0, 4, pad_l).astype(np.uint8), fwd, rng.integers(0, 4, pad_r).astype(np.uint8)])
            strand = int(rng.integers(0, 2))
            reads.append((3 - body[::-1]).astype(np.uint8) if strand else body)
            rg.append((k, strand, pad_l, pad_l + len(fwd)))
            ms.append(fwd)
            k += 1
        rungs.append(rg)
        members.append(ms)
        templates.append(int(rng.integers(0, int(n))))
    db = os.path.join(wd, name)
    formats.write_db(db, np.asarray([len(r) for r in reads], np.int32), bases=reads)
    return db, rungs, templates, members


def run_set(args, ctx, db, rungs, templates, members):
    from hinge_amd import capi
    n_l = len(rungs)
    out = {"ladders": n_l, "member_alignments": sum(len(r) for r in rungs), "max_members": max(len(r) for r in rungs),
           "member_bases": int(sum(len(m) for ms in members for m in ms)), "max_member_bases": int(max(len(m) for ms in members for m in ms))}
    dr = capi.Draft(ctx, db)
    got = dr.ladders(rungs, templates)            # warm-up (allocations)
    ctx.profile_enable(16 * args.steps)
    t = time.time()
    for _ in range(args.steps):
        got = dr.ladders(rungs, templates)
    call_ms = (time.time() - t) * 1e3 / args.steps
    rep = ctx.profile_report()
    out["call_ms"] = round(call_ms, 3)
    out["kernels_ms"] = {k: round(v[0] / args.steps, 4) for k, v in rep.items() if k.startswith("k_draft") and v[1]}
    ksum = sum(out["kernels_ms"].values())
    out["kernels_ms_sum"] = round(ksum, 4)
    out["ladders_per_s_kernels"] = n_l / (ksum * 1e-3) if ksum else None
    out["ladders_per_s_call"] = n_l / (call_ms * 1e-3)
    if not args.no_cpu:
        import oracle
        import draft_common as dc
        ref = oracle.ref_lib()
        if ref is None or not hasattr(ref, "ref_falcon_ladder"):
            raise SystemExit("oracle/_ref/libhinge_ref.so is needed for the CPU baseline (or pass --no-cpu)")
        fn = dc.bind_ref(ref).ref_falcon_ladder
        t = time.time()
        done = 0
        for l in range(n_l):
            mem = ["".join("acgt"[x] for x in m) for m in members[l]]
            n, want = dc.ladder_call(fn, mem, templates[l])
            assert n >= 0 and want == got[l], "ladder %d: the GPU's consensus differs from the reference's (%d vs %d bases)" % (l, len(got[l]), len(want))
            done += 1
            if time.time() - t > args.cpu_seconds:
                break
        wall = time.time() - t
        out["cpu"] = {"kind": "reference", "cores": 1, "ladders": done, "wall_s": round(wall, 3), "ladders_per_s": done / wall,
                      "sample": "the first %d of the %d ladders" % (done, n_l)}
        out["byte_identical"] = True
        out["speedup_kernels_vs_cpu"] = round(out["ladders_per_s_kernels"] / out["cpu"]["ladders_per_s"], 1) if ksum else None
        out["speedup_call_vs_cpu"] = round(out["ladders_per_s_call"] / out["cpu"]["ladders_per_s"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deep-ladders", type=int, default=1000)
    ap.add_argument("--deep-members", type=int, default=100)
    ap.add_argument("--deep-length", type=int, default=900)
    ap.add_argument("--long-ladders", type=int, default=200)
    ap.add_argument("--long-min", type=int, default=30000)
    ap.add_argument("--long-max", type=int, default=80000)
    ap.add_argument("--err", type=float, default=0.12)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", choices=["deep", "long"])
    args = ap.parse_args()
    import numpy as np
    from hinge_amd import capi
    wd = tempfile.mkdtemp(prefix="hinge_draft_deep_bench_")
    rng = np.random.default_rng(args.seed)
    out = {"error_rate": args.err, "steps": args.steps}
    ctx = capi.Context(0)
    if args.only != "long":
        sizes = np.maximum(65, rng.poisson(args.deep_members, args.deep_ladders))
        big = rng.random(args.deep_ladders) < 0.05
        sizes[big] = rng.integers(300, 601, int(big.sum()))
        lengths = rng.integers(args.deep_length * 9 // 10, args.deep_length * 11 // 10 + 1, args.deep_ladders)
        t0 = time.time()
        data = make(sizes, lengths, args.err, args.seed + 1, wd, "D")
        out["deep"] = {"generate_s": round(time.time() - t0, 2), "mean_members": float(sizes.mean()), "length": args.deep_length}
        out["deep"].update(run_set(args, ctx, *data))
    if args.only != "deep":
        sizes = rng.integers(3, 11, args.long_ladders)
        lengths = rng.integers(args.long_min, args.long_max + 1, args.long_ladders)
        t0 = time.time()
        data = make(sizes, lengths, args.err, args.seed + 2, wd, "L")
        out["long"] = {"generate_s": round(time.time() - t0, 2), "mean_members": float(sizes.mean()), "length": [args.long_min, args.long_max]}
        out["long"].update(run_set(args, ctx, *data))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
