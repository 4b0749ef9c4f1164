#!/usr/bin/env python3
"""Measurements behind the defaults of `hinge seed`, on the numpy model of tests/seed_common.py - no GPU.

  min-hits   the largest best-window count of 16 seeded reads of 7 128 random bases (the bench's mean placement) against a random
             4.6 Mb draft, both strands, at the defaults; HINGE_SEED_MIN_HITS is that plus half, rounded up - the rule
             HINGE_TRACE_LOCAL_MIN_SCORE was set by
  recall     on cns_tiny, cns_twobyte, cns_noisy and cns_small: the generator's records of >= 400 contig bases (a read's longest)
             whose contig, strand and diagonal the first placement gives, and the smallest winning count; --step to vary
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seed_common as sm  # noqa: E402


def min_hits(args):
    rng = np.random.default_rng(args.seed)
    draft = rng.integers(0, 4, size=args.draft, dtype=np.uint8)
    index = sm.Index([draft], args.k, args.max_occ)
    best = []
    for _ in range(args.reads):
        read = rng.integers(0, 4, size=args.length, dtype=np.uint8)
        for comp in (0, 1):
            st, nh, picks = sm.job_picks(index, sm.revcomp(read) if comp else read, args.step, args.window, args.list, 1, 1)
            best.append(picks[0][0] if picks else 0)
    top = max(best)
    value = top + -(-top // 2)
    print(json.dumps({"mode": "min-hits", "k": args.k, "step": args.step, "window": args.window, "max_occ": args.max_occ, "draft_bases": args.draft, "reads": args.reads,
                      "read_bases": args.length, "best_window_counts": best, "largest": top, "min_hits": value}))


def recall(args):
    from hinge_amd import synth_consensus as sc
    out = {"mode": "recall", "k": args.k, "step": args.step, "window": args.window, "sets": {}}
    for name in ("cns_tiny", "cns_twobyte", "cns_noisy", "cns_small"):
        d = sc.generate(sc.CONFIGS[name])
        index = sm.Index(d.contigs, args.k, args.max_occ)
        res = sm.model_seed(d.contigs, d.reads, step=args.step, window=args.window, list_=args.list, min_hits=args.min_hits, index=index)
        checked, missed, left_out = sm.recall(d, res, index, args.window)
        at = np.concatenate([[0], np.cumsum(res[3])])
        firsts = [res[1][int(a)] for a, n in zip(at[:-1], res[3]) if n]
        out["sets"][name] = {"records_checked": checked, "missed": len(missed), "under_400_left_out": len(left_out), "smallest_winning_count": min(firsts) if firsts else 0,
                             "unplaced_reads": int(sum(n == 0 for n in res[3]))}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("min-hits", "recall"))
    ap.add_argument("--k", type=int, default=sm.K)
    ap.add_argument("--step", type=int, default=sm.STEP)
    ap.add_argument("--window", type=int, default=sm.WINDOW)
    ap.add_argument("--max-occ", type=int, default=sm.MAX_OCC)
    ap.add_argument("--list", type=int, default=sm.LIST)
    ap.add_argument("--min-hits", type=int, default=sm.MIN_HITS)
    ap.add_argument("--draft", type=int, default=4_600_000)
    ap.add_argument("--reads", type=int, default=16)
    ap.add_argument("--length", type=int, default=7128)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    {"min-hits": min_hits, "recall": recall}[args.mode](args)


if __name__ == "__main__":
    main()
