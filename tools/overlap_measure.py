#!/usr/bin/env python3
"""Measurements behind the defaults of `hinge overlap`, on the numpy model of tests/overlap_common.py - no GPU.

  min-hits   the largest group count over all pairs of seeded UNRELATED reads of 7 128 random bases (the bench's mean read), both
             strands, one block, at the defaults with min_hits 1; the rule of `hinge seed`: that plus half, rounded up
  max-occ    on a synth_draft set at a given coverage: the share of the index's codes and entries that max_occ drops, and the
             largest number of entries of one code
  recall     on the noisy set of tests/test_overlap_model.py: the generator's pairs sharing >= 2 000 genome bases that are
             candidates, the smallest count among them, and the candidates of pairs with disjoint genome intervals
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overlap_common as oc  # noqa: E402
import seed_common as sm  # noqa: E402
from hinge_amd import synth_draft as sd  # noqa: E402


def min_hits(args):
    rng = np.random.default_rng(args.seed)
    reads = [rng.integers(0, 4, size=args.length, dtype=np.uint8) for _ in range(args.reads)]
    rows, cnt, dg, rep, status, hits, st = oc.model_overlap(reads, args.k, args.step, args.window, args.max_occ, args.list, oc.MAX_PARTNERS, 1)
    top = max(cnt) if cnt else 0
    hist = np.bincount(np.asarray(cnt, np.int64), minlength=top + 1).tolist() if cnt else []
    print(json.dumps({"mode": "min-hits", "k": args.k, "step": args.step, "window": args.window, "max_occ": args.max_occ, "reads": args.reads, "read_bases": args.length,
                      "pairs_with_a_hit": len(cnt), "count_histogram": hist, "largest": top, "min_hits_by_rule": top + -(-top // 2)}))


def max_occ(args):
    d = sd.generate(sd.DraftSpec(genome_len=args.genome, coverage=args.coverage, read_len=(3_000, 11_000), p_sub=0.02, p_ins=0.05, p_del=0.03, seed=args.seed))
    codes = np.sort(np.concatenate([sm.kmer_codes(r, args.k) for r in d.reads]))
    first = np.concatenate([[True], codes[1:] != codes[:-1]])
    size = np.bincount(np.cumsum(first) - 1)
    print(json.dumps({"mode": "max-occ", "k": args.k, "max_occ": args.max_occ, "coverage": args.coverage, "genome": args.genome, "reads": len(d.reads), "codes": int(len(size)),
                      "entries": int(size.sum()), "largest_code": int(size.max()), "codes_dropped": int((size > args.max_occ).sum()), "entries_dropped": int(size[size > args.max_occ].sum())}))


def recall(args):
    d = sd.generate(sd.DraftSpec(genome_len=20_000, coverage=12, read_len=(2_000, 4_000), min_ovl=1_000, p_sub=0.02, p_ins=0.05, p_del=0.03))
    rows, cnt, dg, rep, status, hits, st = oc.model_overlap(d.reads, args.k, args.step, args.window, args.max_occ, args.list, oc.MAX_PARTNERS, args.min_hits)
    want = oc.truth_pairs(d, 2_000)
    got = {tuple(r[:3]): c for r, c in zip(rows, cnt)}
    found = [got[x] for x in want if x in got]
    print(json.dumps({"mode": "recall", "step": args.step, "min_hits": args.min_hits, "pairs_2000": len(want), "candidates_of_them": len(found), "recall": len(found) / max(len(want), 1),
                      "smallest_count": min(found) if found else 0, "median_count": float(np.median(found)) if found else 0.0,
                      "disjoint_candidates": sum(1 for r in rows if oc.shared_bases(d, r[0], r[1]) <= 0), "largest_hits_kept": max(max(h) for h in hits), "stats": st}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("min-hits", "max-occ", "recall"))
    ap.add_argument("--k", type=int, default=oc.K)
    ap.add_argument("--step", type=int, default=oc.STEP)
    ap.add_argument("--window", type=int, default=oc.WINDOW)
    ap.add_argument("--max-occ", type=int, default=oc.MAX_OCC)
    ap.add_argument("--list", type=int, default=oc.LIST)
    ap.add_argument("--min-hits", type=int, default=oc.MIN_HITS)
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--length", type=int, default=7128)
    ap.add_argument("--genome", type=int, default=60_000)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    {"min-hits": min_hits, "max-occ": max_occ, "recall": recall}[args.mode](args)


if __name__ == "__main__":
    main()
