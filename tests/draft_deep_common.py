"""Generators of ladders beyond the first kernels' envelope, shared by test_draft_deep_oracle.py (CPU) and test_draft_deep_gpu.py:
deep ladders (65+ members: k_draft_cns_deep) and ladders with long members (32768+ bases, or member + template beyond the aligner's
LDS: k_draft_align_long).  Every ladder is (members, template index); members are lower-case acgt strings.

No generator can make a run of 255 inserted bases: members are noisy copies of one truth at <= 20 % errors (an insertion before a
base with probability <= 9 %), an unrelated member has the template's length, a shared insertion is at most 100 bases.  The tests
assert it through the oracle's return value (>= 0: no reference-undefined case) instead of skipping such ladders."""
import numpy as np

import draft_common as dc

DEEP_SIZES = (65, 96, 128, 129, 200, 500, 1000, 4096)
LONG_SIZES = (32767, 32768, 40000, 70000)


def rand_seq(rng, n):
    return "".join("acgt"[i] for i in rng.integers(0, 4, n))


def deep_ladder(rng, n, L, err, kind=""):
    """n noisy copies (err) of a random L-base truth.  kind: 'early' (some members end early), 'unrelated' (one member is
    random), 'identical' (all members the same string: every column a tie), 'insertion' (most members share a 40-100-base
    insertion the template lacks: deltas >= 32, S2F)."""
    truth = rand_seq(rng, L)
    if kind == "identical":
        m = dc.noisy(rng, truth, err)
        return [m] * n, int(rng.integers(0, n))
    if kind == "insertion":
        ins = rand_seq(rng, int(rng.integers(40, 101)))
        at = L // 2
        with_ins = truth[:at] + ins + truth[at:]
        mem = [dc.noisy(rng, truth, min(err, 0.02))] + [dc.noisy(rng, with_ins, err) for _ in range(n - 1)]
        return mem, 0
    mem = [dc.noisy(rng, truth, err) for _ in range(n)]
    if kind == "early":
        for i in range(1, n, 7):
            mem[i] = mem[i][:max(1, int(len(mem[i]) * rng.uniform(0.2, 0.8)))]
    if kind == "unrelated":
        mem[int(rng.integers(1, n))] = rand_seq(rng, L)
    mem = [m if m else "a" for m in mem]
    return mem, int(rng.integers(0, n))


def tie_ladder(seed, L=300, sites=6, noise=0.0, swap=False):
    """Links that first appear in a member >= 64 and tie with a link from members 0 .. 63: at `sites` positions group X carries
    the truth's base, group Y another one and group Z a third.  X = members 0 .. 55 and 120 .. 127, Z = 56 .. 63 (the template is
    member 56), Y = 64 .. 119 and 128 .. 135: X and Y have 64 members each, Y's links first appear in member 64, both counts are
    sums over two chunks.  The columns behind such a site have links of equal score, and the one numbered first wins: with
    swap=True (X's and Y's sequences traded, same template) the consensus changes."""
    rng = np.random.default_rng(seed)
    truth = list(rand_seq(rng, L))
    alt, third = list(truth), list(truth)
    for p in np.sort(rng.choice(np.arange(20, L - 20), size=sites, replace=False)):
        b = "acgt".index(truth[p])
        alt[p], third[p] = "acgt"[(b + 1) % 4], "acgt"[(b + 2) % 4]
    seqs = {"x": "".join(truth), "y": "".join(alt), "z": "".join(third)}
    if swap:
        seqs["x"], seqs["y"] = seqs["y"], seqs["x"]
    group = "x" * 56 + "z" * 8 + "y" * 56 + "x" * 8 + "y" * 8
    mem = [dc.noisy(rng, seqs[g], noise) for g in group]
    return [m if m else "a" for m in mem], 56


def deep_cases(rng):
    """The deep set: every size of DEEP_SIZES with error rates 0-20 % and each kind, plus the tie ladders."""
    cases = []
    kinds = ["", "early", "unrelated", "identical", "insertion"]
    for i, n in enumerate(DEEP_SIZES):
        L = 400 if n <= 200 else (200 if n <= 1000 else 60)
        for j, kind in enumerate(kinds):
            if n >= 1000 and j >= 3:
                continue
            err = [0.0, 0.05, 0.1, 0.15, 0.2][(i + j) % 5]
            cases.append(deep_ladder(rng, n, L, err, kind))
    for seed in (1, 2):
        cases.append(tie_ladder(seed))
        cases.append(tie_ladder(seed, swap=True))
    cases.append(tie_ladder(3, noise=0.01))
    return cases


def long_cases(rng):
    """Long members (LONG_SIZES), strand handling left to the caller; plus one ladder whose member + template exceed the old
    ~61 000-base LDS bound with both under 32768 bases."""
    cases = []
    for i, Lm in enumerate(LONG_SIZES):
        truth = rand_seq(rng, Lm)
        err = [0.0, 0.02, 0.05, 0.03][i]
        mem = [truth if err == 0 else dc.noisy(rng, truth, err) for _ in range(3)]
        mem[0] = truth[:Lm]                       # a member of exactly Lm bases
        cases.append((mem, 0))
    truth = rand_seq(rng, 31000)
    mem = [truth, dc.noisy(rng, truth, 0.02), dc.noisy(rng, truth[:30000], 0.03)]
    cases.append((mem, 0))
    return cases


def check_defined(lib, cases):
    """The oracle's consensus of every case; asserts that none is reference-undefined (return value >= 0)."""
    out = []
    for k, (mem, mx) in enumerate(cases):
        n, s = dc.ladder_call(lib.oracle_falcon_ladder, mem, mx)
        assert n >= 0, (k, len(mem), n)
        out.append(s)
    return out


def deep_chain(lib, wd):
    """An executable-level data set whose ladders are deep: synth_draft reads of one length (8 kb, 1-2 % errors each kind) at 100x
    over a 20 kb genome, and a graph whose one path runs through every read not contained in another, in genome order (the
    layout's own paths skip most of them: its ladders stay at ~20 members).  Writes the DB, .las, nominal.ini, G.max (every read
    active), the graph and - through `hinge draft-path` - G.edges.list into wd; runs the oracle's `hinge draft` and returns
    (FASTA, stdout, the member counts of its ladders as the printed lanes give them)."""
    import os
    import re

    from hinge_amd import clip, draft_path, synth_draft as sd
    d = sd.generate(sd.DraftSpec(genome_len=20_000, coverage=100.0, read_len=(8_000, 8_000), p_sub=0.01, p_ins=0.02, p_del=0.01, seed=71))
    sd.write_dataset(d, wd, "G")
    with open(os.path.join(wd, "nominal.ini"), "w") as f:
        f.write(dc.DRAFT_INI)
    with open(os.path.join(wd, "G.max"), "w") as f:
        f.write("".join("%d\n" % i for i in range(len(d.reads))))
    path, top = [], -1
    for i in sorted(range(len(d.reads)), key=lambda i: (d.g0[i], -d.g1[i])):
        if d.g1[i] > top:
            path.append(i)
            top = d.g1[i]
    g = clip.StrandGraph()
    rec = d.rec
    for x, y in zip(path, path[1:]):
        r = rec[np.nonzero((rec["aread"] == x) & (rec["bread"] == y))[0][0]]
        g.add_edge((x, int(d.strand[x])), (y, int(d.strand[y])), length=int(r["aepos"] - r["abpos"] + r["bepos"] - r["bbpos"]))
    clip.write_graphml(g, os.path.join(wd, "chain.graphml"))
    assert draft_path.main([wd, "G", os.path.join(wd, "chain.graphml")]) == 0
    fa, log = dc.run_oracle(lib, wd)
    # ladders as draft.cpp:540-556 makes them: the reads two consecutive lanes share
    lanes = [[int(a) for a in re.findall(r"\[(\d+) -?\d+\]", l)] for l in log.decode().split("\n") if l.startswith("[")]
    sizes = []
    for l1, l2 in zip(lanes, lanes[1:]):
        pos, n = 0, 0
        for r in l2:
            while l1[pos] != r and pos < len(l1) - 1:
                pos += 1
            n += l1[pos] == r
        sizes.append(n)
    return fa, log, sizes
