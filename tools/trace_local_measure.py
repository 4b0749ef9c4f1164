#!/usr/bin/env python
"""The two measured constants of `hinge paf2las --ends local` ("Local"), from the numpy model alone (no GPU):

    python tools/trace_local_measure.py minscore   # HINGE_TRACE_LOCAL_MIN_SCORE: the largest local score of seeded unrelated pairs of the
                                                   # bench's mean placement size (7128 bases) at band_max (W = 1024), scores 1 / 2; plus half
    python tools/trace_local_measure.py margin     # TRACE_LOCAL_MARGIN: planted alignments (alen 200-500, 6 % and 15 % errors, extend 50) whose
                                                   # true diagonal lies 24 .. 104 beside the centre line of a W = 64 band, either side, eight
                                                   # per offset: per margin, the worst miss of an end point among the cases that finish OK at W
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def minscore():
    import numpy as np
    import trace_local_common as lc
    scores = []
    for c0 in range(0, 16, 4):
        rng = np.random.default_rng([77, 7128, c0])
        pairs = [(rng.integers(0, 4, 7128, dtype=np.uint8), rng.integers(0, 4, 7128, dtype=np.uint8)) for _ in range(4)]
        scores += [b[0] for b in lc.fill_local(pairs, 1024)[2]]
        print("scores so far:", scores, flush=True)
    print("largest %d, plus half: %d" % (max(scores), max(scores) + max(scores) // 2))


def margin():
    import numpy as np
    import trace_common as tc
    import trace_local_common as lc
    W = 64
    rows = []
    for err in (0.06, 0.15):
        rng = np.random.default_rng([5, int(err * 100)])
        for off in range(W - 40, W + 41):
            for sign in (1, -1):
                for rep in range(8):
                    contig, read, given, truth = lc.planted(rng, int(rng.integers(200, 501)), err, 0, 0, flank=2 * off + 60)
                    # the planted alignment whole inside the box, its diagonal sign * off beside the box's centre line
                    box = lc.widen(lc.beside(truth, sign * off), len(contig), len(read), 50)
                    Ds, Cs, bests = lc.fill_local([tc.stretches([contig], [read], box)], W)
                    for m in range(1, 33):
                        st, cells, tr, df, sc = lc.local_of(Ds[0], Cs[0], bests[0], box[3], 100, W, 1, 2, lc.MIN_SCORE, m)
                        if st == tc.OK:
                            ends = (box[3] + cells[0], box[3] + cells[2], box[5] + cells[1], box[5] + cells[3])
                            rows.append((err, m, max(abs(a - b) for a, b in zip(ends, truth))))
    for err in (0.06, 0.15):
        for m in range(1, 33):
            ok = [r[2] for r in rows if r[0] == err and r[1] == m]
            print("%.0f %% errors, margin %2d: %4d of 1296 cases OK at W = 64, worst miss %s" % (err * 100, m, len(ok), max(ok) if ok else "-"))


if __name__ == "__main__":
    {"minscore": minscore, "margin": margin}[sys.argv[1]]()
