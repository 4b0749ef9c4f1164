"""The pile-up vote of `hinge consensus` in plain numpy/Python, from an alignment's indel list: getAlignmentTags' columns
(LAInterface.cpp:3822-3866), chop_end (consensus.cpp:27-45) and the counters of consensus.cpp:163-212.  The model of
tests/test_consensus_host.py for k_cns_columns' CnsCols and the nine count planes of k_cns_vote / k_cns_vote_tiles, and the base
calls of consensus.cpp:228-270 for tests/test_consensus_edges_gpu.py."""
import numpy as np


def columns(ab, ae, bb, indels, bseq):
    """The alignment's columns in order: (kind, apos, base) arrays.  kind 0: a column with an A base (apos, 0-based; base = the B
    base, or 4 where B has a gap); kind 1: an inserted B base in front of A position apos.  indels: 1-based positions, -(A position)
    for a gap in A, +(B position) for a gap in B; bseq: the B sequence in the alignment's frame (complemented when comp)."""
    kind, apos, base = [], [], []
    i, j = ab + 1, bb + 1
    for p in indels:
        p = int(p)
        if p < 0:
            while i != -p:
                kind.append(0); apos.append(i - 1); base.append(int(bseq[j - 1])); i += 1; j += 1
            kind.append(1); apos.append(i - 1); base.append(int(bseq[j - 1])); j += 1
        else:
            while j != p:
                kind.append(0); apos.append(i - 1); base.append(int(bseq[j - 1])); i += 1; j += 1
            kind.append(0); apos.append(i - 1); base.append(4); i += 1
    while i <= ae:
        kind.append(0); apos.append(i - 1); base.append(int(bseq[j - 1])); i += 1; j += 1
    return np.asarray(kind, np.int64), np.asarray(apos, np.int64), np.asarray(base, np.int64)


def chop_end(kind, chop=100):
    """(start, end, offset): the columns [start, end) vote; offset = A bases in front of column `start`."""
    n = len(kind)
    if n < 2 * chop + 10:
        return 0, n, 0
    start = chop
    while kind[start] == 1:
        start += 1
    return start, n - chop, int((kind[:start] == 0).sum())


def vote(planes, first, alen, kind, apos, base, start, end):
    """planes: int64 [9, positions of all contigs]; first: the contig's first position.  Planes 0-4: A C G T '-' of the columns with an
    A base, 5-8: A C G T of the inserted ones.  An inserted base behind the contig's last base has no position and is dropped."""
    k, a, b = kind[start:end], apos[start:end], base[start:end]
    np.add.at(planes, (b[k == 0], first + a[k == 0]), 1)
    ins = (k == 1) & (a < alen)
    np.add.at(planes, (5 + b[ins], first + a[ins]), 1)


def call(planes, draft):
    """One contig's string from its planes [9, alen] (consensus.cpp:228-270): the draft's base in lower case below depth 3; an inserted
    base where more than half the depth has one; the most frequent aligned symbol unless it is the gap.  Ties: the first of A C G T -."""
    out = []
    for j in range(len(draft)):
        sc, ib = planes[:5, j], planes[5:, j]
        depth = int(sc.sum())
        if depth < 3:
            out.append("acgt"[int(draft[j])])
            continue
        if int(ib.sum()) > depth // 2:
            out.append("ACGT"[int(np.argmax(ib))])
        mb = int(np.argmax(sc))
        if mb < 4:
            out.append("ACGT"[mb])
    return "".join(out)
