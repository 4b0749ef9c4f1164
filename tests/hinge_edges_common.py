"""Hand-built pile-ups that sit on the thresholds of the hinge calling (hinge_amd/csrc/hinge_call_kernel.h, k_hinge_exact), shared by
tests/test_hinge_edges.py (the model against the oracle, on the CPU) and tests/test_hinge_edges_gpu.py (every route of the kernels
against the model).  TEST INFRASTRUCTURE.

A part is written as DB + .las (formats.write_db / write_las) and read back (read_las, pileups_from_las): the model, the oracle
program and the kernels see one and the same part.

  partner reads   20 000 bases, 30 overlaps over their whole length each: mask (320, 19 680), no annotation.  There are more of them
                  than case reads, so the coverage median - MIN_COV = 9 - is theirs (the overflow part pins it with `ec`).
  case reads      20 000 bases.  30 overlaps over [0, 20 000]; 15 "gate extras" over [0, 3000 + 97 k] so that the fp32 end-coverage
                  gate does not skip the read; per SITE (one annotation) the supporters, the fillers that carry the coverage step
                  past the annotation threshold without supporting (R = 100 <= theta); padding up to the pile-up size asked for.
                  The pile-up is in the order of its B reads, as a .las is: B = position * partners // n.
  last read       one more partner: .hinges.txt stops before a part's last read.

A site of type -1 at p (a multiple of 40; 12 000, 13 000, ...) has supporters [f, p + near], near = 20.  A supporter is written as
(d, sec): d = f - mask_lo, its distance from the mask edge (d < BIN: the scan's first branch), sec its overhang on the far side
(sec < theta: category 2, > theta: category 3, == theta: category 0).  A site of type +1 at q (7960, 6960, ...) is the mirror image:
supporters [q + near, mask_hi - d], the roles of L and R swapped, gate extras at the tail.  B spans, partner mask (320, 19 680):
  form X = (320 + sec, 19 680 - big)     form Y = (320 + big, 19 680 - sec)      big = the supporting overhang, 4680 + u by default
  type -1: uncomplemented X, complemented Y;   type +1: uncomplemented Y, complemented X.
`u` shortens the B span: it sets the overlap's length sum - the key of the pile-up sort - without touching f, sec or the support.
With ties=False the supporters of a site get pairwise different length sums, with ties=True u is what the case says (0: supporters
of one (d, sec) tie)."""
import os
from dataclasses import dataclass, field

import numpy as np

import spec_model
import wide_keys_common as wk

RLEN = 20000
MLO, MHI = 320, 19680
TH = 300
C2, C0, C3 = 0, 300, 1000          # sec of the scan's categories 2, 0 (neither branch), 3


def params(kind="shipped"):
    """shipped: utils/nominal.ini.  low: SUP 3, PIL 3, UNB 2, tolerance 60.  tiny: low, and an annotation threshold of 4, MIN_COV 1
    (ec = 3) and a no-hinge region of 2000, so that a pile-up of 16 overlaps carries an annotation inside its mask and passes the gate."""
    from hinge_amd.config import default_filter_params
    p = default_filter_params()
    if kind in ("low", "tiny"):
        p.hinge_min_support, p.hinge_bin_pileup, p.hinge_unbridged, p.hinge_tolerance = 3, 3, 2, 60
    if kind == "tiny":
        p.min_repeat_annotation, p.min_cov, p.est_cov, p.no_hinge_region = 4, 1, 3, 2000
    return p


def ini_text(p):
    return ("[filter]\nlength_threshold = 1000;\naln_threshold = 1000;\nmin_cov = %d;\ncut_off = %d;\ntheta = %d;\nec = %d;\n"
            "min_repeat_annotation_threshold = %d;\nhinge_min_support = %d;\nhinge_min_pileup = %d;\nhinge_unbridged = %d;\n"
            "hinge_tolerance_length = %d;\nno_hinge_region = %d;\n" % (p.min_cov, p.cut_off, p.theta, p.est_cov, p.min_repeat_annotation, p.hinge_min_support,
                                                                    p.hinge_bin_pileup, p.hinge_unbridged, p.hinge_tolerance, p.no_hinge_region))


@dataclass
class Sup:
    d: int
    sec: int
    comp: int = 0
    near: int = 20
    big: int = None       # the supporting overhang (None: 4680 + u)
    u: int = 0


def S(d, sec, k=1, **kw):
    return [Sup(d, sec, **kw) for _ in range(k)]


@dataclass
class Site:
    typ: int
    sups: list
    fillers: int = None   # None: as many as bring the coverage step to 23
    ties: bool = False
    idx: int = 0          # which of the read's sites of this type (1000 bases apart)

    @property
    def pos(self):
        return 12000 + 1000 * self.idx if self.typ == -1 else 7960 - 1000 * self.idx


@dataclass
class Case:
    name: str
    sites: list
    n: int = None         # pile-up size (padding); None: what the rows come to
    at: list = None       # pile-up positions of the first site's supporters (None: behind the base rows, in order)
    base: int = 30
    extras: int = 15
    expect: dict = field(default_factory=dict)     # facts the CPU test holds the case to


def _bspan(typ, s):
    big = s.big if s.big is not None else 4680 + s.u
    x = (MLO + s.sec, MHI - big)
    y = (MLO + big, MHI - s.sec)
    return (x if s.comp == 0 else y) if typ == -1 else (y if s.comp == 0 else x)


def _aspan(site, d, near):
    return (MLO + d, site.pos + near) if site.typ == -1 else (site.pos + near, MHI - d)


def _detie(site):
    """u per supporter such that the supporters of the site have pairwise different length sums."""
    seen = set()
    for s in site.sups:
        if s.big is not None:
            b = _bspan(site.typ, s)
            a = _aspan(site, s.d, s.near)
            seen.add(a[1] - a[0] + b[1] - b[0])
    for s in site.sups:
        if s.big is not None:
            continue
        while True:
            a, b = _aspan(site, s.d, s.near), _bspan(site.typ, s)
            key = a[1] - a[0] + b[1] - b[0]
            if key not in seen:
                seen.add(key)
                break
            s.u += 1


def case_rows(case):
    """The pile-up of one case read in .las order: [(ab, ae, bb, be, comp)]."""
    head = case.sites[0].typ == -1
    other, first = [], []
    for j in range(case.base):
        other.append((0, RLEN, 0, RLEN - 7 * (j % 5), 0))
    for k in range(case.extras):
        other.append(((0, 3000 + 97 * k) if head else (RLEN - 3000 - 97 * k, RLEN)) + (0, RLEN, 0))
    for si, site in enumerate(case.sites):
        if not site.ties:
            _detie(site)
        rows = [_aspan(site, s.d, s.near) + _bspan(site.typ, s) + (s.comp,) for s in site.sups]
        (first if si == 0 and case.at is not None else other).extend(rows)
        nf = site.fillers if site.fillers is not None else max(0, 23 - sum(1 for s in site.sups if s.near == 20))
        for t in range(nf):
            a = (6000 + 40 * t, site.pos + 20) if site.typ == -1 else (site.pos + 20, 14000 - 40 * t)
            other.append(a + _bspan(site.typ, Sup(0, 0, big=100)) + (0,))
    n = case.n if case.n is not None else len(other) + len(first)
    assert n >= len(other) + len(first), (case.name, n, len(other) + len(first))
    for j in range(n - len(other) - len(first)):
        other.append((0, RLEN, 0, RLEN - 1 - j % 977, j & 1))       # padding: whole length, many length ties
    if not first:
        return other
    at = dict(zip(case.at, first))
    assert len(at) == len(first) and max(at) < n
    it = iter(other)
    return [at[k] if k in at else next(it) for k in range(n)]


@dataclass
class Part:
    name: str
    rlen: np.ndarray
    cols: tuple              # (rlen, row_ptr, a_span, b_span, b_flag): what wide_keys_common.model and the kernels take
    r0: int
    r1: int
    read_of: dict            # case name -> read id
    cases: dict              # case name -> Case
    fp: object
    n_partners: int
    dir: str


def build_part(name, cases, fp, wd, n_partners=None):
    """Writes the part under wd (G.db, G.las, nominal.ini) and reads it back."""
    from hinge_amd import formats
    NP = n_partners if n_partners is not None else max(40, len(cases) + 2)
    n_reads = NP + len(cases) + 1
    cols = []          # per read: int array [k, 7] aread bread ab ae bb be comp
    for k in list(range(NP)) + [n_reads - 1]:
        b = np.sort((k % NP + 1 + np.arange(30)) % NP)          # (NP > 30: never k itself)
        r = np.zeros((len(b), 7), np.int64)
        r[:, 0], r[:, 1], r[:, 3], r[:, 5] = k, b, RLEN, RLEN
        cols.append(r)
    read_of = {}
    for c, case in enumerate(cases):
        rows = np.array(case_rows(case), np.int64)
        r = np.zeros((len(rows), 7), np.int64)
        r[:, 0] = NP + c
        r[:, 1] = np.arange(len(rows)) * NP // len(rows)
        r[:, 2:7] = rows[:, [0, 1, 2, 3, 4]]
        cols.append(r)
        assert case.name not in read_of, case.name
        read_of[case.name] = NP + c
    rows = np.concatenate(cols)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    assert ((rows[:, 2] >= 0) & (rows[:, 2] < rows[:, 3]) & (rows[:, 3] <= RLEN) & (rows[:, 4] >= 0) & (rows[:, 4] < rows[:, 5]) & (rows[:, 5] <= RLEN)).all()
    rlen = np.full(n_reads, RLEN, np.int32)
    rec = np.zeros(len(rows), dtype=formats.LAS_REC_DTYPE)
    comp = rows[:, 6]
    rec["diffs"] = (rows[:, 3] - rows[:, 2]) // 8
    rec["abpos"], rec["aepos"] = rows[:, 2], rows[:, 3]
    rec["bbpos"] = np.where(comp == 1, RLEN - rows[:, 5], rows[:, 4])       # a complemented overlap is stored in the complemented B frame
    rec["bepos"] = np.where(comp == 1, RLEN - rows[:, 4], rows[:, 5])
    rec["flags"] = comp.astype(np.uint32)
    rec["aread"], rec["bread"] = rows[:, 0], rows[:, 1]
    os.makedirs(wd, exist_ok=True)
    formats.write_db(os.path.join(wd, "G"), rlen)
    formats.write_las(os.path.join(wd, "G.las"), formats.LasRecords(tspace=100, rec=rec, trace=np.zeros(0, np.uint8), trace_off=np.zeros(len(rows) + 1, np.int64)))
    with open(os.path.join(wd, "nominal.ini"), "w") as f:
        f.write(ini_text(fp))
    rl = formats.read_db_index(os.path.join(wd, "G"))["rlen"]
    recs = formats.read_las(os.path.join(wd, "G.las"))
    pile = formats.pileups_from_las(recs, rl)
    assert np.array_equal(rl, rlen) and pile.n_ovl == len(rows) and int(recs.rec["aread"][0]) == 0 and int(recs.rec["aread"][-1]) == n_reads - 1
    return Part(name, rlen, (rlen, pile.row_ptr, pile.a_span, pile.b_span, pile.b_flag), 0, n_reads - 1, read_of, {c.name: c for c in cases}, fp, NP, wd)


# ---- the model and the facts --------------------------------------------------------------------------------------------------

def supporters(part, mask, i, p, t, P):
    """[(f, sec, length sum, pile-up position)] of annotation (p, t) on read i, in .las order: the rule of spec_model.filter_part."""
    rlen, row_ptr, a_span, b_span, b_flag = part.cols
    s, e = int(row_ptr[i]), int(row_ptr[i + 1])
    out = []
    for k in range(s, e):
        ab, ae, bb, be = int(a_span[k, 0]), int(a_span[k, 1]), int(b_span[k, 0]), int(b_span[k, 1])
        near = ae if t == -1 else ab
        if not (p - P["TOL"] < near < p + P["TOL"]):
            continue
        mf, msd = (int(v) for v in mask[int(b_flag[k] & 0x7FFFFFFF)])
        R, L = max(msd - be, 0), max(bb - mf, 0)
        if b_flag[k] >> 31:
            R, L = L, R
        if t == -1 and R > P["TH"]:
            out.append((ab, L, ae - ab + be - bb, k - s))
        if t == 1 and L > P["TH"]:
            out.append((ae, R, ae - ab + be - bb, k - s))
    return out


def _cat(sec, P):
    return 2 if sec < P["TH"] else 3 if sec > P["TH"] else 0


def anno_facts(part, m, i, p, t, P):
    sup = supporters(part, m["mask"], i, p, t, P)
    sign = 1 if t == -1 else -1
    edge = int(m["mask"][i][0] if t == -1 else m["mask"][i][1])
    g = [sign * (f - edge) for f, _, _, _ in sup]          # the kernels' scan-ascending form, relative to the mask edge
    near_end = sum(1 for x in g if x < P["BIN"])
    answers = []
    for first in (2, 3):         # every tie group category-2-first, then category-3-first; category 0 between them
        rank = {first: 0, 0: 1, 5 - first: 2}
        x = sorted(sup, key=lambda v: (sign * v[0], rank[_cat(v[1], P)]))
        answers.append(spec_model.hinge_scan([(v[0], v[1]) for v in x], edge, sign, P))
    lens = [v[2] for v in sup]
    return dict(support=len(sup), near_end=near_end, span=(max(g) - min(g)) if g else 0, order_matters=len(sup) >= P["SUP"] and answers[0] != answers[1],
                undecided=len(sup) > P["SUP"] and near_end <= P["UNB"], len_tie=len(set(lens)) < len(lens), at=[v[3] for v in sup],
                hinge=(p, t) in m["hinges"][i])


def model(part, params, oracle_lib, with_facts=True):
    """wide_keys_common.model on the part, and per case read the facts the tests hold it to: facts[name] = dict(n, annos = [(p, t)],
    gated, a = [anno_facts per annotation])."""
    m = wk.model(part.cols, params, oracle_lib)
    P = wk.model_params(params)
    row_ptr = part.cols[1]
    facts = {}
    for name, i in (part.read_of.items() if with_facts else ()):
        facts[name] = dict(n=int(row_ptr[i + 1] - row_ptr[i]), annos=list(m["annos"][i]), gated=m["gated"][i],
                           a=[anno_facts(part, m, i, p, t, P) for (p, t) in m["annos"][i]])
    m["facts"] = facts
    return m


# ---- the named cases ----------------------------------------------------------------------------------------------------------

def slice_len(n):
    return ((n + 255) // 256) * 64


def _core(BIN=200, UNB=6, PIL=7, extra=0, tie=False, first=2, comp=0):
    """A supporter list the tie order decides: UNB first-branch supporters, one tie group behind BIN holding a category-2 and a
    category-3 member, PIL - 1 category-0 followers inside BIN of it, `extra` category-0 elements further out.  Category 2 first:
    considered = UNB + 1, unbridged.  Category 3 first: 1 + 1 + (PIL - 1) > PIL, bridged.
    tie: the two members have one length sum (the pile-up sort decides their order); else `first` has the larger one."""
    d = BIN + 300
    sups = [Sup(10 * i, C2, comp) for i in range(UNB)]
    sups += [Sup(d, C2, comp, u=1000 if tie else (0 if first == 2 else 1500)), Sup(d, C3, comp)]
    sups += [Sup(d + 10 + 10 * i, C0, comp) for i in range(PIL - 1)]
    sups += [Sup(d + BIN + 50 + 3 * i, C0, comp) for i in range(extra)]
    return sups


def _pair_positions(n, k, hole=None):
    """k pile-up positions of a pile-up of n: the first and last position of every non-empty slice (not of slice `hole`), the rest
    just behind the first."""
    q = slice_len(n)
    pos = []
    for w in range(4):
        lo, hi = w * q, min(n, (w + 1) * q)
        if lo < hi and w != hole:
            pos += [lo, hi - 1]
    pos = sorted(set(pos))
    w = next(w for w in range(4) if w != hole)
    x = w * q + 1
    while len(pos) < k:
        if x not in pos:
            pos.append(x)
        x += 1
    return sorted(pos)[:k] if len(pos) > k else sorted(pos)


def named_cases():
    """The cases of the shipped parameters (SUP 7, PIL 7, UNB 6, TOL 100, BIN 200, theta 300), each as type -1 uncomplemented, and
    the groups again as type +1 and with complemented supporters.  `expect`: hinge (one ungated annotation with that answer),
    support / near_end / span / n / order_matters / undecided / len_tie of the first annotation, annos (their number)."""
    B, out = 200, []

    def add(name, sups, expect, typ=-1, **kw):
        site_kw = {k: kw.pop(k) for k in ("fillers", "ties") if k in kw}
        out.append(Case(name, [Site(typ, sups, **site_kw)], expect=expect, **kw))

    for typ, comp, tag in ((-1, 0, ""), (1, 0, "_plus"), (-1, 1, "_comp"), (1, 1, "_plus_comp")):
        near = lambda k: [Sup(10 * i, C2, comp) for i in range(k)]      # noqa: E731  first-branch supporters
        # 1. support
        for k in (6, 7, 8):
            add("support_%d%s" % (k, tag), near(k), dict(support=k, hinge=k == 8), typ)
        for big in (TH, TH + 1):
            add("overhang_%d%s" % (big, tag), near(7) + [Sup(70, C2, comp, big=big)], dict(support=7 + (big > TH), hinge=big > TH), typ)
        for off in (-100, -99, 99, 100):
            add("window_%+d%s" % (off, tag), near(7) + [Sup(70, C2, comp, near=off)], dict(support=7 + (abs(off) < 100), hinge=abs(off) < 100), typ, fillers=16)
        # the same edge inside a scan: 2 first-branch + 4 category-2 behind BIN + 2 category-0 make 8; the supporter at the window's
        # edge is the FIRST of the pile-up (a gather that takes it shifts every slot) and, taken, makes considered = UNB + 1
        for off in (99, 100):
            sups = [Sup(B + 260, C2, comp, near=off)] + near(2) + [Sup(B + 210 + 10 * i, C2, comp) for i in range(4)] + [Sup(B + 300, C0, comp), Sup(B + 310, C0, comp)]
            add("window_scan_%+d%s" % (off, tag), sups, dict(support=8 + (off < 100), hinge=off < 100, undecided=True), typ, fillers=16,
                at=[0] + list(range(50, 58)), n=80)
        # 2. first branch
        for k in (6, 7):
            add("near_end_%d%s" % (k, tag), near(k) + [Sup(1000, C3, comp), Sup(2000, C3, comp)][:8 - k + (k == 6)], dict(near_end=k, hinge=k == 7), typ)
        for d in (B - 1, B):
            add("seventh_at_%d%s" % (d, tag), near(6) + [Sup(d, C3, comp), Sup(2000, C3, comp)], dict(near_end=6 + (d < B), hinge=d < B, support=8), typ)
        # 3. the unbridged stop: c1 first-branch supporters at d = 0 (f[0]), a category-2 element at BIN or BIN + 1
        for c1 in (5, 6):
            for d in (B, B + 1):
                sups = S(0, C2, c1, comp=comp) + [Sup(d, C2, comp)] + [Sup(3000 + 500 * i, C3, comp) for i in range(8 - c1 - 1)]
                add("unbridged_c%d_at_%d%s" % (c1 + 1, d, tag), sups, dict(near_end=c1, support=8, hinge=c1 == 6 and d == B + 1, undecided=True), typ)
        # 4. the bridged stop: a category-3 element, k followers inside BIN, a far category-2 element behind them
        for k in (6, 7):
            sups = [Sup(300, C3, comp)] + [Sup(310 + 10 * i, C2, comp) for i in range(k)] + [Sup(300 + B + 50, C2, comp)]
            add("bridged_%d_followers%s" % (k, tag), sups, dict(near_end=0, support=k + 2, hinge=k == 6, undecided=True), typ)
        for d in (B - 1, B):
            sups = [Sup(300, C3, comp)] + [Sup(310 + 10 * i, C2, comp) for i in range(6)] + [Sup(300 + d, C2, comp), Sup(300 + B + 50, C2, comp)]
            add("bridged_follower_at_%d%s" % (d, tag), sups, dict(support=9, hinge=d == B, undecided=True), typ)
        for k in (7, 8):       # the followers are the members of its own tie group
            add("bridged_own_group_%d%s" % (k, tag), S(300, C3, k, comp=comp) + [Sup(300 + B + 50, C2, comp)], dict(support=k + 1, hinge=k == 7, undecided=True, order_matters=False), typ, ties=True)
        # 5. sec == theta: category 0 counts among the followers (W) ...
        for k in (6, 7):
            sups = [Sup(300, C3, comp)] + [Sup(310 + 10 * i, C0, comp) for i in range(k)] + [Sup(300 + B + 10 + 10 * i, C2, comp) for i in range(6)]
            add("cat0_followers_%d%s" % (k, tag), sups, dict(hinge=k == 6, undecided=True), typ)
        for k in (6, 7):       # ... and not in `considered`
            sups = S(250, C0, 6, comp=comp) + [Sup(250 + B + 1 + 10 * i, C2, comp) for i in range(k)]
            add("cat0_not_considered_%d%s" % (k, tag), sups, dict(hinge=k == 7, support=6 + k, undecided=True), typ, ties=True)
        # 6. tie groups holding categories 2 and 3 behind BIN
        add("umust%s" % tag, near(5) + S(500, C2, 2, comp=comp) + [Sup(500, C3, comp)], dict(hinge=True, undecided=True, order_matters=False, support=8), typ, ties=True)
        add("bmust%s" % tag, near(1) + [Sup(500, C2, comp)] + S(500, C3, 2, comp=comp) + [Sup(510 + 10 * i, C3, comp) for i in range(6)] + [Sup(500 + B + 50, C2, comp)],
            dict(hinge=False, undecided=True, order_matters=False, support=11), typ, ties=True)
        for first in (2, 3):      # support 14 <= 16: the supporter sort is an insertion sort, the pile-up order of the pair decides
            add("order_first_%d%s" % (first, tag), _core(first=first, comp=comp), dict(order_matters=True, undecided=True, hinge=first == 2, support=14, len_tie=False), typ)
        add("order_tie%s" % tag, _core(tie=True, comp=comp), dict(order_matters=True, undecided=True, support=14, len_tie=True), typ, ties=True)
        for sup in (16, 17, 64, 65):      # the shortcut: no replay of the pile-up sort up to HC_SMALL supporters without a length tie
            for tie in (False, True):
                add("shortcut_%d%s%s" % (sup, "_tie" if tie else "", tag), _core(extra=sup - 14, tie=tie, comp=comp),
                    dict(order_matters=True, undecided=True, support=sup, len_tie=tie), typ, ties=tie)
    # 7. the light kernel's limits, 8. the 2 * CAP bins of k_hinge_call<CAP> (type -1, type +1, complemented)
    for typ, comp, tag in ((-1, 0, ""), (1, 0, "_plus"), (-1, 1, "_comp")):
        for sup in (1023, 1024):
            sups = _core(comp=comp) + [Sup(760 + 3 * i, C0, comp) for i in range(sup - 14)]
            add("light_%d%s" % (sup, tag), sups, dict(order_matters=True, undecided=True, support=sup), typ)
        # One bin of the light kernel's g2 | g3 << 10 | g0 << 20 word filled past 2^9, with a support of LIGHT_CAP = 1023 so that the
        # kernel does bin it.  1015 category-2 supporters at f[0] (not `far`: no stop), 7 more inside BIN, one behind BIN that stops
        # the scan unbridged.  A g2 field of nine bits would spill into g3: a category-3 member at f[0] with 7 followers - bridged.
        add("light_bin_1015_cat2%s" % tag, S(250, C2, 1015, comp=comp) + [Sup(260 + 10 * i, C2, comp) for i in range(7)] + [Sup(250 + B + 1, C2, comp)],
            dict(support=1023, undecided=True, hinge=True, near_end=0, order_matters=False), typ, ties=True)
        # The same for g3: 1022 category-3 supporters in one bin behind BIN.  (The tables cannot show a g3 field that is too narrow:
        # what spills lands in g0, which enters only the sum g, and 1022 followers are bridged with any of these counts.)
        add("light_bin_1022_cat3%s" % tag, [Sup(250, C2, comp)] + S(250 + B + 1, C3, 1022, comp=comp), dict(support=1023, undecided=True, hinge=False, near_end=0), typ, ties=True)
        # 10b. so dense at one f (here behind the no-hinge region) that the step UP is an annotation of the other type - it happens by
        # itself with 1022 supporters at one position; its own supporters are these 1022, tied at their other end
        add("light_dense_other_type%s" % tag, S(680, C3, 1022, comp=comp) + [Sup(680 + B + 1, C2, comp)], dict(annos=2), typ, ties=True)
        for span in (4095, 4096):      # the light kernel's 4096 bins, and 2 * CAP bins of k_hinge_call<2048>
            add("span_%d%s" % (span, tag), S(250, C2, 6, comp=comp) + [Sup(250 + span, C2, comp), Sup(250 + 100, C0, comp)], dict(span=span, hinge=True, undecided=True, support=8), typ, ties=True)
        for span in (8191, 8192):      # 2 * CAP bins of k_hinge_call<4096>: a pile-up beyond 2048
            add("span_%d_n2100%s" % (span, tag), S(250, C2, 6, comp=comp) + [Sup(250 + span, C2, comp), Sup(250 + 100, C0, comp)],
                dict(span=span, hinge=True, undecided=True, support=8, n=2100), typ, ties=True, n=2100)
    # 9. pile-up sizes: the tied pair, so that the replay sorts the whole pile-up
    for n in (255, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097):
        add("pile_%d" % n, _core(tie=True), dict(n=n, order_matters=True, undecided=True, len_tie=True), ties=True, n=n)
    add("pile_2049_plus_comp", _core(tie=True, comp=1), dict(n=2049, order_matters=True, undecided=True, len_tie=True), 1, ties=True, n=2049)
    for n in (256, 257, 513):
        for hole in (None, 1):
            at = _pair_positions(n, 14, hole)
            add("slices_%d%s" % (n, "" if hole is None else "_hole"), _core(tie=True), dict(n=n, order_matters=True, undecided=True, at=at), ties=True, n=n, at=at)
    at = _pair_positions(257, 14)
    add("slices_257_plus_comp", _core(tie=True, comp=1), dict(n=257, order_matters=True, undecided=True, at=at), 1, ties=True, n=257, at=at)
    # 10. several annotations per read: 2, 3 and 5, both types, decided by the count sweep and not
    opn = lambda t, i, **kw: Site(t, _core(**kw), ties=kw.get("tie", False), idx=i)      # noqa: E731
    cnt = lambda t, i, k, c=0: Site(t, [Sup(10 * j, C2, c) for j in range(k)], idx=i)            # noqa: E731
    brd = lambda t, i, k, c=0: Site(t, [Sup(300, C3, c)] + [Sup(310 + 10 * j, C2, c) for j in range(k)] + [Sup(550, C2, c)], idx=i)      # noqa: E731
    out.append(Case("annos_2", [opn(-1, 0, first=3), opn(-1, 1)], expect=dict(annos=2, open=2)))
    out.append(Case("annos_3", [opn(-1, 0), brd(-1, 1, 7), opn(1, 0, first=3)], extras=40, expect=dict(annos=3, open=3)))
    out.append(Case("annos_5", [cnt(-1, 0, 8), opn(-1, 1, tie=True), brd(-1, 2, 6), opn(1, 0), cnt(1, 1, 6)], extras=40, expect=dict(annos=5, open=3)))
    out.append(Case("annos_5_open", [opn(-1, 0), opn(-1, 1, first=3), brd(-1, 2, 7), opn(1, 0, tie=True), brd(1, 1, 6)], extras=40, expect=dict(annos=5, open=5)))
    out.append(Case("annos_5_comp", [cnt(-1, 0, 8, 1), opn(-1, 1, tie=True, comp=1), brd(-1, 2, 6, 1), opn(1, 0, comp=1), brd(1, 1, 7, 1)], extras=40, expect=dict(annos=5, open=4)))
    return out


def tiny_cases():
    """Pile-ups of 16 and 17 overlaps (params("tiny"): SUP 3, PIL 3, UNB 2, BIN 120, annotation threshold 4, MIN_COV 1).  std::sort of
    16 elements is an insertion sort: stable, so the pile-up order of a tied pair is its .las order."""
    out = []
    for n in (16, 17):
        for first in (2, 3):
            for tie in (False, True):
                sups = _core(BIN=120, UNB=2, PIL=3, extra=8, tie=tie, first=first)
                if tie and first == 3:
                    sups[2], sups[3] = sups[3], sups[2]       # .las order: the category-3 member in front
                out.append(Case("tiny_%d_first_%d%s" % (n, first, "_tie" if tie else ""), [Site(-1, sups, fillers=0, ties=tie)], n=n, base=2, extras=0,
                                expect=dict(n=n, support=14, order_matters=True, undecided=True, len_tie=tie)))
    return out


def drawn_cases(seed, BIN, UNB, n_cases=300, pad=None, lo=5, hi=40):
    """Case reads whose supporter lists are drawn from small alphabets that crowd the thresholds: d round BIN (the first branch) and
    round d0 + BIN (`far`, the followers' window), with repeats; categories 2, 2, 3, 0; both types, both strands."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_cases):
        typ = -1 if rng.integers(2) else 1
        k = int(rng.integers(lo, hi + 1))
        d0 = int(rng.choice([BIN - 1, BIN, BIN + 1, BIN + 40]))
        alpha = [d0, d0, d0 + 1, d0 + BIN - 1, d0 + BIN, d0 + BIN + 1, d0 + BIN + 2, d0 + 2 * BIN - 1, d0 + 2 * BIN, d0 + 2 * BIN + 1, d0 + 3 * BIN]
        n_near = int(rng.choice([0, 0, 1, UNB // 2, UNB - 1, UNB, UNB, UNB + 1]))        # first-branch supporters: round UNB
        sups = [Sup(int(rng.integers(0, BIN)), C2, int(rng.integers(2))) for _ in range(min(n_near, k))]
        for _ in range(k - len(sups)):
            sups.append(Sup(int(rng.choice(alpha)), int(rng.choice([C2, C2, C3, C0])), int(rng.integers(2)), u=int(rng.choice([0, 0, 1000, 37]))))
        order = rng.permutation(len(sups))
        sups = [sups[j] for j in order]
        n = None if pad is None else pad
        out.append(Case("drawn_%d_%d" % (seed, c), [Site(typ, sups, ties=True)], n=n))
    return out


def pack(part):
    """The packed hand-over's facts (capi.pack_spans) of the part."""
    from hinge_amd import capi
    return capi.pack_spans(part.cols[1], part.cols[2], part.rlen)


PARTS = ("named", "tiny", "drawn_shipped_1", "drawn_shipped_2", "drawn_low_1", "drawn_low_2")
OVERFLOW_READS, OVERFLOW_PILE = 4200, 205        # 5 * 4200 * 205 > 2^22 ints of arena, 4200 > 4096 queue entries


def make_part(name, wd):
    """The part of that name, written under wd.  "overflow": 4200 drawn case reads of 8 to 40 supporters (support > SUP: force_exact(1) queues every one)
    padded to 205 overlaps, 40 partners, MIN_COV pinned to 9;
    "overflow_queue": the same reads without the padding - they overflow the exact queue and NOT the arena, whose own rerun would
    otherwise hide a queue that is not grown by ec = 27 (so many deep case reads would move the coverage median)."""
    if name == "named":
        return build_part(name, named_cases(), params(), wd)
    if name == "tiny":
        return build_part(name, tiny_cases(), params("tiny"), wd)
    if name in ("overflow", "overflow_queue"):
        fp = params()
        fp.est_cov = 27
        pad = OVERFLOW_PILE if name == "overflow" else None
        return build_part(name, drawn_cases(3, 2 * fp.hinge_tolerance, fp.hinge_unbridged, n_cases=OVERFLOW_READS, pad=pad, lo=8), fp, wd, n_partners=40)
    _, kind, seed = name.split("_")
    fp = params(kind)
    return build_part(name, drawn_cases(int(seed), 2 * fp.hinge_tolerance, fp.hinge_unbridged), fp, wd)
