// overlap  ==  `hinge overlap READ_DB OUT.las [--k K] [--step S] [--window W] [--max-occ C] [--list L] [--max-partners N] [--min-hits H] [--block-bases B]
//                              [--max-stretches S] [--tile T] [--tile-stretches S] [--min-len M] [--max-err E] [--tspace T] [--band W] [--band-max W]`
// Not a program of the reference: it stands where the reference's run script calls DALIGNER (HPC.daligner + LAsort / LAmerge) on the
// read DB against itself to get the read-vs-read .las that `hinge filter` opens.  The candidates - "reads a and b, strand, about this
// diagonal" - are found by k-mer votes behind the C ABI (hinge_overlap_run, include/hinge_hip.h) and aligned by hinge_trace_local,
// both on the GPU; this file reads the DB, makes the candidate set symmetric, filters the records and writes the .las.
//   candidates  from all blocks; for every (a, b, comp) without its mirror, (b, a, comp) along the mirrored diagonal is added
//   alignment   in chunks of A reads (both DB slots hold the read DB; --band / --band-max and the scratch budget are the library's):
//               of every pair the candidate with aread < bread through hinge_trace_local; the pair's other record is the same
//               stretch with the end points swapped, aligned between them by hinge_trace_run - both records cover the same bases
//   filter      a record stays with both aligned lengths >= M (1000) and diffs / (aepos - abpos) <= E (0.30)
//   pairs       a pair is written only if both of its directed records stay
//   output      LAsort order (aread, bread, comp, abpos); trace values one byte up to tspace 125, as paf2las writes them
// --max-stretches S (1..8; default HINGE_OVERLAP_MAX_STRETCHES, else 1; 1 is the path above, call for call): up to S records per
// (aread, bread, comp), one per stretch - a repeat inside both reads, a circular genome's wrap
//   candidates  hinge_overlap_run_multi: up to S per (a, b, comp), by rounds of pick and suppress
//   canonical   a candidate (a, b, comp, diag) with a > b becomes (b, a, comp, mirrored diag)
//   merge       per (a < b, comp) the diagonals of both directions sorted; neighbours closer than `window` merge (single linkage);
//               a cluster's representative is its member found from a's side of the largest count - where a's side found it, the
//               diagonal that goes into the alignment is the one the path above would take, so a set without a second stretch gives
//               the same bytes -, without one its member of the largest count; ties to the smaller diagonal
//   alignment   every cluster projected as above - both reads whole along the representative's diagonal - through
//               hinge_trace_local; --min-len and --max-err as above
//   duplicates  the records of a key in the order (A length descending, abpos, bbpos): one is dropped if against a record already
//               kept their A ranges intersect by more than half the shorter one AND the smaller of |difference of the begin
//               diagonals bbpos - abpos| and |difference of the end diagonals bepos - aepos| is below `window` - the same alignment
//               reached from two bands, or a cut piece of it; a repeat's cross alignment lies a copy distance away on both ends
//   mirror      every kept record's mirror is the same stretch from read b through hinge_trace_run, tied to its origin by index;
//               a stretch is written only with both records
//   output      (aread, bread, comp, abpos, bbpos)
// --tile T (a power of two 64..8192, at most list * step; default HINGE_OVERLAP_TILE; neither: off, the path above call for call):
//   candidates  hinge_overlap_run_tiled: every query in half-overlapping tiles of T bases, so that a read of any length below 2^30
//               bases is sampled at --step (without it a read's step grows until it has at most --list positions, and a read of
//               2^20 or more bases is refused); everything behind the candidates is the path above
//   alignment   a record of a read of more than one tile that begins or ends inside both reads - the box along a tile's diagonal cut
//               it - runs through hinge_trace_local once more from its own end points with room for 1024 bases per side; the longer
//               of the two stays
//   Not together with --max-stretches above 1 (the usage, exit 1): --tile-stretches is the spelling for both.  Not claimed: that the
//   alignment of a placement of 2^20 or more bases succeeds - the option lifts the limit of the candidate search.
// --tile T --tile-stretches S (1..8; default HINGE_OVERLAP_TILE_STRETCHES, else 1; 1 is the --tile path above, call for call; needs a
// tile; not with --max-stretches above 1): up to S records per (aread, bread, comp) from tiles
//   candidates  hinge_overlap_run_tiled_multi: S rounds of pick and suppress in every tile, and again over the tiles' candidates
//   behind them both blocks above, in this order: canonical frame and merge, alignment, the tiled path's second run, the duplicate
//               rule, the mirrors tied by index, the output order of --max-stretches; both summary lines are printed
// Not claimed: two stretches on one diagonal; a weaker stretch inside the band that a stronger one's alignment settles in (after a
// TOUCHED widening both boxes may return the same optimum: the duplicate rule then leaves one); stretches of fewer than min-hits hits.
#include "host_common.h"

#include <unordered_set>

using namespace hh;

static void usage() {
    fprintf(stderr, "usage: overlap <read db> <out.las> [--k K] [--step S] [--window W] [--max-occ C] [--list L] [--max-partners N] [--min-hits H] [--block-bases B]\n"
                    "               [--max-stretches S] [--tile T] [--tile-stretches S] [--min-len M] [--max-err E] [--tspace T] [--band W] [--band-max W]\n"
                    "       read-vs-read overlaps of <read db> by k-mer votes and banded local alignment, as the .las `hinge filter` reads\n"
                    "       --max-stretches S: up to S (1..8) records per (aread, bread, strand), one per stretch; default HINGE_OVERLAP_MAX_STRETCHES, else 1\n"
                    "       --tile T: the candidates of every read from half-overlapping query tiles of T bases (a power of two 64..8192, at most list * step):\n"
                    "                 reads of any length below 2^30 bases at --step; default HINGE_OVERLAP_TILE, else off; not with --max-stretches above 1\n"
                    "       --tile-stretches S: with a tile, up to S (1..8) records per (aread, bread, strand) from the tiles; default HINGE_OVERLAP_TILE_STRETCHES, else 1;\n"
                    "                 not with --max-stretches above 1\n");
}

// both reads whole along the record-frame diagonal (bbpos - abpos), clamped to both; the rule of overlap_project (overlap_kernels.h)
static bool along(int alen, int blen, long long diag, int k, hinge_cns_alignment& r) {
    const long long ab = std::max(0ll, -diag), ae = std::min<long long>(alen, blen - diag);
    if (ae - ab < k) return false;
    r.abpos = (int)ab; r.aepos = (int)ae; r.bbpos = (int)(ab + diag); r.bepos = (int)(ae + diag);
    return true;
}

constexpr int TILE_EXTEND = 1024;     // --tile: the room per side of a record's second run (the widest default band: a diagonal further off is not followed anyway)

static inline uint64_t pair_key(int a, int b, int comp) { return ((uint64_t)(uint32_t)a << 33) | ((uint64_t)(uint32_t)b << 1) | (uint64_t)(comp & 1); }

int main(int argc, char* argv[]) {
    std::vector<std::string> pos;
    hinge_overlap_params prm;
    memset(&prm, 0, sizeof(prm));                   // the library's defaults (15, 2, 256, 64, 4096, 64, 6, 16 Mi)
    int min_len = 1000, tspace = 100, band = 0, band_max = 0;
    double max_err = 0.30;
    int stretches = 0;                              // 0: not given
    int tile = 0;                                   // 0: not given
    int tstretches = 0;                             // 0: not given
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto text = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "overlap: %s needs a value\n", name); usage(); exit(1); }
            return argv[++i];
        };
        auto val = [&](const char* name) -> long long {
            const long long v = atoll(text(name));
            if (v < 1) { fprintf(stderr, "overlap: %s needs a positive number\n", name); usage(); exit(1); }
            return v;
        };
        if (a == "--k") prm.k = (int32_t)val("--k");
        else if (a == "--step") prm.step = (int32_t)val("--step");
        else if (a == "--window") prm.window = (int32_t)val("--window");
        else if (a == "--max-occ") prm.max_occ = (int32_t)val("--max-occ");
        else if (a == "--list") prm.list = (int32_t)val("--list");
        else if (a == "--max-partners") prm.max_partners = (int32_t)val("--max-partners");
        else if (a == "--min-hits") prm.min_hits = (int32_t)val("--min-hits");
        else if (a == "--block-bases") prm.block_bases = (int64_t)val("--block-bases");
        else if (a == "--max-stretches") {
            stretches = (int)val("--max-stretches");
            if (stretches > HINGE_OVERLAP_MAX_STRETCHES_LIMIT) { fprintf(stderr, "overlap: --max-stretches needs a number in 1..8\n"); usage(); return 1; }
        }
        else if (a == "--tile") tile = (int)val("--tile");
        else if (a == "--tile-stretches") {
            tstretches = (int)val("--tile-stretches");
            if (tstretches > HINGE_OVERLAP_MAX_STRETCHES_LIMIT) { fprintf(stderr, "overlap: --tile-stretches needs a number in 1..8\n"); usage(); return 1; }
        }
        else if (a == "--min-len") min_len = (int)val("--min-len");
        else if (a == "--tspace") tspace = (int)val("--tspace");
        else if (a == "--band") band = (int)val("--band");
        else if (a == "--band-max") band_max = (int)val("--band-max");
        else if (a == "--max-err") {
            char* e = nullptr;
            const char* t = text("--max-err");
            max_err = strtod(t, &e);
            if (e == t || *e || !(max_err >= 0.0 && max_err <= 1.0)) { fprintf(stderr, "overlap: --max-err needs a number in [0, 1]\n"); usage(); return 1; }
        }
        else if (a.size() > 2 && a[0] == '-' && a[1] == '-') { fprintf(stderr, "overlap: unknown option %s\n", a.c_str()); usage(); return 1; }
        else pos.push_back(a);
    }
    if (pos.size() != 2 || tspace > 32767) { usage(); return 1; }
    if (stretches == 0) {
        const char* g = getenv("HINGE_OVERLAP_MAX_STRETCHES");
        stretches = (g && *g) ? atoi(g) : 1;
        if (stretches < 1 || stretches > HINGE_OVERLAP_MAX_STRETCHES_LIMIT) { fprintf(stderr, "overlap: HINGE_OVERLAP_MAX_STRETCHES needs a number in 1..8\n"); usage(); return 1; }
    }
    const bool tstretches_given = tstretches != 0;
    if (tstretches == 0) {
        const char* g = getenv("HINGE_OVERLAP_TILE_STRETCHES");
        tstretches = (g && *g) ? atoi(g) : 1;
        if (tstretches < 1 || tstretches > HINGE_OVERLAP_MAX_STRETCHES_LIMIT) { fprintf(stderr, "overlap: HINGE_OVERLAP_TILE_STRETCHES needs a number in 1..8\n"); usage(); return 1; }
    }
    if ((tstretches_given || tstretches > 1) && stretches > 1) { fprintf(stderr, "overlap: --tile-stretches and --max-stretches above 1 do not go together\n"); usage(); return 1; }
    const bool tmulti = tstretches > 1;             // the candidates from hinge_overlap_run_tiled_multi; behind them --max-stretches' blocks and --tile's
    const bool multi = stretches > 1 || tmulti;
    if (tmulti) stretches = tstretches;
    if (tile == 0) {
        const char* g = getenv("HINGE_OVERLAP_TILE");
        if (g && *g) tile = atoi(g);
        if (g && *g && tile < 1) { fprintf(stderr, "overlap: HINGE_OVERLAP_TILE needs a power of two in 64..8192\n"); usage(); return 1; }
    }
    if (tile != 0 && (tile < 64 || tile > HINGE_OVERLAP_TILE_MAX || (tile & (tile - 1)))) { fprintf(stderr, "overlap: --tile needs a power of two in 64..8192\n"); usage(); return 1; }
    if (tile != 0 && multi && !tmulti) { fprintf(stderr, "overlap: --tile and --max-stretches above 1 do not go together (--tile-stretches)\n"); usage(); return 1; }
    if (tile == 0 && (tstretches_given || tmulti)) { fprintf(stderr, "overlap: --tile-stretches needs a tile (--tile or HINGE_OVERLAP_TILE)\n"); usage(); return 1; }
    PhaseTimer tm("overlap");
    CtxInit gpu;
    gpu.start();
    ReadDB db;
    if (db.open(pos[0]) != 0) { fprintf(stderr, "overlap: Could not open database\n"); quit(1); }
    Mapped bps;
    const bool has = bps.open(db.dir + "/." + db.root + ".bps");
    if (!has && !db.rlen.empty()) { fprintf(stderr, "overlap: cannot read the .bps file of the database\n"); quit(1); }
    const int n_reads = (int)db.rlen.size();
    tm.mark("ingest");
    if (gpu.join() != HINGE_OK) { fprintf(stderr, "overlap: no usable GPU (%s)\n", gpu.ctx ? hinge_last_error(gpu.ctx) : "hinge_ctx_create failed"); quit(2); }
    hinge_ctx* ctx = gpu.ctx;
    auto die = [&](const char* what) { fprintf(stderr, "overlap: %s: %s\n", what, hinge_last_error(ctx)); quit(2); };
    for (int which = 0; which < 2; which++)         // both slots: hinge_trace_local aligns reads to reads
        if (hinge_consensus_set_db(ctx, which, n_reads, db.rlen.data(), db.boff.data(), bps.p, (int64_t)bps.n) != HINGE_OK) die("read DB");
    tm.mark("H2D bases");

    // ---- the candidates, made symmetric ------------------------------------------------------------------------------------------
    std::vector<int32_t> jstatus((size_t)std::max(2 * n_reads, 2));
    int64_t n_cand = 0;
    if ((tmulti ? hinge_overlap_run_tiled_multi(ctx, &prm, tile, stretches, jstatus.data(), nullptr, &n_cand)
         : multi ? hinge_overlap_run_multi(ctx, &prm, stretches, jstatus.data(), nullptr, &n_cand)
         : tile ? hinge_overlap_run_tiled(ctx, &prm, tile, jstatus.data(), nullptr, &n_cand)
                : hinge_overlap_run(ctx, &prm, jstatus.data(), nullptr, &n_cand)) != HINGE_OK) die("votes");
    std::vector<hinge_cns_alignment> cand((size_t)std::max<int64_t>(n_cand, 1));
    std::vector<int32_t> count((size_t)std::max<int64_t>(n_cand, 1)), diag((size_t)std::max<int64_t>(n_cand, 1));
    if (hinge_overlap_fetch(ctx, n_cand, cand.data(), count.data(), diag.data(), nullptr) != HINGE_OK) die("votes");
    cand.resize((size_t)n_cand);
    std::vector<int64_t> per_round((size_t)stretches, 0);
    if (multi) {
        std::vector<int32_t> round((size_t)std::max<int64_t>(n_cand, 1));
        if (hinge_overlap_fetch_round(ctx, n_cand, round.data()) != HINGE_OK) die("votes");
        for (int64_t x = 0; x < n_cand; x++) per_round[(size_t)round[(size_t)x]]++;
    }
    int64_t ost[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hinge_overlap_last_stats(ctx, ost);
    int64_t tst[4] = {0, 0, 0, 0};
    if (tile) (void)hinge_overlap_tile_stats(ctx, tst);
    tm.mark("index + votes");
    const int k = prm.k ? prm.k : (getenv("HINGE_OVERLAP_K") && *getenv("HINGE_OVERLAP_K") ? atoi(getenv("HINGE_OVERLAP_K")) : 15);
    const int window = prm.window ? prm.window : (getenv("HINGE_OVERLAP_WINDOW") && *getenv("HINGE_OVERLAP_WINDOW") ? atoi(getenv("HINGE_OVERLAP_WINDOW")) : 256);
    int64_t mirrored = 0, merged = 0;
    if (multi) {
        // ---- the canonical frame and the merge: per (a < b, comp) the diagonals of both directions, clustered by single linkage -----
        struct Canon { int a, b, comp; long long diag; int cnt, from_a; };
        std::vector<Canon> cn;
        cn.reserve((size_t)n_cand);
        for (int64_t x = 0; x < n_cand; x++) {
            const hinge_cns_alignment& r = cand[(size_t)x];
            const int alen = db.rlen[(size_t)r.aread], blen = db.rlen[(size_t)r.bread];
            if (r.aread < r.bread) cn.push_back(Canon{r.aread, r.bread, r.comp, diag[(size_t)x], count[(size_t)x], 1});
            else cn.push_back(Canon{r.bread, r.aread, r.comp, r.comp ? (long long)alen - blen + diag[(size_t)x] : -(long long)diag[(size_t)x], count[(size_t)x], 0});
        }
        std::sort(cn.begin(), cn.end(), [](const Canon& x, const Canon& y) {
            if (x.a != y.a) return x.a < y.a;
            if (x.b != y.b) return x.b < y.b;
            if (x.comp != y.comp) return x.comp < y.comp;
            if (x.diag != y.diag) return x.diag < y.diag;
            return x.from_a > y.from_a;
        });
        cand.clear();
        for (size_t x0 = 0; x0 < cn.size();) {
            size_t x1 = x0 + 1, best = x0;
            while (x1 < cn.size() && cn[x1].a == cn[x0].a && cn[x1].b == cn[x0].b && cn[x1].comp == cn[x0].comp && cn[x1].diag - cn[x1 - 1].diag < window) {
                const Canon &c = cn[x1], &q = cn[best];            // a's side first; then the largest count; then the smaller diagonal (the earlier one)
                if (c.from_a > q.from_a || (c.from_a == q.from_a && c.cnt > q.cnt)) best = x1;
                x1++;
            }
            merged += (int64_t)(x1 - x0) - 1;
            hinge_cns_alignment m;
            m.aread = cn[best].a; m.bread = cn[best].b; m.comp = cn[best].comp; m.tlen = 0; m.trace_off = 0;
            if (along(db.rlen[(size_t)m.aread], db.rlen[(size_t)m.bread], cn[best].diag, k, m)) cand.push_back(m);
            x0 = x1;
        }
    } else {
        std::unordered_set<uint64_t> have;
        have.reserve((size_t)n_cand * 2 + 16);
        for (const hinge_cns_alignment& r : cand) have.insert(pair_key(r.aread, r.bread, r.comp));
        for (int64_t x = 0; x < n_cand; x++) {
            const hinge_cns_alignment r = cand[(size_t)x];
            if (have.count(pair_key(r.bread, r.aread, r.comp))) continue;
            const int alen = db.rlen[(size_t)r.aread], blen = db.rlen[(size_t)r.bread];
            const long long md = r.comp ? (long long)alen - blen + diag[(size_t)x] : -(long long)diag[(size_t)x];      // the mirrored diagonal
            hinge_cns_alignment m;
            m.aread = r.bread; m.bread = r.aread; m.comp = r.comp; m.tlen = 0; m.trace_off = 0;
            if (!along(blen, alen, md, k, m)) continue;
            cand.push_back(m);
            mirrored++;
        }
        std::sort(cand.begin(), cand.end(), [](const hinge_cns_alignment& x, const hinge_cns_alignment& y) {
            if (x.aread != y.aread) return x.aread < y.aread;
            if (x.bread != y.bread) return x.bread < y.bread;
            return x.comp < y.comp;
        });
    }
    const int64_t n = (int64_t)cand.size();

    // ---- aligned in chunks of A reads.  The directed candidates with aread < bread go through hinge_trace_local; a record stays with
    //      both lengths >= M and diffs / (aepos - abpos) <= E.  Its pair's other record is the SAME stretch seen from read b: the end
    //      points swapped (in the comp frame: counted from the other end), aligned between them by hinge_trace_run - so both records of
    //      a pair cover the same bases, as the two records DALIGNER writes for one alignment do (`hinge draft` finds an edge's record by
    //      the sum of its two lengths, whichever direction the layout took it from) ----------------------------------------------------------
    int room = 50;                                  // no widened box reaches further than this beyond the given one (HINGE_TRACE_EXTEND)
    {
        const char* g = getenv("HINGE_TRACE_EXTEND");
        if (g && *g) room = std::max(atoi(g), 0);
    }
    const int64_t chunk_records = 1 << 18;
    struct Kept { hinge_cns_alignment r; int32_t diffs; int64_t toff; int64_t origin; };   // origin: the element of the round's input
    std::vector<Kept> kept;
    std::vector<uint16_t> ktrace;
    int64_t aligned = 0, asym = 0;
    auto by_key = [](const hinge_cns_alignment& x, const hinge_cns_alignment& y) {
        if (x.aread != y.aread) return x.aread < y.aread;
        if (x.bread != y.bread) return x.bread < y.bread;
        return x.comp < y.comp;
    };
    // one round: `in` (sorted by A read) through hinge_trace_local (local) or hinge_trace_run; what stays goes to `kept`, the rest is counted
    // ends / rm: hinge_trace_local's end rule and the room it may add per side (nullptr: the library's, `room`)
    auto align_round = [&](const std::vector<hinge_cns_alignment>& in, bool local, int64_t& dropped, const hinge_trace_ends* ends = nullptr, int rm_given = -1) {
        std::vector<hinge_cns_alignment> out;
        std::vector<uint16_t> trace;
        std::vector<int32_t> diffs, status, score;
        const int64_t n_in = (int64_t)in.size();
        const int rm = !local ? 0 : rm_given >= 0 ? rm_given : room;
        for (int64_t x0 = 0; x0 < n_in;) {
            int64_t x1 = std::min(n_in, x0 + chunk_records);
            while (x1 < n_in && in[(size_t)x1].aread == in[(size_t)x1 - 1].aread) x1++;        // whole A reads
            const int64_t m = x1 - x0;
            int64_t cap = 0;
            for (int64_t x = x0; x < x1; x++) cap += 2 * (int64_t)((in[(size_t)x].aepos + rm - 1) / tspace - std::max(in[(size_t)x].abpos - rm, 0) / tspace + 1);
            out.resize((size_t)m); trace.resize((size_t)std::max<int64_t>(cap, 1)); diffs.resize((size_t)m); status.resize((size_t)(2 * m)); score.resize((size_t)m);
            int64_t n_trace = 0;
            const int rc = local ? hinge_trace_local(ctx, m, in.data() + x0, tspace, band, band_max, ends, out.data(), trace.data(), cap, &n_trace, diffs.data(), status.data(), score.data())
                                 : hinge_trace_run(ctx, m, in.data() + x0, tspace, band, band_max, out.data(), trace.data(), cap, &n_trace, diffs.data(), status.data());
            if (rc != HINGE_OK) die("trace");
            for (int64_t x = 0; x < m; x++) {
                const hinge_cns_alignment& r = out[(size_t)x];
                if (status[(size_t)(2 * x)] != 0) { dropped++; continue; }
                aligned++;
                if (r.aepos - r.abpos < min_len || r.bepos - r.bbpos < min_len || (double)diffs[(size_t)x] > max_err * (double)(r.aepos - r.abpos)) { dropped++; continue; }
                kept.push_back(Kept{r, diffs[(size_t)x], (int64_t)ktrace.size(), x0 + x});
                ktrace.insert(ktrace.end(), trace.begin() + r.trace_off, trace.begin() + r.trace_off + r.tlen);
            }
            x0 = x1;
        }
    };
    std::vector<hinge_cns_alignment> first;
    for (const hinge_cns_alignment& r : cand)
        if (r.aread < r.bread) first.push_back(r);
    int64_t unaligned = 0, duplicates = 0;
    align_round(first, true, unaligned);
    int64_t reextended = 0;
    if (tile) {
        // ---- --tile: a tile's diagonal is that of 8 kb of the query, and the box - both reads whole along it - cuts an end whose own
        //      diagonal lies on its far side: the record then begins (ends) inside BOTH reads.  Such a record of a read of more than one
        //      tile runs again from its own end points with room for TILE_EXTEND bases per side (reads of one tile: nothing changes) ------
        std::vector<hinge_cns_alignment> again;
        std::vector<size_t> again_of;
        auto tiles_of = [&](int r) { return (long long)db.rlen[(size_t)r] - k + 1 > tile; };
        for (size_t x = 0; x < kept.size(); x++) {
            const hinge_cns_alignment& r = kept[x].r;
            const int alen = db.rlen[(size_t)r.aread], blen = db.rlen[(size_t)r.bread];
            if (!(tiles_of(r.aread) || tiles_of(r.bread))) continue;
            if (std::min(r.abpos, r.bbpos) == 0 && std::min(alen - r.aepos, blen - r.bepos) == 0) continue;
            hinge_cns_alignment m = r;
            m.tlen = 0; m.trace_off = 0;
            again.push_back(m);
            again_of.push_back(x);
        }
        if (!again.empty()) {
            std::vector<Kept> k1;
            std::vector<uint16_t> t1;
            k1.swap(kept); t1.swap(ktrace);
            const int64_t aligned1 = aligned;
            int64_t not_better = 0;
            hinge_trace_ends e;
            e.extend = TILE_EXTEND; e.match = 0; e.diff = 0; e.min_score = 0;
            align_round(again, true, not_better, &e, TILE_EXTEND);
            aligned = aligned1;
            for (const Kept& q : kept) {                // (a record the second run dropped stays as the first run left it)
                Kept& o = k1[again_of[(size_t)q.origin]];
                if (q.r.aepos - q.r.abpos < o.r.aepos - o.r.abpos) continue;
                const int64_t origin = o.origin;
                o = q;
                o.origin = origin;
                o.toff = (int64_t)t1.size();
                t1.insert(t1.end(), ktrace.begin() + q.toff, ktrace.begin() + q.toff + q.r.tlen);
                reextended++;
            }
            kept.swap(k1); ktrace.swap(t1);
        }
    }
    if (multi) {
        // ---- duplicates: per key in the order (A length descending, abpos, bbpos), against the records already kept ------------------
        std::sort(kept.begin(), kept.end(), [&](const Kept& x, const Kept& y) {
            if (by_key(x.r, y.r) || by_key(y.r, x.r)) return by_key(x.r, y.r);
            const int lx = x.r.aepos - x.r.abpos, ly = y.r.aepos - y.r.abpos;
            if (lx != ly) return lx > ly;
            if (x.r.abpos != y.r.abpos) return x.r.abpos < y.r.abpos;
            if (x.r.bbpos != y.r.bbpos) return x.r.bbpos < y.r.bbpos;
            return x.origin < y.origin;
        });
        std::vector<Kept> uniq;
        size_t key0 = 0;                            // where the current key's kept records begin in uniq
        for (const Kept& q : kept) {
            if (!uniq.empty() && (by_key(uniq.back().r, q.r) || by_key(q.r, uniq.back().r))) key0 = uniq.size();
            bool dup = false;
            for (size_t u = key0; u < uniq.size() && !dup; u++) {
                const hinge_cns_alignment &r = q.r, &o = uniq[u].r;
                const long long inter = (long long)std::min(r.aepos, o.aepos) - std::max(r.abpos, o.abpos);
                const long long near = std::min(std::llabs(((long long)r.bbpos - r.abpos) - ((long long)o.bbpos - o.abpos)), std::llabs(((long long)r.bepos - r.aepos) - ((long long)o.bepos - o.aepos)));
                dup = 2 * inter > std::min(r.aepos - r.abpos, o.aepos - o.abpos) && near < window;
            }
            if (dup) duplicates++;
            else uniq.push_back(q);
        }
        kept.swap(uniq);
    }
    const size_t n_first = kept.size();
    std::vector<hinge_cns_alignment> second;
    second.reserve(kept.size());
    for (const Kept& q : kept) {
        const hinge_cns_alignment& r = q.r;
        const int alen = db.rlen[(size_t)r.aread], blen = db.rlen[(size_t)r.bread];
        hinge_cns_alignment m;
        m.aread = r.bread; m.bread = r.aread; m.comp = r.comp; m.tlen = 0; m.trace_off = 0;
        if (!r.comp) { m.abpos = r.bbpos; m.aepos = r.bepos; m.bbpos = r.abpos; m.bepos = r.aepos; }
        else { m.abpos = blen - r.bepos; m.aepos = blen - r.bbpos; m.bbpos = alen - r.aepos; m.bepos = alen - r.abpos; }
        second.push_back(m);
    }
    std::vector<size_t> order;                      // the elements of kept that are written, in the file's order
    if (multi) {
        // ---- the mirrors, tied to their origins by index: second[v] is the mirror of kept[perm[v]]; a stretch is written with both ------
        std::vector<size_t> perm(second.size());
        for (size_t v = 0; v < perm.size(); v++) perm[v] = v;
        std::sort(perm.begin(), perm.end(), [&](size_t x, size_t y) { return by_key(second[x], second[y]) || (!by_key(second[y], second[x]) && x < y); });
        std::vector<hinge_cns_alignment> sorted_second(second.size());
        for (size_t v = 0; v < perm.size(); v++) sorted_second[v] = second[perm[v]];
        align_round(sorted_second, false, asym);
        for (size_t v = n_first; v < kept.size(); v++) {
            order.push_back(perm[(size_t)kept[v].origin]);
            order.push_back(v);
        }
        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
            const hinge_cns_alignment &u = kept[x].r, &w = kept[y].r;
            if (by_key(u, w) || by_key(w, u)) return by_key(u, w);
            if (u.abpos != w.abpos) return u.abpos < w.abpos;
            if (u.bbpos != w.bbpos) return u.bbpos < w.bbpos;
            return x < y;
        });
    } else {
        std::sort(second.begin(), second.end(), by_key);
        align_round(second, false, asym);
        std::sort(kept.begin(), kept.end(), [&](const Kept& x, const Kept& y) { return by_key(x.r, y.r); });
    }
    tm.mark("align + trace");

    // ---- a pair only with both of its directed records; the .las in LAsort order (aread, bread, comp, abpos: one record per key) ---------
    if (!multi) {
        std::unordered_set<uint64_t> stay;
        stay.reserve(kept.size() * 2 + 16);
        for (const Kept& q : kept) stay.insert(pair_key(q.r.aread, q.r.bread, q.r.comp));
        for (size_t x = 0; x < kept.size(); x++)
            if (stay.count(pair_key(kept[x].r.bread, kept[x].r.aread, kept[x].r.comp))) order.push_back(x);
    }
    const int64_t written = (int64_t)order.size();
    FILE* fo = fopen(pos[1].c_str(), "wb");
    if (!fo) { fprintf(stderr, "overlap: cannot write %s\n", pos[1].c_str()); quit(1); }
    const int32_t ts32 = tspace;
    fwrite(&written, 8, 1, fo);
    fwrite(&ts32, 4, 1, fo);
    const int tbytes = tspace <= 125 ? 1 : 2;
    std::vector<uint8_t> tb;
    std::vector<char> has_record((size_t)std::max(n_reads, 1), 0);
    for (const size_t at : order) {
        const Kept& q = kept[at];
        const hinge_cns_alignment& r = q.r;
        has_record[(size_t)r.aread] = 1;
        uint8_t rec[40];
        memset(rec, 0, sizeof(rec));
        const int32_t v[9] = {r.tlen, q.diffs, r.abpos, r.bbpos, r.aepos, r.bepos, r.comp ? 1 : 0, r.aread, r.bread};
        memcpy(rec, v, 36);
        fwrite(rec, 40, 1, fo);
        tb.resize((size_t)r.tlen * (size_t)tbytes);
        for (int t = 0; t < r.tlen; t++) {
            const uint16_t val = ktrace[(size_t)q.toff + (size_t)t];
            if (tbytes == 1) tb[(size_t)t] = (uint8_t)val;
            else { tb[(size_t)2 * t] = (uint8_t)(val & 0xff); tb[(size_t)2 * t + 1] = (uint8_t)(val >> 8); }
        }
        if (!tb.empty()) fwrite(tb.data(), 1, tb.size(), fo);
    }
    if (fclose(fo) != 0) { fprintf(stderr, "overlap: cannot write %s\n", pos[1].c_str()); quit(1); }
    int64_t lonely = 0;
    for (int r = 0; r < n_reads; r++) lonely += !has_record[(size_t)r];
    if (multi) {
        std::string rounds;
        for (int r = 0; r < stretches; r++) rounds += (r ? " + " : "") + std::to_string((long long)per_round[(size_t)r]);
        printf("overlap: %s %d: %s candidates per round, %lld merged into clusters, %lld clusters, %lld duplicates dropped\n", tmulti ? "--tile-stretches" : "--max-stretches", stretches, rounds.c_str(), (long long)merged,
               (long long)n, (long long)duplicates);
    }
    if (tile)
        printf("overlap: --tile %d: %lld tile(s), %lld job(s) of more than one, the largest tile kept %lld hit(s), %lld reduce launch(es); %lld record(s) extended by a second run\n", tile, (long long)tst[0], (long long)tst[1],
               (long long)tst[2], (long long)tst[3], (long long)reextended);
    printf("overlap: %d reads, %lld job(s) in %lld batch(es) over %lld block(s); %lld candidates, %lld mirrored, %lld aligned, %lld written, %lld dropped for asymmetry; index %lld entries (%lld codes dropped by max-occ)\n",
           n_reads, (long long)ost[0], (long long)ost[1], (long long)ost[2], (long long)n_cand, (long long)mirrored, (long long)aligned, (long long)written, (long long)asym, (long long)ost[3],
           (long long)ost[4]);
    fprintf(stderr, "overlap: %lld job(s) with dropped hits (OVERFLOW), %lld job(s) with dropped partners (TRUNCATED), %lld read(s) without any overlap\n", (long long)ost[5], (long long)ost[6],
            (long long)lonely);
    tm.mark("write");
    return finish(ctx, tm, 0);
}
