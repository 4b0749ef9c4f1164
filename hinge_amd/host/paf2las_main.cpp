// paf2las  ==  `hinge paf2las DRAFT_DB READ_DB PAF OUT.las [--band W] [--band-max W] [--tspace T] [--draft-names FASTA] [--read-names FASTA]
//                                [--ends given|refine|local] [--extend E] [--scores M,X] [--min-score S]`
// Not a program of the reference: it stands where demo/ecoli_demo/run.sh:30-37 runs HPC.daligner + LAmerge on (draft, reads) to get
// the draft-vs-reads .las WITH trace points that `hinge consensus` needs.  Input: placements as PAF, query = read, target =
// contig (what `hinge seed` writes and `minimap2 draft.fasta reads.fasta` prints).  The base-level alignment between the given
// end points and its trace points are computed behind the C ABI (hinge_trace_run, include/hinge_hip.h) on the GPU; this file reads the DBs and the PAF,
// resolves names, and writes the .las (align.h:98-110: the records `Read_Overlap` reads).
// --ends given (the default): the PAF's end points are exact (hinge_trace_run).  --ends refine: they are approximate - every
// placement is widened by up to E bases per side and the best-scoring stretch of its path is kept (hinge_trace_refine); the
// records carry the refined end points.  --ends local: the diagonal is approximate too (all four end points off independently) -
// the best local alignment inside the band of the widened box is kept (hinge_trace_local); --extend, --scores and --min-score apply.
#include "host_common.h"

#include <map>
#include <unordered_map>

using namespace hh;

static void usage() {
    fprintf(stderr, "usage: paf2las <draft db> <read db> <paf> <out.las> [--band W] [--band-max W] [--tspace T] [--draft-names FASTA] [--read-names FASTA]\n"
                    "               [--ends given|refine|local] [--extend E] [--scores M,X] [--min-score S]\n"
                    "       <paf>: placements with query = read, target = contig, e.g. from `hinge seed <draft db> <read db> <paf>` (then --ends local)\n");
}

// first word of every header of a FASTA file -> record index
static bool fasta_names(const std::string& path, std::unordered_map<std::string, int>& ids) {
    std::string t;
    if (!slurp_gz(path, t)) return false;
    int n = 0;
    size_t i = 0;
    while (i < t.size()) {
        size_t e = t.find('\n', i);
        if (e == std::string::npos) e = t.size();
        if (t[i] == '>') {
            size_t w = i + 1;
            while (w < e && !isspace((unsigned char)t[w])) w++;
            ids.emplace(t.substr(i + 1, w - i - 1), n++);
        }
        i = e + 1;
    }
    return true;
}

// get_id_from_string - 1 (LAInterface.cpp:4808-4819): the 1-based id between the first two '/'
static int id_between_slashes(const std::string& name) {
    const size_t s0 = name.find('/');
    if (s0 == std::string::npos) return -1;
    const size_t s1 = name.find('/', s0 + 1);
    if (s1 == std::string::npos || s1 - s0 - 1 >= 15 || s1 == s0 + 1) return -1;
    return atoi(name.substr(s0 + 1, s1 - s0 - 1).c_str()) - 1;
}

int main(int argc, char* argv[]) {
    std::vector<std::string> pos;
    int band = 0, band_max = 0, tspace = 100;
    std::string draft_names, read_names, ends_mode = "given";
    hinge_trace_ends ends = {-1, 0, 0, 0};          // the library's defaults (50; 1, 2; refine 1, local 24)
    bool ends_opts = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "paf2las: %s needs a value\n", name); usage(); exit(1); }
            return argv[++i];
        };
        if (a == "--band") band = atoi(val("--band"));
        else if (a == "--band-max") band_max = atoi(val("--band-max"));
        else if (a == "--tspace") tspace = atoi(val("--tspace"));
        else if (a == "--draft-names") draft_names = val("--draft-names");
        else if (a == "--read-names") read_names = val("--read-names");
        else if (a == "--ends") ends_mode = val("--ends");
        else if (a == "--extend") { ends.extend = atoi(val("--extend")); ends_opts = true; if (ends.extend < 0) { usage(); return 1; } }
        else if (a == "--scores") {
            int m = 0, x = 0;
            if (sscanf(val("--scores"), "%d,%d", &m, &x) != 2 || m < 1 || x < 1) { fprintf(stderr, "paf2las: --scores needs M,X (each 1..15)\n"); usage(); return 1; }
            ends.match = m; ends.diff = x; ends_opts = true;
        }
        else if (a == "--min-score") { ends.min_score = atoi(val("--min-score")); ends_opts = true; if (ends.min_score < 1) { usage(); return 1; } }
        else if (a.size() > 2 && a[0] == '-' && a[1] == '-') { fprintf(stderr, "paf2las: unknown option %s\n", a.c_str()); usage(); return 1; }
        else pos.push_back(a);
    }
    if (pos.size() != 4 || tspace <= 0 || tspace > 32767 || band < 0 || band_max < 0) { usage(); return 1; }
    if (ends_mode != "given" && ends_mode != "refine" && ends_mode != "local") { fprintf(stderr, "paf2las: --ends takes given or refine or local\n"); usage(); return 1; }
    const bool local = ends_mode == "local";
    const bool refine = ends_mode == "refine" || local;      // everything below that refined end points need
    if (ends_opts && !refine) { fprintf(stderr, "paf2las: --extend, --scores and --min-score belong to --ends refine and --ends local\n"); usage(); return 1; }
    PhaseTimer tm("paf2las");
    CtxInit gpu;
    gpu.start();
    ReadDB db1, db2;
    if (db1.open(pos[0]) != 0 || db2.open(pos[1]) != 0) { fprintf(stderr, "paf2las: Could not open database\n"); quit(1); }
    Mapped bps1, bps2;
    const bool has1 = bps1.open(db1.dir + "/." + db1.root + ".bps"), has2 = bps2.open(db2.dir + "/." + db2.root + ".bps");
    if ((!has1 && !db1.rlen.empty()) || (!has2 && !db2.rlen.empty())) { fprintf(stderr, "paf2las: cannot read the .bps file of a database\n"); quit(1); }
    const int n_contigs = (int)db1.rlen.size(), n_reads = (int)db2.rlen.size();
    std::unordered_map<std::string, int> ids_draft, ids_read;
    if (!draft_names.empty() && !fasta_names(draft_names, ids_draft)) { fprintf(stderr, "paf2las: cannot read %s\n", draft_names.c_str()); quit(1); }
    if (!read_names.empty() && !fasta_names(read_names, ids_read)) { fprintf(stderr, "paf2las: cannot read %s\n", read_names.c_str()); quit(1); }
    auto resolve = [](const std::string& name, bool by_file, const std::unordered_map<std::string, int>& ids) {
        if (!by_file) return id_between_slashes(name);
        auto it = ids.find(name);
        return it == ids.end() ? -1 : it->second;
    };

    // ---- the PAF: query = read, target = contig --------------------------------------------------------------------------------
    std::string t;
    if (!slurp_gz(pos[2], t)) { fprintf(stderr, "paf2las: cannot read %s\n", pos[2].c_str()); quit(1); }
    std::vector<hinge_cns_alignment> pl;
    {
        size_t i = 0;
        long long line = 0;
        while (i < t.size()) {
            size_t e = t.find('\n', i);
            if (e == std::string::npos) e = t.size();
            size_t le = e;
            if (le > i && t[le - 1] == '\r') le--;
            line++;
            if (le == i) { i = e + 1; continue; }                      // an empty line
            std::vector<std::string> f;
            size_t p0 = i;
            for (size_t k = i; k <= le; k++)
                if (k == le || t[k] == '\t') { f.push_back(t.substr(p0, k - p0)); p0 = k + 1; }
            i = e + 1;
            auto bad = [&](const char* why) { fprintf(stderr, "paf2las: %s line %lld: %s\n", pos[2].c_str(), line, why); quit(1); };
            if (f.size() < 9) bad("fewer than 9 columns");
            const int b = resolve(f[0], !read_names.empty(), ids_read), a = resolve(f[5], !draft_names.empty(), ids_draft);
            if (b < 0 || b >= n_reads) bad("unknown read (query) name");
            if (a < 0 || a >= n_contigs) bad("unknown contig (target) name");
            const long long qlen = atoll(f[1].c_str()), qs = atoll(f[2].c_str()), qe = atoll(f[3].c_str());
            const long long tlen = atoll(f[6].c_str()), ts = atoll(f[7].c_str()), te = atoll(f[8].c_str());
            if (qlen != db2.rlen[(size_t)b]) bad("the query length is not the read's length in the read DB");
            if (tlen != db1.rlen[(size_t)a]) bad("the target length is not the contig's length in the draft DB");
            if (f[4] != "+" && f[4] != "-") bad("the strand is neither + nor -");
            if (!(0 <= qs && qs < qe && qe <= qlen && 0 <= ts && ts < te && te <= tlen)) bad("coordinates outside their sequence, or an empty stretch");
            hinge_cns_alignment r;
            r.aread = a; r.bread = b; r.comp = f[4] == "-" ? 1 : 0;
            r.abpos = (int)ts; r.aepos = (int)te;
            r.bbpos = r.comp ? (int)(qlen - qe) : (int)qs;          // the complemented frame of a `-` line
            r.bepos = r.comp ? (int)(qlen - qs) : (int)qe;
            r.tlen = 0; r.trace_off = 0;
            pl.push_back(r);
        }
    }
    std::stable_sort(pl.begin(), pl.end(), [](const hinge_cns_alignment& x, const hinge_cns_alignment& y) {
        if (x.aread != y.aread) return x.aread < y.aread;
        if (x.bread != y.bread) return x.bread < y.bread;
        return x.abpos < y.abpos;
    });
    tm.mark("ingest");

    if (gpu.join() != HINGE_OK) { fprintf(stderr, "paf2las: no usable GPU (%s)\n", gpu.ctx ? hinge_last_error(gpu.ctx) : "hinge_ctx_create failed"); quit(2); }
    hinge_ctx* ctx = gpu.ctx;
    auto die = [&](const char* what) { fprintf(stderr, "paf2las: %s: %s\n", what, hinge_last_error(ctx)); quit(2); };
    if (hinge_consensus_set_db(ctx, 0, n_contigs, db1.rlen.data(), db1.boff.data(), bps1.p, (int64_t)bps1.n) != HINGE_OK) die("draft DB");
    if (hinge_consensus_set_db(ctx, 1, n_reads, db2.rlen.data(), db2.boff.data(), bps2.p, (int64_t)bps2.n) != HINGE_OK) die("read DB");
    tm.mark("H2D bases");
    const int64_t n = (int64_t)pl.size();
    int64_t cap = 0;
    int room = 0;                                   // refine: no widened box reaches further than this beyond the given one
    if (refine) {
        const char* g = getenv("HINGE_TRACE_EXTEND");
        room = ends.extend >= 0 ? ends.extend : (g && *g) ? std::max(atoi(g), 0) : 50;
    }
    for (const hinge_cns_alignment& r : pl) cap += 2 * (int64_t)((r.aepos + room - 1) / tspace - std::max(r.abpos - room, 0) / tspace + 1);
    std::vector<hinge_cns_alignment> out((size_t)std::max<int64_t>(n, 1));
    std::vector<uint16_t> trace((size_t)std::max<int64_t>(cap, 1));
    std::vector<int32_t> diffs((size_t)std::max<int64_t>(n, 1)), status((size_t)std::max<int64_t>(2 * n, 2));
    int64_t n_trace = 0;
    if (refine) {
        std::vector<int32_t> score((size_t)std::max<int64_t>(n, 1));
        if ((local ? hinge_trace_local : hinge_trace_refine)(ctx, n, pl.data(), tspace, band, band_max, &ends, out.data(), trace.data(), cap, &n_trace, diffs.data(), status.data(),
                                                             score.data()) != HINGE_OK)
            die("trace");
    } else if (hinge_trace_run(ctx, n, pl.data(), tspace, band, band_max, out.data(), trace.data(), cap, &n_trace, diffs.data(), status.data()) != HINGE_OK) die("trace");
    tm.mark("align + trace");

    // ---- the .las: records sorted by (aread, bread, abpos) - the placements' order ------------------------------------------------
    FILE* fo = fopen(pos[3].c_str(), "wb");
    if (!fo) { fprintf(stderr, "paf2las: cannot write %s\n", pos[3].c_str()); quit(1); }
    int64_t written = 0;
    for (int64_t x = 0; x < n; x++) written += status[(size_t)(2 * x)] == 0;
    const int32_t ts32 = tspace;
    fwrite(&written, 8, 1, fo);
    fwrite(&ts32, 4, 1, fo);
    const int tbytes = tspace <= 125 ? 1 : 2;
    std::vector<uint8_t> tb;
    std::vector<int64_t> order((size_t)n);
    for (int64_t x = 0; x < n; x++) order[(size_t)x] = x;
    if (refine)                          // refined abpos: two placements of one read on one contig may have changed places
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
            const hinge_cns_alignment &p = out[(size_t)x], &q = out[(size_t)y];
            if (p.aread != q.aread) return p.aread < q.aread;
            if (p.bread != q.bread) return p.bread < q.bread;
            return p.abpos < q.abpos;
        });
    for (int64_t x : order) {
        if (status[(size_t)(2 * x)] != 0) continue;
        const hinge_cns_alignment& r = out[(size_t)x];
        uint8_t rec[40];
        memset(rec, 0, sizeof(rec));
        const int32_t v[9] = {r.tlen, diffs[(size_t)x], r.abpos, r.bbpos, r.aepos, r.bepos, r.comp ? 1 : 0, r.aread, r.bread};
        memcpy(rec, v, 36);
        fwrite(rec, 40, 1, fo);
        tb.resize((size_t)r.tlen * (size_t)tbytes);
        for (int k = 0; k < r.tlen; k++) {
            const uint16_t val = trace[(size_t)r.trace_off + (size_t)k];
            if (tbytes == 1) tb[(size_t)k] = (uint8_t)val;
            else { tb[(size_t)2 * k] = (uint8_t)(val & 0xff); tb[(size_t)2 * k + 1] = (uint8_t)(val >> 8); }
        }
        if (!tb.empty()) fwrite(tb.data(), 1, tb.size(), fo);
    }
    if (fclose(fo) != 0) { fprintf(stderr, "paf2las: cannot write %s\n", pos[3].c_str()); quit(1); }

    // ---- the summary line ------------------------------------------------------------------------------------------------------------
    std::map<int, int64_t> widened;      // final W -> records made there (beyond the first W)
    int64_t dropped[6] = {0, 0, 0, 0, 0, 0};
    int first_w = 0;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hinge_trace_last_stats(ctx, stats);
    for (int64_t x = 0; x < n; x++) {
        const int w = status[(size_t)(2 * x + 1)];
        if (first_w == 0 || (w > 0 && w < first_w)) first_w = w;
    }
    for (int64_t x = 0; x < n; x++) {
        const int st = status[(size_t)(2 * x)], w = status[(size_t)(2 * x + 1)];
        if (st == 0) { if (w != first_w) widened[w]++; }
        else if (st >= 1 && st <= 5) dropped[st]++;
    }
    std::string rtxt;                    // refine: "; clipped out N, end points moved by B bases on average" (all four of a record)
    if (refine) {
        long long moved = 0;
        for (int64_t x = 0; x < n; x++)
            if (status[(size_t)(2 * x)] == 0) {
                const hinge_cns_alignment &o = out[(size_t)x], &g = pl[(size_t)x];
                moved += std::abs(o.abpos - g.abpos) + std::abs(o.aepos - g.aepos) + std::abs(o.bbpos - g.bbpos) + std::abs(o.bepos - g.bepos);
            }
        char buf[128];
        snprintf(buf, sizeof(buf), "; clipped out %lld, end points moved by %.1f bases on average", (long long)dropped[5], written ? (double)moved / (4.0 * (double)written) : 0.0);
        rtxt = buf;
    }
    std::string wtxt;
    for (auto& kv : widened) wtxt += (wtxt.empty() ? "" : ", ") + std::string("W=") + std::to_string(kv.first) + ": " + std::to_string(kv.second);
    printf("paf2las: %lld placements read, %lld written, widened %s, dropped %lld (touched %lld, no path %lld, wide %lld, steps %lld); %lld batch(es)%s\n", (long long)n,
           (long long)written, wtxt.empty() ? "0" : ("(" + wtxt + ")").c_str(), (long long)(n - written), (long long)dropped[1], (long long)dropped[2], (long long)dropped[3],
           (long long)dropped[4], (long long)stats[0], rtxt.c_str());
    for (int64_t x = 0; x < n; x++)
        if (status[(size_t)(2 * x)] != 0) {
            static const char* const why[6] = {"", "touched the band's edge", "no path", "wide segment", "steps", "clipped out (no stretch reaches the minimum score)"};
            const hinge_cns_alignment& r = pl[(size_t)x];
            const int st = status[(size_t)(2 * x)];
            fprintf(stderr, "paf2las: dropped contig %d [%d, %d) read %d%s [%d, %d): %s at W = %d\n", r.aread, r.abpos, r.aepos, r.bread, r.comp ? " (-)" : "", r.bbpos, r.bepos,
                    (st >= 1 && st <= 5) ? why[st] : "?", status[(size_t)(2 * x + 1)]);
        }
    tm.mark("write");
    return finish(ctx, tm, 0);
}
