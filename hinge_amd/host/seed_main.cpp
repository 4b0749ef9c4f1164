// seed  ==  `hinge seed DRAFT_DB READ_DB OUT.paf [--k K] [--step S] [--window W] [--max-occ C] [--min-hits H] [--max-placements N] [--list L]`
// Not a program of the reference: it stands where demo/ecoli_demo/run.sh:30-37 runs HPC.daligner on (draft, reads) to find where
// every read lies on the draft, and where this build's README used to say `minimap2`.  The k-mer votes are computed behind the C ABI
// (hinge_seed_run, include/hinge_hip.h) on the GPU; this file reads the DBs and writes the placements as PAF for
// `hinge paf2las --ends local`: query = read, target = contig, names whose middle field is the 1-based id (what paf2las resolves
// without --draft-names / --read-names), `-` lines with query coordinates on the stored read, column 10 = the window's hit count,
// column 11 = the projected length, column 12 = 255, tags sd:i: (the diagonal gpos - p) and sc:i: (the count).
// --self-test-paf FILE (a self-test of the PAF writer, not in the usage text: no GPU, NO seeding): the PAF text of placements given as
// lines "read comp contig abpos aepos bbpos bepos count diag"; it says so on stderr.
#include "host_common.h"

using namespace hh;

static void usage() {
    fprintf(stderr, "usage: seed <draft db> <read db> <out.paf> [--k K] [--step S] [--window W] [--max-occ C] [--min-hits H] [--max-placements N] [--list L]\n");
}

static void paf_line(FILE* fo, const hinge_cns_alignment& r, int count, int diag, int qlen, int tlen) {
    const int qs = r.comp ? qlen - r.bepos : r.bbpos, qe = r.comp ? qlen - r.bbpos : r.bepos;   // a `-` line: on the stored read
    fprintf(fo, "read/%d/0_%d\t%d\t%d\t%d\t%c\tcontig/%d/0_%d\t%d\t%d\t%d\t%d\t%d\t255\tsd:i:%d\tsc:i:%d\n", r.bread + 1, qlen, qlen, qs, qe, r.comp ? '-' : '+', r.aread + 1, tlen, tlen,
            r.abpos, r.aepos, count, r.aepos - r.abpos, diag, count);
}

int main(int argc, char* argv[]) {
    std::vector<std::string> pos;
    hinge_seed_params prm = {0, 0, 0, 0, 0, 0, 0};      // the library's defaults (15, 2, 256, 16, 2048, 1, 3)
    std::string given;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](const char* name) -> int {
            if (i + 1 >= argc) { fprintf(stderr, "seed: %s needs a value\n", name); usage(); exit(1); }
            const int v = atoi(argv[++i]);
            if (v < 1) { fprintf(stderr, "seed: %s needs a positive number\n", name); usage(); exit(1); }
            return v;
        };
        if (a == "--k") prm.k = val("--k");
        else if (a == "--step") prm.step = val("--step");
        else if (a == "--window") prm.window = val("--window");
        else if (a == "--max-occ") prm.max_occ = val("--max-occ");
        else if (a == "--min-hits") prm.min_hits = val("--min-hits");
        else if (a == "--max-placements") prm.max_placements = val("--max-placements");
        else if (a == "--list") prm.list = val("--list");
        else if (a == "--self-test-paf") {
            if (i + 1 >= argc) { fprintf(stderr, "seed: --self-test-paf needs a value\n"); usage(); return 1; }
            given = argv[++i];
        }
        else if (a.size() > 2 && a[0] == '-' && a[1] == '-') { fprintf(stderr, "seed: unknown option %s\n", a.c_str()); usage(); return 1; }
        else pos.push_back(a);
    }
    if (pos.size() != 3) { usage(); return 1; }
    ReadDB db1, db2;
    if (db1.open(pos[0]) != 0 || db2.open(pos[1]) != 0) { fprintf(stderr, "seed: Could not open database\n"); return 1; }
    const int n_contigs = (int)db1.rlen.size(), n_reads = (int)db2.rlen.size();
    if (!given.empty()) {
        fprintf(stderr, "seed: --self-test-paf: writing the given placements as PAF, nothing is seeded\n");
        std::string t;
        if (!slurp_gz(given, t)) { fprintf(stderr, "seed: cannot read %s\n", given.c_str()); return 1; }
        FILE* fo = fopen(pos[2].c_str(), "wb");
        if (!fo) { fprintf(stderr, "seed: cannot write %s\n", pos[2].c_str()); return 1; }
        const char* p = t.c_str();
        int b, comp, a, ab, ae, bb, be, cnt, dg, used = 0;
        while (sscanf(p, "%d %d %d %d %d %d %d %d %d%n", &b, &comp, &a, &ab, &ae, &bb, &be, &cnt, &dg, &used) == 9) {
            p += used;
            if (b < 0 || b >= n_reads || a < 0 || a >= n_contigs) { fprintf(stderr, "seed: %s: an id outside its DB\n", given.c_str()); return 1; }
            hinge_cns_alignment r;
            r.aread = a; r.bread = b; r.comp = comp ? 1 : 0; r.abpos = ab; r.aepos = ae; r.bbpos = bb; r.bepos = be; r.tlen = 0; r.trace_off = 0;
            paf_line(fo, r, cnt, dg, db2.rlen[(size_t)b], db1.rlen[(size_t)a]);
        }
        if (fclose(fo) != 0) { fprintf(stderr, "seed: cannot write %s\n", pos[2].c_str()); return 1; }
        return 0;
    }
    PhaseTimer tm("seed");
    CtxInit gpu;
    gpu.start();
    Mapped bps1, bps2;
    const bool has1 = bps1.open(db1.dir + "/." + db1.root + ".bps"), has2 = bps2.open(db2.dir + "/." + db2.root + ".bps");
    if ((!has1 && !db1.rlen.empty()) || (!has2 && !db2.rlen.empty())) { fprintf(stderr, "seed: cannot read the .bps file of a database\n"); quit(1); }
    tm.mark("ingest");
    if (gpu.join() != HINGE_OK) { fprintf(stderr, "seed: no usable GPU (%s)\n", gpu.ctx ? hinge_last_error(gpu.ctx) : "hinge_ctx_create failed"); quit(2); }
    hinge_ctx* ctx = gpu.ctx;
    auto die = [&](const char* what) { fprintf(stderr, "seed: %s: %s\n", what, hinge_last_error(ctx)); quit(2); };
    if (hinge_consensus_set_db(ctx, 0, n_contigs, db1.rlen.data(), db1.boff.data(), bps1.p, (int64_t)bps1.n) != HINGE_OK) die("draft DB");
    if (hinge_consensus_set_db(ctx, 1, n_reads, db2.rlen.data(), db2.boff.data(), bps2.p, (int64_t)bps2.n) != HINGE_OK) die("read DB");
    tm.mark("H2D bases");
    const int64_t cap = (int64_t)n_reads * HINGE_SEED_MAX_PLACEMENTS_LIMIT;      // room for any --max-placements: the default is the library's alone
    std::vector<hinge_cns_alignment> out((size_t)std::max<int64_t>(cap, 1));
    std::vector<int32_t> count((size_t)std::max<int64_t>(cap, 1)), diag((size_t)std::max<int64_t>(cap, 1)), n_placed((size_t)std::max(n_reads, 1)), status((size_t)std::max(2 * n_reads, 2));
    int64_t m = 0;
    if (hinge_seed_run(ctx, &prm, n_reads, nullptr, cap, out.data(), count.data(), diag.data(), n_placed.data(), status.data(), &m) != HINGE_OK) die("seed");
    tm.mark("index + votes");
    FILE* fo = fopen(pos[2].c_str(), "wb");
    if (!fo) { fprintf(stderr, "seed: cannot write %s\n", pos[2].c_str()); quit(1); }
    for (int64_t x = 0; x < m; x++) paf_line(fo, out[(size_t)x], count[(size_t)x], diag[(size_t)x], db2.rlen[(size_t)out[(size_t)x].bread], db1.rlen[(size_t)out[(size_t)x].aread]);
    if (fclose(fo) != 0) { fprintf(stderr, "seed: cannot write %s\n", pos[2].c_str()); quit(1); }
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hinge_seed_last_stats(ctx, st);
    int64_t over_reads = 0;
    for (int r = 0; r < n_reads; r++) over_reads += status[(size_t)(2 * r)] == 2 || status[(size_t)(2 * r + 1)] == 2;
    printf("seed: %d reads, %lld placements written; index %lld entries (%lld codes dropped by max-occ); %lld job(s) in %lld batch(es)\n", n_reads, (long long)m, (long long)st[2],
           (long long)st[3], (long long)st[0], (long long)st[1]);
    fprintf(stderr, "seed: %lld read(s) without a placement, %lld read(s) with dropped hits (OVERFLOW)\n", (long long)st[5], (long long)over_reads);
    tm.mark("write");
    return finish(ctx, tm, 0);
}
