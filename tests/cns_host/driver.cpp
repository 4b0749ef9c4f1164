// tests/test_consensus_host.py: the kernels of hinge_amd/csrc/consensus_kernels.h (a copy made by the test, beside the stand-in
// <hip/hip_runtime.h> of this directory) on the CPU under AddressSanitizer and UBSan, in the order and with the buffer sizes of
// hinge_amd/csrc/consensus_capi.inc.  Buffers the kernels only read are heap blocks of exactly the library's size (the sanitizer's
// red zones are the bound: the .bps copies are bps_bytes + CNS_BPS_SPARE); buffers they write carry guard words that are checked
// at the end.  Kernels without a barrier run one thread after the other; k_cns_scan (1024 threads) and k_cns_vote_tiles (256) run
// as host threads with a barrier.  k_cns_call / k_cns_emit (cross-lane shuffles) are not run.
//
//   driver windows            cns_window, CnsPair::winA / winB, cns_stage + cns_lds_window / cns_lds_base against cns_base / A / B
//   driver run IN OUT         one data set (the test's binary layout, below) -> segment table, indel lists, columns, both votes
#include "consensus_kernels.h"
#include <pthread.h>
#include <sanitizer/asan_interface.h>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>
thread_local Idx3 threadIdx, blockIdx;
Idx3 gridDim, blockDim;
bool hip_host_parallel = false;
namespace hinge { unsigned cnt_lds[5 * (CNS_TILE_MAX + 1)]; }
static pthread_barrier_t bar;
void __syncthreads() { pthread_barrier_wait(&bar); }
using namespace hinge;

template <typename F> static void launch(unsigned grid, unsigned block, bool threads, F f) {
    gridDim = Idx3{grid, 1, 1}; blockDim = Idx3{block, 1, 1};
    for (unsigned b = 0; b < grid; b++) {
        if (!threads) {
            for (unsigned t = 0; t < block; t++) { threadIdx = Idx3{t, 0, 0}; blockIdx = Idx3{b, 0, 0}; f(); }
            continue;
        }
        hip_host_parallel = true;
        pthread_barrier_init(&bar, nullptr, block);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block; t++) th.emplace_back([&, t] { threadIdx = Idx3{t, 0, 0}; blockIdx = Idx3{b, 0, 0}; f(); });
        for (auto& t : th) t.join();
        pthread_barrier_destroy(&bar);
        hip_host_parallel = false;
    }
}

template <typename T> struct Exact {      // read-only input: a heap block of exactly n elements (at least one, as the library's ensure())
    T* p; size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(sizeof(T) * std::max<size_t>(n_, 1))), n(n_) {}
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};
static bool guards_ok = true;
template <typename T> struct Guarded {    // written by the kernels: 4 guard elements on either side
    std::vector<T> v; size_t n; const char* name;
    Guarded(size_t n_, const char* name_, int fill = 0) : v(std::max<size_t>(n_, 1) + 8), n(std::max<size_t>(n_, 1)), name(name_) {
        memset(v.data(), 0xcd, sizeof(T) * v.size());
        memset(v.data() + 4, fill, sizeof(T) * n);
    }
    T* p() { return v.data() + 4; }
    void check() {
        const unsigned char* b = (const unsigned char*)v.data();
        for (size_t k = 0; k < 4 * sizeof(T); k++)
            if (b[k] != 0xcd || b[(4 + n) * sizeof(T) + k] != 0xcd) { fprintf(stderr, "GUARD %s\n", name); guards_ok = false; return; }
    }
};

static int windows() {
    const int lens[] = {1, 15, 16, 17, 31, 33, 64};
    long checked = 0, bad = 0;
    unsigned rnd = 12345u;
    Exact<unsigned> LW((size_t)2 * CNS_LDS_WORDS * 256);
    for (int len : lens)
        for (int order = 0; order < 2; order++) {     // the sequence as the last one of its DB, and with another one behind it
            const int rl[2] = {order ? len : 7, order ? 7 : len};
            const long long bo[2] = {0, (rl[0] + 3) / 4};
            const size_t bytes = (size_t)bo[1] + (size_t)(rl[1] + 3) / 4;
            Exact<unsigned char> bps(bytes + CNS_BPS_SPARE);
            memset(bps.p, 0, bytes);
            memset(bps.p + bytes, 0xa5, CNS_BPS_SPARE);       // (the library never writes the spare bytes)
            for (int s = 0; s < 2; s++)
                for (int p = 0; p < rl[s]; p++) { rnd = rnd * 1664525u + 1013904223u; bps.p[bo[s] + (p >> 2)] |= (unsigned char)(((rnd >> 24) & 3u) << (6 - 2 * (p & 3))); }
            for (int s = 0; s < 2; s++)
                for (int comp = 0; comp < 2; comp++) {
                    CnsPair S;
                    S.abps = bps.p; S.aoff = bo[s]; S.bbps = bps.p; S.boff = bo[s]; S.comp = comp; S.blen = rl[s];
                    const int L = rl[s];
                    auto cmp = [&](unsigned w, int x, int lim, bool isA) {
                        for (int t = 0; t < 16 && x + t < lim; t++) { checked++; if ((int)((w >> (30 - 2 * t)) & 3u) != (isA ? S.A(x + t) : S.B(x + t))) bad++; }
                    };
                    for (int x = 0; x < L; x++) {
                        if (comp == 0) cmp(cns_window(bps.p, bo[s], x), x, L, true);
                        cmp(S.winA(x), x, L, true);
                        cmp(S.winB(x), x, L, false);     // (comp: x within 15 bases of either end among them)
                    }
                    // every segment [a0, a0 + m) x [b0, b0 + n) that ends at the sequence's end, and a few that end inside it
                    unsigned* LA = LW.p + 0, * LB = LW.p + (size_t)CNS_LDS_WORDS * 256 + 255;    // (the first and the last lane's column)
                    for (int a0 = 0; a0 < L; a0++)
                        for (int m : {L - a0, (L - a0 + 1) / 2, 1}) {
                            memset(LW.p, 0x5a, sizeof(unsigned) * 2 * CNS_LDS_WORDS * 256);
                            cns_stage(S, a0, m, a0, m, LA, LB);
                            for (int x = 0; x < m; x++) {
                                const unsigned wa = cns_lds_window(LA, x), wb = cns_lds_window(LB, x);
                                for (int t = 0; t < 16 && x + t < m; t++) {
                                    checked += 2;
                                    if ((int)((wa >> (30 - 2 * t)) & 3u) != S.A(a0 + x + t)) bad++;
                                    if ((int)((wb >> (30 - 2 * t)) & 3u) != S.B(a0 + x + t)) bad++;
                                }
                                checked += 2;
                                if (cns_lds_base(LA, x) != S.A(a0 + x)) bad++;
                                if (cns_lds_base(LB, x) != S.B(a0 + x)) bad++;
                            }
                        }
                }
        }
    printf("windows checked %ld mismatches %ld\n", checked, bad);
    return bad ? 5 : 0;
}

// IN: int64 hd[8] = {tspace, nA, nB, bytesA, bytesB, n_aln, n_trace, 0}; int32 rlenA[nA]; int64 boffA[nA]; bytesA bytes; the same
// for B; int32 aln[n_aln][10] = {a, b, comp, ab, ae, bb, be, tlen, trace_off, 0}; uint16 trace[n_trace].
// OUT (int32 stream): hd[8] = {n_seg, n_tiles (0: no tile vote), tile, n_pos, status, tiled, 0, 0}; seg[n_seg][7] (CnsSeg);
// n_indel[n_seg]; n_ins[n_seg]; col_base[n_seg]; cols[n_aln][3]; indels[out_total] preceded by out_total; global counts[9 n_pos];
// tile counts[9 n_pos]; halo[4 n_tiles]; tile_base[nA + 1].
static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

static int run(const char* in, const char* outp) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    long long hd[8];
    rd(f, hd, sizeof(hd));
    const int tspace = (int)hd[0];
    const int nseq[2] = {(int)hd[1], (int)hd[2]};
    const size_t bytes[2] = {(size_t)hd[3], (size_t)hd[4]};
    const int n_aln = (int)hd[5];
    const size_t n_trace = (size_t)hd[6];
    // hinge_consensus_set_db
    Exact<int> rlen0(nseq[0]), rlen1(nseq[1]);
    Exact<long long> boff0(nseq[0]), boff1(nseq[1]);
    Exact<unsigned char> bps0(bytes[0] + CNS_BPS_SPARE), bps1(bytes[1] + CNS_BPS_SPARE);
    rd(f, rlen0.p, sizeof(int) * nseq[0]); rd(f, boff0.p, sizeof(long long) * nseq[0]); rd(f, bps0.p, bytes[0]);
    rd(f, rlen1.p, sizeof(int) * nseq[1]); rd(f, boff1.p, sizeof(long long) * nseq[1]); rd(f, bps1.p, bytes[1]);
    memset(bps0.p + bytes[0], 0xa5, CNS_BPS_SPARE);
    memset(bps1.p + bytes[1], 0xa5, CNS_BPS_SPARE);
    std::vector<int> ain((size_t)n_aln * 10);
    rd(f, ain.data(), sizeof(int) * ain.size());
    Exact<unsigned short> trace(n_trace);
    rd(f, trace.p, sizeof(unsigned short) * n_trace);
    fclose(f);
    CnsSeqs SA{bps0.p, boff0.p, rlen0.p}, SB{bps1.p, boff1.p, rlen1.p};
    // cns_realign_stage
    Guarded<CnsAln> alns(n_aln, "alns");
    long long n_seg = 0;
    for (int x = 0; x < n_aln; x++) {
        const int* r = &ain[(size_t)x * 10];
        CnsAln& a = alns.p()[x];
        a.a = r[0]; a.b = r[1]; a.comp = r[2]; a.ab = r[3]; a.ae = r[4]; a.bb = r[5]; a.be = r[6]; a.blen = rlen1.p[r[1]];
        a.seg0 = (int)n_seg; a.nseg = std::max(r[7] / 2, 1); a.dcap = 0; a.tlen = r[7]; a.toff = r[8];
        n_seg += a.nseg;
    }
    Guarded<CnsSeg> segs(n_seg, "segs");
    Guarded<unsigned> aln_slots(n_aln, "aln_slots");
    Guarded<int> n_indel(n_seg, "n_indel"), n_ins(n_seg, "n_ins"), scal(16, "scal");
    const unsigned galn = (unsigned)((n_aln + CNS_BLOCK - 1) / CNS_BLOCK);
    launch(galn, CNS_BLOCK, false, [&] { k_cns_segments(alns.p(), n_aln, trace.p, tspace, rlen0.p, segs.p(), aln_slots.p(), scal.p() + 8, scal.p()); });
    launch(1, 1024, true, [&] { k_cns_scan(aln_slots.p(), n_aln, (unsigned long long*)(scal.p() + 10)); });
    launch(galn, CNS_BLOCK, false, [&] { k_cns_seg_offsets(alns.p(), n_aln, aln_slots.p(), segs.p()); });
    if (scal.p()[0] & CNS_ST_TRACE) { fprintf(stderr, "CNS_ST_TRACE\n"); return 3; }
    const int width_max = std::max(scal.p()[8], 4), dcap_max = scal.p()[9];
    unsigned long long out_total;
    memcpy(&out_total, scal.p() + 10, sizeof(out_total));
    Guarded<int> indels(out_total, "indels");
    const long long cells_max = cns_cells(dcap_max, width_max);
    Guarded<int> scratch((size_t)(CNS_BLOCK * cells_max), "scratch", 0x7e);       // one workgroup's wave storage
    launch(1, CNS_BLOCK, false, [&] { k_cns_realign(SA, SB, alns.p(), segs.p(), (int)n_seg, scratch.p(), width_max, dcap_max + 3, indels.p(), n_indel.p(), n_ins.p(), scal.p()); });
    // hinge_consensus_run
    const int n_contigs = nseq[0];
    Exact<long long> cbase((size_t)n_contigs + 1);
    cbase.p[0] = 0;
    for (int c = 0; c < n_contigs; c++) cbase.p[c + 1] = cbase.p[c] + rlen0.p[c];
    const long long n_pos = cbase.p[n_contigs];
    const int tile = cns_tile_len(tspace);
    const bool tiled = tile <= CNS_TILE_MAX;
    Exact<int> tile_base((size_t)n_contigs + 1);
    std::vector<int> cot;
    tile_base.p[0] = 0;
    for (int c = 0; c < n_contigs; c++) {
        tile_base.p[c + 1] = tile_base.p[c] + (rlen0.p[c] + tile - 1) / tile;
        for (int t = tile_base.p[c]; t < tile_base.p[c + 1]; t++) cot.push_back(c);
    }
    const int n_tiles = tile_base.p[n_contigs];
    const size_t plane = (size_t)std::max<long long>(n_pos, 1);
    Guarded<int> col_base(n_seg, "col_base");
    Guarded<CnsCols> cols(n_aln, "cols");
    Guarded<int> counts_g(9 * plane, "counts (global vote)"), counts_t(9 * plane, "counts (tile vote)", 0x7f);   // (the tile vote stores every position itself)
    launch(galn, CNS_BLOCK, false, [&] { k_cns_columns(alns.p(), n_aln, segs.p(), indels.p(), n_indel.p(), n_ins.p(), col_base.p(), cols.p(), 100); });
    launch((unsigned)((n_seg + CNS_BLOCK - 1) / CNS_BLOCK), CNS_BLOCK, false,
           [&] { k_cns_vote(SB, alns.p(), segs.p(), (int)n_seg, indels.p(), n_indel.p(), col_base.p(), cols.p(), cbase.p, counts_g.p(), (long long)plane); });
    Exact<int> contig_of_tile(n_tiles);
    memcpy(contig_of_tile.p, cot.data(), sizeof(int) * cot.size());
    Guarded<unsigned> tile_ptr((size_t)n_tiles + 1, "tile_ptr"), tile_cursor((size_t)n_tiles + 1, "tile_cursor");
    Guarded<int> seg_order(n_seg, "seg_order"), halo(4 * (size_t)n_tiles, "halo");
    if (tiled) {
        unsigned long long* total = (unsigned long long*)(scal.p() + 2);
        launch(galn, CNS_BLOCK, false, [&] { k_cns_tile_count(alns.p(), n_aln, segs.p(), tile_base.p, tile, tile_ptr.p()); });
        launch(1, 1024, true, [&] { k_cns_scan(tile_ptr.p(), n_tiles + 1, total + 1); });
        memcpy(tile_cursor.p(), tile_ptr.p(), sizeof(unsigned) * ((size_t)n_tiles + 1));
        launch(galn, CNS_BLOCK, false, [&] { k_cns_tile_fill(alns.p(), n_aln, segs.p(), tile_base.p, tile, tile_cursor.p(), seg_order.p()); });
        // the launch's dynamic LDS: 5 words per position of the tile and of the halo slot - what lies behind is poisoned
        const size_t lds = sizeof(unsigned) * 5 * ((size_t)tile + 1);
        memset(cnt_lds, 0xee, sizeof(cnt_lds));
        if (lds < sizeof(cnt_lds)) ASAN_POISON_MEMORY_REGION((char*)cnt_lds + lds, sizeof(cnt_lds) - lds);
        launch((unsigned)n_tiles, CNS_BLOCK, true, [&] {
            k_cns_vote_tiles(SB, alns.p(), segs.p(), indels.p(), n_indel.p(), col_base.p(), cols.p(), cbase.p, tile_base.p, contig_of_tile.p, tile_ptr.p(), seg_order.p(), tile,
                             counts_t.p(), (long long)plane, halo.p(), scal.p());
        });
        ASAN_UNPOISON_MEMORY_REGION(cnt_lds, sizeof(cnt_lds));
    }
    alns.check(); segs.check(); aln_slots.check(); n_indel.check(); n_ins.check(); scal.check(); indels.check(); scratch.check(); col_base.check(); cols.check();
    counts_g.check(); counts_t.check(); tile_ptr.check(); tile_cursor.check(); seg_order.check(); halo.check();
    if (!guards_ok) return 4;
    FILE* o = fopen(outp, "wb");
    if (!o) return 2;
    const int oh[8] = {(int)n_seg, tiled ? n_tiles : 0, tile, (int)n_pos, scal.p()[0], tiled ? 1 : 0, 0, 0};
    fwrite(oh, 4, 8, o);
    static_assert(sizeof(CnsSeg) == 28 && sizeof(CnsCols) == 12, "the output layout");
    fwrite(segs.p(), sizeof(CnsSeg), (size_t)n_seg, o);
    fwrite(n_indel.p(), 4, (size_t)n_seg, o);
    fwrite(n_ins.p(), 4, (size_t)n_seg, o);
    fwrite(col_base.p(), 4, (size_t)n_seg, o);
    fwrite(cols.p(), sizeof(CnsCols), (size_t)n_aln, o);
    const int ot = (int)out_total;
    fwrite(&ot, 4, 1, o);
    fwrite(indels.p(), 4, (size_t)out_total, o);
    fwrite(counts_g.p(), 4, 9 * (size_t)n_pos, o);
    fwrite(counts_t.p(), 4, 9 * (size_t)n_pos, o);
    if (tiled) fwrite(halo.p(), 4, 4 * (size_t)n_tiles, o);
    fwrite(tile_base.p, 4, (size_t)n_contigs + 1, o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "windows")) return windows();
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: driver windows | driver run IN OUT\n");
    return 2;
}
