// tests/test_overlap_tile_multi_host.py: k_overlap_vote_tile_multi and k_overlap_tile_reduce_multi of
// hinge_amd/csrc/overlap_tile_multi_kernels.h (a copy made by the test, beside the host stand-ins of tests/trace_host) and the index
// of seed_index.h run on the CPU - a wavefront = 64 threads in lock step - under AddressSanitizer and UBSan, with guard words around
// every output row (each tile's, the reduced one, the reduce's largest-tile word) and behind the LDS the tile may use; the packed
// bases, the index and the tile rows the reduce reads are heap blocks of their exact size.  The ballot and the lane exchange are
// arrays of 64 slots between two barriers.
// stdin: "k step window max_occ list max_partners min_hits tile stretches", "n_reads" and the reads (bases as digits 0-3, as stored),
// "n_blocks" and per block "first end".  stdout per block: "index ENTRIES DROPPED", then per job (read, strand) "tiles top status
// candidates hits", the round counts and per candidate, round by round, "b cnt d p abpos aepos bbpos bepos diag".
#include "overlap_tile_multi_kernels.h"
#include "seed_index.h"
#include <pthread.h>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>
thread_local Idx3 threadIdx, blockIdx;
namespace hinge {
unsigned char ovl_lds[OVL_LDS_MAX + 256];
unsigned char seed_lds[16];          // (k_seed_vote of seed_kernels.h is compiled along; never run here)
}
static pthread_barrier_t bar;
void __syncthreads() { pthread_barrier_wait(&bar); }
static int lanes[64];
static int lane_xor(int v, int lane_mask) {
    lanes[threadIdx.x] = v;
    pthread_barrier_wait(&bar);
    const int got = lanes[threadIdx.x ^ (unsigned)lane_mask];
    pthread_barrier_wait(&bar);
    return got;
}
static unsigned long long ballot(bool p) {
    lanes[threadIdx.x] = p ? 1 : 0;
    pthread_barrier_wait(&bar);
    unsigned long long m = 0;
    for (int l = 0; l < 64; l++) if (lanes[l]) m |= 1ull << l;
    pthread_barrier_wait(&bar);
    return m;
}
using namespace hinge;
template <class F> static void wavefront(F f) {
    pthread_barrier_init(&bar, nullptr, 64);
    std::vector<std::thread> th;
    for (int l = 0; l < 64; l++)
        th.emplace_back([&, l] { threadIdx = Idx3{(unsigned)l, 0, 0}; blockIdx = Idx3{0, 0, 0}; f(); });
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&bar);
}
int main() {
    int k, step, window, max_occ, list, max_partners, min_hits, tile, S, n_reads, n_blocks;
    std::cin >> k >> step >> window >> max_occ >> list >> max_partners >> min_hits >> tile >> S >> n_reads;
    std::vector<unsigned char> bps;
    std::vector<int64_t> boff;
    std::vector<int32_t> rlen;
    for (int r = 0; r < n_reads; r++) {
        std::string s;
        std::cin >> s;
        boff.push_back((int64_t)bps.size());
        rlen.push_back((int32_t)s.size());
        std::vector<unsigned char> o((s.size() + 3) / 4, 0);
        for (size_t p = 0; p < s.size(); p++) o[p >> 2] |= (unsigned char)((s[p] - '0') << (6 - 2 * (p & 3)));
        bps.insert(bps.end(), o.begin(), o.end());
    }
    std::vector<long long> boff_ll(boff.begin(), boff.end());
    if (ovl_multi_lds_bytes(list) > (size_t)OVL_LDS_MAX || tile < OVT_TILE_MIN || tile > OVT_TILE_MAX || (tile & (tile - 1)) || (long long)tile > (long long)list * step || S < 1 ||
        S > OVL_STRETCHES_MAX)
        return 3;
    seed_lane_xor_host = lane_xor;
    seed_ballot_host = ballot;
    std::cin >> n_blocks;
    const int G = 0x5a5a5a5a, W = ovl_multi_out_ints(max_partners, S);
    OvlTileParams TP;
    TP.step = step; TP.tile = tile; TP.adv = tile / 2; TP.part_top = 1;
    while (2 * TP.part_top <= max_partners) TP.part_top *= 2;
    for (int blk = 0; blk < n_blocks; blk++) {
        int first, end;
        std::cin >> first >> end;
        SeedIndex ix;
        seed_build_index(bps.data(), boff.data() + first, rlen.data() + first, end - first, k, max_occ, ix);
        printf("index %zu %lld\n", ix.codes.size(), (long long)ix.dropped_codes);
        OvlParams P;
        P.k = k; P.window = window; P.max_occ = max_occ; P.list = list; P.max_partners = max_partners; P.min_hits = min_hits;
        P.n_entries = (int)ix.codes.size();
        P.search_top = 0;
        for (int s = 1; s > 0 && s <= P.n_entries; s <<= 1) P.search_top = s;
        P.first = first; P.n_reads = end - first;
        P.read_top = 0;
        for (int s = 1; s > 0 && s <= P.n_reads; s <<= 1) P.read_top = s;
        std::vector<unsigned> codes(ix.codes);          // heap blocks of the exact size (an empty index: one spare element, never read)
        std::vector<int> gpos(ix.gpos);
        if (codes.empty()) { codes.push_back(0); gpos.push_back(0); }
        for (int a = 0; a < n_reads; a++)
            for (int comp = 0; comp < 2; comp++) {
                CnsSeqs SB{bps.data(), boff_ll.data(), rlen.data()};
                const int alen = rlen[(size_t)a], nt = (int)ovl_tile_count(alen, k, tile);
                std::vector<int> rows((size_t)nt * (size_t)W);                // exactly what the reduce may read
                for (int t = 0; t < nt; t++) {
                    OvlTileJob J;
                    J.a = a; J.comp = comp; J.alen = alen; J.t = t;
                    std::vector<int> out((size_t)W + 8, G);
                    for (int v = 0; v < W; v++) out[4 + v] = -1;              // the poison
                    memset(ovl_lds, 0xa5, sizeof(ovl_lds));
                    wavefront([&] { k_overlap_vote_tile_multi(SB, &J, 1, P, TP, S, codes.data(), gpos.data(), ix.off.data(), out.data() + 4); });
                    for (int g = 0; g < 4; g++) if (out[g] != G || out[(size_t)W + 4 + g] != G) { printf("GUARD tile row\n"); return 4; }
                    for (size_t g = ovl_multi_lds_bytes(list); g < sizeof(ovl_lds); g++) if (ovl_lds[g] != 0xa5) { printf("GUARD lds\n"); return 4; }
                    memcpy(rows.data() + (size_t)t * (size_t)W, out.data() + 4, sizeof(int) * (size_t)W);
                }
                OvlRedJob R;
                R.row0 = 0; R.n_tiles = nt;
                std::vector<int> out((size_t)W + 8, G), top(9, G);
                for (int v = 0; v < W; v++) out[4 + v] = -1;
                top[4] = -1;
                wavefront([&] { k_overlap_tile_reduce_multi(rows.data(), &R, 1, max_partners, TP.part_top, S, window, out.data() + 4, top.data() + 4); });
                for (int g = 0; g < 4; g++) if (out[g] != G || out[(size_t)W + 4 + g] != G || top[g] != G || top[5 + g] != G) { printf("GUARD out\n"); return 4; }
                const int* o = out.data() + 4;
                if (o[0] < 0 || o[0] > 6 || o[1] < 0 || o[1] > S * max_partners || o[3] != 0 || top[4] < 0) { printf("UNWRITTEN head\n"); return 5; }
                printf("%d %d %d %d %d", nt, top[4], o[0], o[1], o[2]);
                int sum = 0;
                for (int r = 0; r < S; r++) {
                    if (o[OVL_HEAD + r] < 0 || o[OVL_HEAD + r] > max_partners) { printf(" UNWRITTEN round\n"); return 5; }
                    printf(" %d", o[OVL_HEAD + r]);
                    sum += o[OVL_HEAD + r];
                }
                if (sum != o[1]) { printf(" ROUND SUM\n"); return 5; }
                for (int r = 0; r < S; r++)
                    for (int q = 0; q < max_partners; q++) {
                        const int* pk = o + OVL_HEAD + S + 4 * (r * max_partners + q);
                        if (q >= o[OVL_HEAD + r]) {
                            for (int v = 0; v < 4; v++) if (pk[v] != -1) { printf(" STRAY\n"); return 5; }
                            continue;
                        }
                        int ab, ae, bb, be, dg;
                        if (pk[0] < 0 || pk[0] >= n_reads || !overlap_project(alen, rlen[(size_t)pk[0]], comp, pk[2], k, &ab, &ae, &bb, &be, &dg)) { printf(" NO PROJECTION\n"); return 5; }
                        printf(" %d %d %d %d %d %d %d %d %d", pk[0], pk[1], pk[2], pk[3], ab, ae, bb, be, dg);
                    }
                printf("\n");
            }
    }
    return 0;
}
