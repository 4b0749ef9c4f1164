// tests/test_seed_host.py: k_seed_vote of hinge_amd/csrc/seed_kernels.h (a copy made by the test, beside the host stand-ins of
// tests/trace_host) and the index of seed_index.h run on the CPU - a wavefront = 64 threads in lock step - under AddressSanitizer and
// UBSan, with guard words around the output and behind the LDS the job may use; the packed bases and the index are heap blocks of
// their exact size.  The ballot and the cross-lane exchange are arrays of 64 slots between two barriers.
// stdin: "k step window max_occ list n_max min_hits", "n_contigs" and the contigs, "n_jobs" and per job "comp READ" (bases as digits
// 0-3, the read as stored).  stdout: "index ENTRIES DROPPED", then per job "status picks hits" and per pick "cnt d p gpos" followed by
// "1 contig abpos aepos bbpos bepos" or "0".
#include "seed_kernels.h"
#include "seed_index.h"
#include <pthread.h>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>
thread_local Idx3 threadIdx, blockIdx;
namespace hinge { unsigned char seed_lds[(1 << 16) + 256]; }
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
static std::vector<unsigned char> pack(const std::string& s) {
    std::vector<unsigned char> o((s.size() + 3) / 4, 0);
    for (size_t p = 0; p < s.size(); p++) o[p >> 2] |= (unsigned char)((s[p] - '0') << (6 - 2 * (p & 3)));
    return o;
}
int main() {
    int k, step, window, max_occ, list, n_max, min_hits, n_contigs, n_jobs;
    std::cin >> k >> step >> window >> max_occ >> list >> n_max >> min_hits >> n_contigs;
    std::vector<unsigned char> dbps;
    std::vector<int64_t> dboff;
    std::vector<int32_t> drlen;
    for (int c = 0; c < n_contigs; c++) {
        std::string s;
        std::cin >> s;
        const std::vector<unsigned char> pk = pack(s);
        dboff.push_back((int64_t)dbps.size());
        drlen.push_back((int32_t)s.size());
        dbps.insert(dbps.end(), pk.begin(), pk.end());
    }
    SeedIndex ix;
    seed_build_index(dbps.data(), dboff.data(), drlen.data(), n_contigs, k, max_occ, ix);
    printf("index %zu %lld\n", ix.codes.size(), (long long)ix.dropped_codes);
    SeedParams P;
    P.k = k; P.window = window; P.max_occ = max_occ; P.list = list; P.n_max = n_max; P.min_hits = min_hits;
    P.n_entries = (int)ix.codes.size();
    P.search_top = 0;
    for (int s = 1; s > 0 && s <= P.n_entries; s <<= 1) P.search_top = s;
    if (seed_lds_bytes(list) + 256 > sizeof(seed_lds)) return 3;
    seed_lane_xor_host = lane_xor;
    seed_ballot_host = ballot;
    std::cin >> n_jobs;
    const int G = 0x5a5a5a5a, W = seed_out_ints(n_max);
    for (int x = 0; x < n_jobs; x++) {
        int comp;
        std::string R;
        std::cin >> comp >> R;
        std::vector<unsigned char> pb = pack(R);
        long long boff = 0;
        int rl = (int)R.size();
        CnsSeqs SB{pb.data(), &boff, &rl};
        SeedJob J;
        J.b = 0; J.comp = comp; J.blen = rl; J.stride = rl >= k ? seed_stride(rl, k, step, list) : step;
        std::vector<int> out((size_t)W + 8, G);
        for (int v = 0; v < W; v++) out[4 + v] = -1;                  // the poison
        memset(seed_lds, 0xa5, sizeof(seed_lds));
        pthread_barrier_init(&bar, nullptr, 64);
        std::vector<std::thread> th;
        for (int l = 0; l < 64; l++)
            th.emplace_back([&, l] { threadIdx = Idx3{(unsigned)l, 0, 0}; blockIdx = Idx3{0, 0, 0}; k_seed_vote(SB, &J, 1, P, ix.codes.data(), ix.gpos.data(), out.data() + 4); });
        for (auto& t : th) t.join();
        pthread_barrier_destroy(&bar);
        for (int g = 0; g < 4; g++) if (out[g] != G || out[(size_t)W + 4 + g] != G) { printf("GUARD out\n"); return 4; }
        for (size_t g = seed_lds_bytes(list); g < sizeof(seed_lds); g++) if (seed_lds[g] != 0xa5) { printf("GUARD lds\n"); return 4; }
        const int* o = out.data() + 4;
        if (o[0] < 0 || o[0] > 2 || o[1] < 0 || o[1] > n_max || o[3] != 0) { printf("UNWRITTEN head\n"); return 5; }
        printf("%d %d %d", o[0], o[1], o[2]);
        for (int q = 0; q < n_max; q++) {
            const int* pk = o + SEED_HEAD + 4 * q;
            if (q >= o[1]) {
                for (int v = 0; v < 4; v++) if (pk[v] != -1) { printf(" STRAY\n"); return 5; }
                continue;
            }
            printf(" %d %u %d %d", pk[0], (unsigned)pk[1], pk[2], pk[3]);
            int c, ab, ae, bb, be;
            if (seed_project(ix.off.data(), n_contigs, k, pk[3], pk[2], rl, &c, &ab, &ae, &bb, &be)) printf(" 1 %d %d %d %d %d", c, ab, ae, bb, be);
            else printf(" 0");
        }
        printf("\n");
    }
    return 0;
}
