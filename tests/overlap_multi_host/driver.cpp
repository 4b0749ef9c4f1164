// tests/test_overlap_multi_host.py: k_overlap_vote_multi of hinge_amd/csrc/overlap_multi_kernels.h (a copy made by the test, beside
// overlap_kernels.h and the host stand-ins of tests/trace_host) run on the CPU - a wavefront = 64 threads in lock step - under
// AddressSanitizer and UBSan, with guard words around the output and behind the LDS the job may use (ovl_multi_lds_bytes); the
// packed bases and the index are heap blocks of their exact size.  The ballot is an array of 64 slots between two barriers.
// stdin: "mode k step window max_occ list max_partners min_hits stretches".
//   mode "reads": "n_reads" and the reads (bases as digits 0-3, as stored), "n_blocks" and per block "first end": the index of
//                 seed_index.h per block, every (read, strand) a job.
//   mode "hits":  the query read (digits), "n_targets" and their lengths, "n_hits" and per hit "b d p" (b a target, 0-based): a
//                 hand-made index of one block - the targets are reads 1 .. of a DB whose read 0 is the query - with, per hit, one
//                 entry of the code at p of the query at gpos = off[b] + d + p - alen; one job: the query forward.
// stdout per job: "status candidates hits n_round0 .. n_round(S-1)" and per candidate, round by round, "b cnt d p".
#include "overlap_multi_kernels.h"
#include "seed_index.h"
#include <pthread.h>
#include <algorithm>
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

static void pack(const std::string& s, std::vector<unsigned char>& bps, std::vector<int64_t>& boff, std::vector<int32_t>& rlen) {
    boff.push_back((int64_t)bps.size());
    rlen.push_back((int32_t)s.size());
    std::vector<unsigned char> o((s.size() + 3) / 4, 0);
    for (size_t p = 0; p < s.size(); p++) o[p >> 2] |= (unsigned char)((s[p] - '0') << (6 - 2 * (p & 3)));
    bps.insert(bps.end(), o.begin(), o.end());
}

// one job through the kernel; prints its line; 0 or the exit code
static int run_job(const CnsSeqs& SB, const OvlJob& J, const OvlParams& P, int S, const std::vector<unsigned>& codes, const std::vector<int>& gpos, const std::vector<long long>& off, int n_reads) {
    const int G = 0x5a5a5a5a, W = ovl_multi_out_ints(P.max_partners, S);
    std::vector<int> out((size_t)W + 8, G);
    for (int v = 0; v < W; v++) out[4 + v] = -1;                              // the poison
    memset(ovl_lds, 0xa5, sizeof(ovl_lds));
    pthread_barrier_init(&bar, nullptr, 64);
    std::vector<std::thread> th;
    for (int l = 0; l < 64; l++)
        th.emplace_back([&, l] { threadIdx = Idx3{(unsigned)l, 0, 0}; blockIdx = Idx3{0, 0, 0}; k_overlap_vote_multi(SB, &J, 1, P, S, codes.data(), gpos.data(), off.data(), out.data() + 4); });
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&bar);
    for (int g = 0; g < 4; g++) if (out[g] != G || out[(size_t)W + 4 + g] != G) { printf("GUARD out\n"); return 4; }
    for (size_t g = ovl_multi_lds_bytes(P.list); g < sizeof(ovl_lds); g++) if (ovl_lds[g] != 0xa5) { printf("GUARD lds\n"); return 4; }
    const int* o = out.data() + 4;
    if (o[0] < 0 || o[0] > 6 || o[1] < 0 || o[1] > S * P.max_partners || o[3] != 0) { printf("UNWRITTEN head\n"); return 5; }
    printf("%d %d %d", o[0], o[1], o[2]);
    int sum = 0;
    for (int r = 0; r < S; r++) {
        if (o[OVL_HEAD + r] < 0 || o[OVL_HEAD + r] > P.max_partners) { printf(" UNWRITTEN round\n"); return 5; }
        printf(" %d", o[OVL_HEAD + r]);
        sum += o[OVL_HEAD + r];
    }
    if (sum != o[1]) { printf(" SUM\n"); return 5; }
    for (int r = 0; r < S; r++)
        for (int q = 0; q < P.max_partners; q++) {
            const int* pk = o + OVL_HEAD + S + 4 * (r * P.max_partners + q);
            if (q >= o[OVL_HEAD + r]) {
                for (int v = 0; v < 4; v++) if (pk[v] != -1) { printf(" STRAY\n"); return 5; }
                continue;
            }
            if (pk[0] < 0 || pk[0] >= n_reads) { printf(" NO READ\n"); return 5; }
            printf(" %d %d %d %d", pk[0], pk[1], pk[2], pk[3]);
        }
    printf("\n");
    return 0;
}

int main() {
    std::string mode;
    int k, step, window, max_occ, list, max_partners, min_hits, S;
    std::cin >> mode >> k >> step >> window >> max_occ >> list >> max_partners >> min_hits >> S;
    if (ovl_multi_lds_bytes(list) > (size_t)OVL_LDS_MAX || S < 1 || S > OVL_STRETCHES_MAX) return 3;
    seed_lane_xor_host = lane_xor;
    seed_ballot_host = ballot;
    std::vector<unsigned char> bps;
    std::vector<int64_t> boff;
    std::vector<int32_t> rlen;
    OvlParams P;
    P.k = k; P.window = window; P.max_occ = max_occ; P.list = list; P.max_partners = max_partners; P.min_hits = min_hits;
    auto tops = [&](int n_entries, int first, int n_reads) {
        P.n_entries = n_entries;
        P.search_top = 0;
        for (int s = 1; s > 0 && s <= P.n_entries; s <<= 1) P.search_top = s;
        P.first = first; P.n_reads = n_reads;
        P.read_top = 0;
        for (int s = 1; s > 0 && s <= P.n_reads; s <<= 1) P.read_top = s;
    };
    if (mode == "hits") {
        std::string q;
        int n_targets, n_hits;
        std::cin >> q >> n_targets;
        pack(q, bps, boff, rlen);
        std::vector<long long> off(1, 0);
        for (int t = 0; t < n_targets; t++) { long long len; std::cin >> len; off.push_back(off.back() + len); }
        std::cin >> n_hits;
        const int alen = (int)q.size();
        std::vector<std::pair<unsigned, int>> ent;
        for (int h = 0; h < n_hits; h++) {
            long long b, d, p;
            std::cin >> b >> d >> p;
            const long long in_b = d + p - alen;
            if (b < 0 || b >= n_targets || p < 0 || p + k > alen || in_b < 0 || in_b >= off[(size_t)b + 1] - off[(size_t)b]) return 3;
            unsigned code = 0;
            for (int t = 0; t < k; t++) code = (code << 2) | (unsigned)(q[(size_t)(p + t)] - '0');
            ent.push_back({code, (int)(off[(size_t)b] + in_b)});
        }
        std::sort(ent.begin(), ent.end());
        std::vector<unsigned> codes;                 // heap blocks of the exact size
        std::vector<int> gpos;
        for (auto& e : ent) { codes.push_back(e.first); gpos.push_back(e.second); }
        if (codes.empty()) { codes.push_back(0); gpos.push_back(0); }
        tops((int)ent.size(), 1, n_targets);
        std::vector<long long> boff_ll(boff.begin(), boff.end());
        CnsSeqs SB{bps.data(), boff_ll.data(), rlen.data()};
        OvlJob J;
        J.a = 0; J.comp = 0; J.alen = alen; J.stride = J.alen >= k ? seed_stride(J.alen, k, step, list) : step;
        return run_job(SB, J, P, S, codes, gpos, off, 1 + n_targets);
    }
    if (mode != "reads") return 3;
    int n_reads, n_blocks;
    std::cin >> n_reads;
    for (int r = 0; r < n_reads; r++) {
        std::string s;
        std::cin >> s;
        pack(s, bps, boff, rlen);
    }
    std::vector<long long> boff_ll(boff.begin(), boff.end());
    std::cin >> n_blocks;
    for (int blk = 0; blk < n_blocks; blk++) {
        int first, end;
        std::cin >> first >> end;
        SeedIndex ix;
        seed_build_index(bps.data(), boff.data() + first, rlen.data() + first, end - first, k, max_occ, ix);
        printf("index %zu %lld\n", ix.codes.size(), (long long)ix.dropped_codes);
        tops((int)ix.codes.size(), first, end - first);
        std::vector<unsigned> codes(ix.codes);          // heap blocks of the exact size (an empty index: one spare element, never read)
        std::vector<int> gpos(ix.gpos);
        if (codes.empty()) { codes.push_back(0); gpos.push_back(0); }
        std::vector<long long> off(ix.off.begin(), ix.off.end());
        for (int a = 0; a < n_reads; a++)
            for (int comp = 0; comp < 2; comp++) {
                CnsSeqs SB{bps.data(), boff_ll.data(), rlen.data()};
                OvlJob J;
                J.a = a; J.comp = comp; J.alen = rlen[(size_t)a]; J.stride = J.alen >= k ? seed_stride(J.alen, k, step, list) : step;
                const int rc = run_job(SB, J, P, S, codes, gpos, off, n_reads);
                if (rc) return rc;
            }
    }
    return 0;
}
