// tests/test_index_host.py: the kernels of hinge_amd/csrc/index_kernels.h (a copy made by the test, beside the host stand-ins of
// tests/trace_host) run on the CPU - a wavefront = 64 threads in lock step, a launch = its workgroups one after the other - under
// AddressSanitizer and UBSan, in the launch order of index_capi.inc, with guard words around every output and scratch array and
// behind the LDS in use; compared here with seed_build_index (seed_index.h) and printed for the numpy model.  The ballot is an
// array of 64 slots between two barriers.
// stdin: "k max_occ", "n_reads" and the reads (bases as digits 0-3, as stored; "-" = an empty read), "n_ranges" and per range
// "first end".  stdout per range: "index ENTRIES KEPT DROPPED PASSES", then the lines of codes, gpos and off.
// Or stdin: "scan LEN SEED MAX_VALUE" - the scan alone, at lengths a whole build would take minutes to reach here (scan_mode).
#include "index_kernels.h"
#include "seed_index.h"
#include <pthread.h>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <string>
#include <thread>
#include <vector>
thread_local Idx3 threadIdx, blockIdx;
namespace hinge {
unsigned char idx_lds[IDX_LDS_BYTES + 256];
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

// A heap block of n elements between two rows of GUARD guard words.
template <class T> struct Guarded {
    static constexpr int GUARD = 8;
    std::vector<T> v;
    size_t n;
    explicit Guarded(size_t n_, T fill) : v(n_ + 2 * GUARD, fill), n(n_) {
        for (int g = 0; g < GUARD; g++) { v[(size_t)g] = mark(); v[n + GUARD + (size_t)g] = mark(); }
    }
    static T mark() { return (T)0x5a5a5a5a5a5a5a5aull; }
    T* p() { return v.data() + GUARD; }
    bool ok() const {
        for (int g = 0; g < GUARD; g++) if (v[(size_t)g] != mark() || v[n + GUARD + (size_t)g] != mark()) return false;
        return true;
    }
};

static bool lds_ok = true;
// One launch: 64 threads walk the grid's workgroups in order, all of them at the barrier between two workgroups.
static void launch(long long grid, const std::function<void()>& kernel) {
    memset(idx_lds, 0xa5, sizeof(idx_lds));
    pthread_barrier_init(&bar, nullptr, 64);
    std::vector<std::thread> th;
    for (int l = 0; l < 64; l++)
        th.emplace_back([&, l] {
            for (long long b = 0; b < grid; b++) {
                threadIdx = Idx3{(unsigned)l, 0, 0};
                blockIdx = Idx3{(unsigned)b, 0, 0};
                kernel();
                pthread_barrier_wait(&bar);
            }
        });
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&bar);
    for (size_t g = IDX_LDS_BYTES; g < sizeof(idx_lds); g++) if (idx_lds[g] != 0xa5) lds_ok = false;
}

static long long sums_elems(long long len) {
    long long tot = 0;
    while (len > IDX_SCAN_CHUNK) { len = idx_chunks(len); tot += len; }
    return tot;
}
static void scan(unsigned* a, long long len, unsigned* sums) {
    const long long nb = idx_chunks(len);
    if (nb > 1) {
        launch(nb, [&] { k_index_scan_sums(a, len, sums); });
        scan(sums, nb, sums + nb);
    }
    launch(std::max(nb, 1ll), [&] { k_index_scan_apply(a, len, nb > 1 ? sums : nullptr); });
}

// "scan LEN SEED MAX_VALUE": LEN values in [0, MAX_VALUE] through scan() - the real k_index_scan_sums and k_index_scan_apply, the
// recursion and the carving of the one sums array as index_scan (index_capi.inc) has them - against a serial exclusive scan.
// stdout: "scan LEN LEVELS SUMS_ELEMS TOTAL".
static int scan_mode() {
    long long len;
    unsigned long long seed;
    unsigned max_value;
    std::cin >> len >> seed >> max_value;
    if (!std::cin || len < 1) { printf("BAD scan arguments\n"); return 2; }
    Guarded<unsigned> a((size_t)len, 0u), sums((size_t)std::max(sums_elems(len), 1ll), ~0u);
    std::vector<unsigned> want((size_t)len);
    unsigned long long x = seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull, total = 0;
    for (long long i = 0; i < len; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;                                  // xorshift64
        const unsigned v = (unsigned)((x >> 20) % ((unsigned long long)max_value + 1ull));
        a.p()[i] = v;
        want[(size_t)i] = (unsigned)total;
        total += v;
    }
    if (total >= (1ull << 31)) { printf("BAD scan total %llu\n", total); return 2; }
    scan(a.p(), len, sums.p());
    if (!a.ok() || !sums.ok()) { printf("GUARD array\n"); return 4; }
    if (!lds_ok) { printf("GUARD lds\n"); return 4; }
    for (long long i = 0; i < len; i++)
        if (a.p()[i] != want[(size_t)i]) { printf("MISMATCH scan at %lld: %u, not %u\n", i, a.p()[i], want[(size_t)i]); return 6; }
    int levels = 1;
    for (long long l = len; l > IDX_SCAN_CHUNK; l = idx_chunks(l)) levels++;
    printf("scan %lld %d %lld %llu\n", len, levels, sums_elems(len), total);
    return 0;
}

int main() {
    int k, max_occ, n_reads, n_ranges;
    std::string word;
    std::cin >> word;
    if (word == "scan") return scan_mode();
    k = std::stoi(word);
    std::cin >> max_occ >> n_reads;
    std::vector<unsigned char> bps;
    std::vector<int64_t> boff;
    std::vector<int32_t> rlen;
    for (int r = 0; r < n_reads; r++) {
        std::string s;
        std::cin >> s;
        if (s == "-") s.clear();
        boff.push_back((int64_t)bps.size());
        rlen.push_back((int32_t)s.size());
        std::vector<unsigned char> o((s.size() + 3) / 4, 0);
        for (size_t p = 0; p < s.size(); p++) o[p >> 2] |= (unsigned char)((s[p] - '0') << (6 - 2 * (p & 3)));
        bps.insert(bps.end(), o.begin(), o.end());
    }
    if (bps.empty()) bps.push_back(0);
    std::vector<long long> boff_ll(boff.begin(), boff.end());
    seed_lane_xor_host = lane_xor;
    seed_ballot_host = ballot;
    std::cin >> n_ranges;
    for (int rg = 0; rg < n_ranges; rg++) {
        int first, end;
        std::cin >> first >> end;
        const int nr = end - first;
        SeedIndex ix;
        seed_build_index(bps.data(), boff.data() + first, rlen.data() + first, nr, k, max_occ, ix);
        // ---- the device build, launch by launch as index_build_device (index_capi.inc) has it --------------------------------------
        Guarded<long long> off((size_t)nr + 1, 0), eoff((size_t)nr + 1, 0);
        for (int c = 0; c < nr; c++) {
            off.p()[c + 1] = off.p()[c] + rlen[(size_t)(first + c)];
            eoff.p()[c + 1] = eoff.p()[c] + std::max(rlen[(size_t)(first + c)] - k + 1, 0);
        }
        const long long n = eoff.p()[nr];
        long long kept = 0, drop = 0;
        std::vector<unsigned> codes;
        std::vector<int> gpos;
        if (n > 0) {
            const long long n_tiles = idx_tiles(n), table_len = (long long)IDX_DIGITS * n_tiles;
            Guarded<unsigned long long> ping((size_t)n, ~0ull), pong((size_t)n, ~0ull);
            Guarded<unsigned> table((size_t)table_len, ~0u), sums((size_t)std::max(sums_elems(std::max(table_len, n + 1)), 1ll), ~0u), scal(4, 0u);
            CnsSeqs SB{bps.data(), boff_ll.data(), rlen.data()};
            int seq_top = 0, occ_top = 0;
            for (long long v = 1; v <= (long long)nr; v <<= 1) seq_top = (int)v;
            for (int v = 1; v <= max_occ; v <<= 1) occ_top = v;
            unsigned long long* src = ping.p();
            unsigned long long* dst = pong.p();
            launch((n + 63) / 64, [&] { k_index_extract(SB, first, nr, seq_top, k, off.p(), eoff.p(), (int)n, src); });
            for (int pass = 0; pass < idx_passes(k); pass++) {
                const int shift = 32 + 8 * pass;
                launch(n_tiles, [&] { k_index_hist(src, (int)n, shift, n_tiles, table.p()); });
                scan(table.p(), table_len, sums.p());
                launch(n_tiles, [&] { k_index_scatter(src, dst, (int)n, shift, n_tiles, table.p()); });
                std::swap(src, dst);
            }
            // the flags: n + 1 words in the free one of the two pair arrays (8 n bytes >= 4 (n + 1)), the rest of it a guard of its own
            unsigned* flags = reinterpret_cast<unsigned*>(dst);
            memset(flags, 0xff, sizeof(unsigned long long) * (size_t)n);
            launch((n + 1 + 63) / 64, [&] { k_index_flag(src, (int)n, max_occ, occ_top, flags, scal.p()); });
            scan(flags, n + 1, sums.p());
            for (long long x = n + 1; x < 2 * n; x++) if (flags[x] != ~0u) { printf("GUARD flags\n"); return 4; }
            kept = flags[n]; drop = scal.p()[0];
            if (kept > n || kept + drop * ((long long)max_occ + 1) > n) { printf("COUNTS %lld %lld %lld\n", n, kept, drop); return 5; }
            Guarded<unsigned> o_codes((size_t)kept, ~0u);
            Guarded<int> o_gpos((size_t)kept, -1);
            launch((n + 63) / 64, [&] { k_index_compact(src, flags, (int)n, (unsigned)kept, o_codes.p(), o_gpos.p()); });
            if (!ping.ok() || !pong.ok() || !table.ok() || !sums.ok() || !scal.ok() || !o_codes.ok() || !o_gpos.ok() || !off.ok() || !eoff.ok()) { printf("GUARD array\n"); return 4; }
            if (!lds_ok) { printf("GUARD lds\n"); return 4; }
            codes.assign(o_codes.p(), o_codes.p() + kept);
            gpos.assign(o_gpos.p(), o_gpos.p() + kept);
        }
        // ---- against the host build, value for value ---------------------------------------------------------------------------
        if ((size_t)kept != ix.codes.size() || drop != ix.dropped_codes || codes != ix.codes || gpos != ix.gpos) { printf("MISMATCH host %lld %zu %lld %lld\n", kept, ix.codes.size(), drop, (long long)ix.dropped_codes); return 6; }
        for (int c = 0; c <= nr; c++) if (off.p()[c] != ix.off[(size_t)c]) { printf("MISMATCH off\n"); return 6; }
        printf("index %lld %lld %lld %d\n", n, kept, drop, idx_passes(k));
        for (size_t x = 0; x < codes.size(); x++) printf("%s%u", x ? " " : "", codes[x]);
        printf("\n");
        for (size_t x = 0; x < gpos.size(); x++) printf("%s%d", x ? " " : "", gpos[x]);
        printf("\n");
        for (int c = 0; c <= nr; c++) printf("%s%lld", c ? " " : "", off.p()[c]);
        printf("\n");
    }
    return 0;
}
