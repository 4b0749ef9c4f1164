// The k-mer index of `hinge seed` (seed_kernels.h, "Index"): host C++, no kernel.  Built once per hinge_seed_run from the draft
// DB's packed bases and uploaded; tests/seed_host/driver.cpp builds the same one.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace hinge {

struct SeedIndex {
    std::vector<uint32_t> codes;      // sorted by (code, gpos)
    std::vector<int32_t> gpos;
    std::vector<long long> off;       // [n_contigs + 1]: a contig's first gpos
    int64_t dropped_codes = 0;        // codes with more than max_occ entries
};

// bps: 2 bits per base, four per byte, the first base in the top bits; contig i = rlen[i] bases from byte boff[i].  The caller has
// checked that the contigs total less than 2^31 bases.
inline void seed_build_index(const uint8_t* bps, const int64_t* boff, const int32_t* rlen, int n_contigs, int k, int max_occ, SeedIndex& ix) {
    ix.off.assign((size_t)n_contigs + 1, 0);
    for (int c = 0; c < n_contigs; c++) ix.off[(size_t)c + 1] = ix.off[(size_t)c] + rlen[c];
    std::vector<uint64_t> e;                                     // code << 32 | gpos
    e.reserve((size_t)ix.off[(size_t)n_contigs]);
    const uint32_t mask = k >= 16 ? 0xffffffffu : ((1u << (2 * k)) - 1u);
    for (int c = 0; c < n_contigs; c++) {
        const uint8_t* s = bps + boff[c];
        uint32_t code = 0;
        for (int x = 0; x < rlen[c]; x++) {
            code = ((code << 2) | ((s[x >> 2] >> (6 - 2 * (x & 3))) & 3u)) & mask;
            if (x >= k - 1) e.push_back(((uint64_t)code << 32) | (uint64_t)(ix.off[(size_t)c] + x - (k - 1)));
        }
    }
    std::sort(e.begin(), e.end());
    ix.codes.clear(); ix.gpos.clear(); ix.dropped_codes = 0;
    for (size_t i = 0; i < e.size();) {
        size_t j = i;
        while (j < e.size() && (e[j] >> 32) == (e[i] >> 32)) j++;
        if (j - i > (size_t)max_occ) ix.dropped_codes++;
        else
            for (size_t x = i; x < j; x++) { ix.codes.push_back((uint32_t)(e[x] >> 32)); ix.gpos.push_back((int32_t)(e[x] & 0xffffffffu)); }
        i = j;
    }
}

}  // namespace hinge
