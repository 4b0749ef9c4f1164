// What hinge_set_pile_cov works out on the host from a part's per-read facts (read lengths, bins and sums of the plain
// coverage profiles): the values k_median_hist would produce from the same numbers on the device (filter.cpp:642-678).
// Plain C++, no HIP: tests/test_pile_cov_host.py builds it into a stand-alone program under the host sanitizers.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hinge {

struct PileCovEstimate {
    bool eligible = false;      // every read has nbins >= 0 (the general kernel defines the sum of a read at -1 differently)
    int32_t cov_est = 0;        // element of rank n_long / 2 of the valid means (median_id = size / 2, filter.cpp:660)
    int32_t n_long = 0;         // reads >= 5000 bp (filter.cpp:650); 0: cov_est is undefined in the reference
    int64_t total_cov = 0;      // sum of their sums, sum of their bins (only logged, filter.cpp:666,672)
    int64_t num_slot = 0;
};

// mean coverage of one read (filter.cpp:642-656): C division of the sum by max(1, bins), reads >= 5000 bp only
inline bool pile_cov_mean(int32_t rlen, int32_t nbins, int32_t cov, int32_t* mean) {
    if (rlen < 5000) return false;
    const int32_t m = cov / std::max<int32_t>(1, nbins);
    if (m == INT_MIN) return false;   // (the device's "not in the median" value: cannot be a quotient of an in-range read)
    *mean = m;
    return true;
}

inline PileCovEstimate pile_cov_estimate(const int32_t* rlen, const int32_t* nbins, const int32_t* cov, size_t nr) {
    PileCovEstimate e;
    e.eligible = true;
    std::vector<int32_t> means;
    means.reserve(nr);
    for (size_t k = 0; k < nr; k++) {
        if (nbins[k] < 0) { e.eligible = false; continue; }
        int32_t m;
        if (!pile_cov_mean(rlen[k], nbins[k], cov[k], &m)) continue;
        means.push_back(m);
        e.total_cov += (int64_t)cov[k];
        e.num_slot += (int64_t)nbins[k];
    }
    e.n_long = (int32_t)std::min<size_t>(means.size(), (size_t)INT32_MAX);
    if (!means.empty()) {
        std::nth_element(means.begin(), means.begin() + (ptrdiff_t)(means.size() / 2), means.end());
        e.cov_est = means[means.size() / 2];
    }
    return e;
}

}   // namespace hinge
