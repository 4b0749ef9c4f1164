// tests/test_pile_cov_host.py: the ingest's per-read bins and coverage sums (LasPart::finish_facts, hinge_amd/host/host_common.h)
// and what hinge_set_pile_cov makes of them on the host (hinge_amd/csrc/pile_cov_host.h), as a stand-alone host program that
// the test builds under the address and undefined-behaviour sanitizers.
//   driver IN OUT
// IN : int64 n_reads, r_begin, r_end, n_ovl; int32 rlen[n_reads]; int64 row_ptr[n_reads + 1]; int32 a_span[2 * n_ovl]
// OUT: int64 nr, eligible, cov_est, n_long, total_cov, num_slot; int32 nbins40[nr]; int32 cov40[nr]
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../hinge_amd/host/host_common.h"
#include "../../hinge_amd/csrc/pile_cov_host.h"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[4];
    if (!rd(f, h, 4) || h[0] < 0 || h[3] < 0) return 2;
    const size_t n_reads = (size_t)h[0], n_ovl = (size_t)h[3];
    std::vector<int32_t> rlen(n_reads);
    hh::LasPart las;
    las.r_begin = (int)h[1]; las.r_end = (int)h[2];
    las.row_ptr.resize(n_reads + 1);
    las.a_span.resize(2 * n_ovl);
    if (!rd(f, rlen.data(), n_reads) || !rd(f, las.row_ptr.data(), n_reads + 1) || !rd(f, las.a_span.data(), 2 * n_ovl)) return 2;
    fclose(f);
    las.finish_facts((int)n_reads, &rlen);
    const size_t nr = las.nbins40.size();
    if (las.cov40.size() != nr) return 3;
    hinge::PileCovEstimate e;
    if (nr) e = hinge::pile_cov_estimate(rlen.data() + las.r_begin, las.nbins40.data(), las.cov40.data(), nr);
    const int64_t o[6] = {(int64_t)nr, e.eligible ? 1 : 0, e.cov_est, e.n_long, e.total_cov, e.num_slot};
    f = fopen(argv[2], "wb");
    if (!f || !wr(f, o, 6) || !wr(f, las.nbins40.data(), nr) || !wr(f, las.cov40.data(), nr)) return 2;
    fclose(f);
    return 0;
}
