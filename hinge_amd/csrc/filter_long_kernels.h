// The long-read tier of `hinge filter`: reads whose coverage profile does not fit a wavefront's LDS slot.
//
// The general kernel (k_mask_annotate, filter_kernels.h) keeps a read's two difference histograms in 2 * kcap ints of LDS per
// wavefront; at four wavefronts per workgroup and 160 KiB that is KCAP_LDS_MAX = 5120 bins, a read of ~204 kb at reso 40.  The
// kernels here run the SAME body (mask_annotate_body, coverage_bins_body) with the histograms - and the candidate list, which in
// LDS overlays the cutoff profile - in a per-wavefront slot of device memory: 3 * kcap ints, kcap from the longest read on the
// list.  The host lists the reads of a part that are too long for LDS (long_reads_prepare in hinge_capi.hip); the LDS kernels
// pass exactly those over, this tier passes every other read over, so whatever list either is given (the fast kernel's hand-backs,
// the guard-band list of a one-sweep pass, a whole part) every read is worked on once.
//
// Memory order.  A wavefront's LDS accesses are ordered among its lanes; its device-memory accesses are not: the histogram is
// built with atomics, which execute in L2, and read back with plain loads, which may hit a line the wavefront's CU cached while it
// worked on its previous read.  DeviceProfiles' call operator is an agent-scope fence (write-back + invalidate of the non-coherent
// levels, all of the wavefront's accesses retired); the body calls it between any two phases of which the second reads what other
// lanes wrote in the first: clear | atomics | scan in place | profile reads, and around the sequential merge of the candidates.
//
// Limits that remain: the annotation code packs (reso * j) << 1 | type into an int (mask_gate_annotate), so a read of 2^30 or more
// bases is refused by the host (HINGE_E_CAPACITY); the scratch is 12 bytes per bin and wavefront of the launch (the host caps the
// wavefronts, and a failed allocation is HINGE_E_DEVICE).
#pragma once
#include "filter_kernels.h"

namespace hinge {

struct DeviceProfiles {
    static constexpr bool LONG = true;
    int* scratch;                 // [wavefronts of the launch][3][kcap]: cutoff-0 histogram, cutoff histogram, candidates
    int kcap_lds;                 // the LDS kernels' kcap: a read with fewer bins is theirs
    const int* all_list;          // every long read of the part and their number (MODE_FINAL after a missed prediction)
    const unsigned* all_count;
    __device__ __forceinline__ void operator()() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); }
};

// One read per wavefront, as the general kernel; read_list / list_count as there (never nullptr: the part's long reads, or the
// guard-band list, of which only the long reads are taken).
template <int RESO>
__global__ __launch_bounds__(BLOCK) void k_mask_annotate_long(FilterDev P, int r_begin, int r_end, const int64_t* __restrict__ row_ptr,
                                                              const int2* __restrict__ a_span, const int* __restrict__ rlen,
                                                              const int* __restrict__ d_min_cov, int kcap, AnnoOut o,
                                                              const int* __restrict__ read_list, const unsigned* __restrict__ list_count, SpecArgs sa,
                                                              DeviceProfiles st) {
    mask_annotate_body<RESO, DeviceProfiles>(P, r_begin, r_end, row_ptr, a_span, rlen, d_min_cov, kcap, o, read_list, list_count, sa,
                                             (int)blockIdx.x, (int)gridDim.x, st);
}

// hinge_filter_coverage_bins for the reads of `list`: those with more bins than a wavefront's LDS histogram of k_coverage_bins
// holds (one array per wavefront there: 2 * KCAP_LDS_MAX bins); one read per wavefront, its histogram scratch[wavefront][kcap].
__global__ __launch_bounds__(BLOCK) void k_coverage_bins_long(int r0, int r1, const int64_t* __restrict__ row_ptr, const int2* __restrict__ a_span,
                                                              int reso, int cutoff, int kcap, int* __restrict__ nbins,
                                                              const int64_t* __restrict__ out_off, int* __restrict__ cov, int* __restrict__ status,
                                                              int* __restrict__ scratch, const int* __restrict__ list, int n_list) {
    coverage_bins_body<true>(r0, r1, row_ptr, a_span, reso, cutoff, kcap, nbins, out_off, cov, status, 0, scratch, list, n_list);
}

}  // namespace hinge
