// The k-mer index of `hinge seed` and `hinge overlap`, built on the GPU: value for value what
// seed_build_index (seed_index.h) gives - (code, gpos) of every k-mer of the sequences [first, first + n_seqs) of DB 0 sorted by
// both, codes of more than max_occ entries left out - written into the arrays k_seed_vote and k_overlap_vote read.
//
//   extract   one thread per entry slot.  Sequence c of the range has max(rlen - k + 1, 0) entries from slot eoff[c] on and its
//             bases from gpos off[c] on (both running sums are the host's: two small uploads); c = the last sequence with
//             eoff[c] <= slot, by a fixed-trip search.  The code is read from the k bases themselves (2 bits per base, the first on
//             top), so no mask is needed: k <= 16 bases fill at most 32 bits.  pair = code << 32 | gpos, in ascending gpos
//   sort      LSD radix sort of the pairs by code alone, 8-bit digits, ceil(2 k / 8) passes, each STABLE - and since the input is
//             in ascending gpos, the result is in (code, gpos) order.  A pass: k_index_hist (per tile of IDX_TILE entries the
//             count of every digit, into table[digit][tile]), the exclusive scan of that table in (digit, tile) order, and
//             k_index_scatter (the same walk again: an entry goes to table[digit][tile] + its rank among the tile's entries of
//             that digit).  One wavefront per tile takes the tile's rows of 64 entries in order; an entry's rank = the digit's
//             running count in LDS + the lower lanes of the row with the same digit (idx_peers: nine ballots); the lowest lane of
//             every digit of the row then adds the row's count.  No atomics: the lanes that write a row's counts hold distinct digits
//   scan      exclusive, in place, 32-bit (every total is an entry count < 2^31): chunks of IDX_SCAN_CHUNK elements, one wavefront
//             each - k_index_scan_sums (a chunk's total), the same scan over the totals (the host recurses: at most three levels
//             below 2^31 + 1 elements), k_index_scan_apply (the chunk's own scan on top of its base)
//   filter    k_index_flag on the sorted pairs: an entry's run = itself + the equal codes among the max_occ entries in front of
//             it + among the max_occ behind it, each found by a fixed-trip search (equal codes are contiguous); that is the true
//             run length where it is <= max_occ and more than max_occ otherwise.  flag = the run is kept; a dropped run's head
//             (no equal code in front) counts one dropped code.  The flags (and a 0 behind them) are scanned by the scan above:
//             scan[n] = entries kept; k_index_compact writes entry i to codes[scan[i]], gpos[scan[i]] if scan[i + 1] != scan[i]
//
// Loops.  Every trip count is fixed before its loop from the launch's arguments: the sequence search's log2 steps (seq_top), k
// bases, IDX_ROWS rows of a tile, eight digit bits, 256 / 64 digits per lane, IDX_SCAN_PER_LANE elements, 64 lanes, the run
// searches' log2 steps (occ_top).  Inside one launch nothing is read that another workgroup writes (no look-back, no flag, no
// spin); what one launch writes the next one reads.  Workgroups are one wavefront; tiles and chunks are assigned by blockIdx.
// The one atomic is the integer count of dropped codes (a sum: the same in any order), one add per wavefront that has any.
// Entry indices are below 2^31; tile bases, table indices and byte offsets are 64-bit.
// Not claimed: an LDS reorder in front of the scatter's stores (a row's 64 stores go to up to 64 places); more than one GPU.
#pragma once
#include "seed_kernels.h"

namespace hinge {

constexpr int IDX_ROWS = 32;                         // rows of 64 entries a wavefront takes in order
constexpr int IDX_TILE = 64 * IDX_ROWS;              // entries per tile (hinge_index_tile)
constexpr int IDX_DIGITS = 256;
constexpr int IDX_SCAN_PER_LANE = 32;
constexpr int IDX_SCAN_CHUNK = 64 * IDX_SCAN_PER_LANE;
constexpr int IDX_LDS_BYTES = IDX_DIGITS * (int)sizeof(unsigned);   // the digit counts of hist and scatter; the scan uses the first 64 words

__host__ __device__ inline int idx_passes(int k) { return (2 * k + 7) / 8; }
__host__ __device__ inline long long idx_tiles(long long n) { return (n + IDX_TILE - 1) / IDX_TILE; }
__host__ __device__ inline long long idx_chunks(long long n) { return (n + IDX_SCAN_CHUNK - 1) / IDX_SCAN_CHUNK; }

#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ void idx_count_add(unsigned* p, unsigned v) { atomicAdd(p, v); }
#else   // a host build of the tests (tests/index_host)
inline void idx_count_add(unsigned* p, unsigned v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#endif

// The lanes of the row that are active and hold the same digit as this one (meaningless in an inactive lane).  Every lane calls it.
__device__ __forceinline__ unsigned long long idx_peers(unsigned d, bool act) {
    unsigned long long m = seed_ballot(act);
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = seed_ballot(act && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// grid: one workgroup per 64 slots.  eoff[0 .. n_seqs], off[0 .. n_seqs]: see above; seq_top = the largest power of two <= n_seqs.
__global__ __launch_bounds__(64) void k_index_extract(CnsSeqs SB, int first, int n_seqs, int seq_top, int k, const long long* __restrict__ off, const long long* __restrict__ eoff,
                                                      int n_entries, unsigned long long* __restrict__ pairs) {
    const long long slot = (long long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= n_entries) return;
    int c = 0;                                                                // the last sequence with eoff <= slot: the one that holds it
    for (int s = seq_top; s > 0; s >>= 1)
        if (c + s < n_seqs && eoff[c + s] <= slot) c += s;
    const int p = (int)(slot - eoff[c]);                                      // the k-mer's first base (<= rlen - k)
    const long long boff = SB.boff[first + c];
    unsigned code = 0u;
    for (int t = 0; t < k; t++) code = (code << 2) | (unsigned)cns_base(SB.bps, boff, p + t);
    pairs[slot] = ((unsigned long long)code << 32) | (unsigned long long)(off[c] + p);
}

// grid: one workgroup per tile.  table[digit * n_tiles + tile] = the tile's entries of that digit (every slot is written).
__global__ __launch_bounds__(64) void k_index_hist(const unsigned long long* __restrict__ in, int n, int shift, long long n_tiles, unsigned* __restrict__ table) {
    extern __shared__ __align__(16) unsigned char idx_lds[];
    unsigned* cnt = reinterpret_cast<unsigned*>(idx_lds);
    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int d = lane; d < IDX_DIGITS; d += 64) cnt[d] = 0u;
    __syncthreads();
    for (int row = 0; row < IDX_ROWS; row++) {
        const long long i = tile * IDX_TILE + row * 64 + lane;
        const bool act = i < n;
        const unsigned d = act ? (unsigned)(in[i] >> shift) & 0xffu : 0u;
        const unsigned long long peers = idx_peers(d, act);
        if (act && (peers & below) == 0ull) cnt[d] += (unsigned)__builtin_popcountll(peers);   // one lane per digit of the row
        __syncthreads();
    }
    for (int d = lane; d < IDX_DIGITS; d += 64) table[(long long)d * n_tiles + tile] = cnt[d];
}

// grid: one workgroup per tile.  table: k_index_hist's after the exclusive scan - where the tile's first entry of every digit goes.
__global__ __launch_bounds__(64) void k_index_scatter(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out, int n, int shift, long long n_tiles,
                                                      const unsigned* __restrict__ table) {
    extern __shared__ __align__(16) unsigned char idx_lds[];
    unsigned* cnt = reinterpret_cast<unsigned*>(idx_lds);
    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int d = lane; d < IDX_DIGITS; d += 64) cnt[d] = table[(long long)d * n_tiles + tile];
    __syncthreads();
    for (int row = 0; row < IDX_ROWS; row++) {
        const long long i = tile * IDX_TILE + row * 64 + lane;
        const bool act = i < n;
        const unsigned long long v = act ? in[i] : 0ull;
        const unsigned d = (unsigned)(v >> shift) & 0xffu;
        const unsigned long long peers = idx_peers(d, act);
        const unsigned base = act ? cnt[d] : 0u;
        __syncthreads();                                                      // every lane has the row's bases before one of them moves on
        if (act) {
            const unsigned dest = base + (unsigned)__builtin_popcountll(peers & below);
            if (dest < (unsigned)n) out[dest] = v;                            // (always, with a table that sums to n)
            if ((peers & below) == 0ull) cnt[d] = base + (unsigned)__builtin_popcountll(peers);
        }
        __syncthreads();
    }
}

// grid: one workgroup per chunk.  sums[chunk] = the sum of its elements.
__global__ __launch_bounds__(64) void k_index_scan_sums(const unsigned* __restrict__ a, long long n, unsigned* __restrict__ sums) {
    extern __shared__ __align__(16) unsigned char idx_lds[];
    unsigned* part = reinterpret_cast<unsigned*>(idx_lds);
    const int lane = threadIdx.x;
    const long long at = (long long)blockIdx.x * IDX_SCAN_CHUNK + (long long)lane * IDX_SCAN_PER_LANE;
    unsigned s = 0u;
    for (int t = 0; t < IDX_SCAN_PER_LANE; t++)
        if (at + t < n) s += a[at + t];
    part[lane] = s;
    __syncthreads();
    unsigned tot = 0u;
    for (int l = 0; l < 64; l++) tot += part[l];
    if (lane == 0) sums[blockIdx.x] = tot;
}

// grid: one workgroup per chunk.  a[] becomes its exclusive scan; base[chunk] = what lies in front of the chunk (nullptr: nothing).
__global__ __launch_bounds__(64) void k_index_scan_apply(unsigned* __restrict__ a, long long n, const unsigned* __restrict__ base) {
    extern __shared__ __align__(16) unsigned char idx_lds[];
    unsigned* part = reinterpret_cast<unsigned*>(idx_lds);
    const int lane = threadIdx.x;
    const long long at = (long long)blockIdx.x * IDX_SCAN_CHUNK + (long long)lane * IDX_SCAN_PER_LANE;
    unsigned s = 0u;
    for (int t = 0; t < IDX_SCAN_PER_LANE; t++)
        if (at + t < n) s += a[at + t];
    part[lane] = s;
    __syncthreads();
    unsigned run = base ? base[blockIdx.x] : 0u;
    for (int l = 0; l < 64; l++)
        if (l < lane) run += part[l];
    for (int t = 0; t < IDX_SCAN_PER_LANE; t++)
        if (at + t < n) {
            const unsigned v = a[at + t];
            a[at + t] = run;
            run += v;
        }
}

// grid: one workgroup per 64 of the n + 1 flags.  occ_top = the largest power of two <= max_occ.  *dropped: zero before the launch.
__global__ __launch_bounds__(64) void k_index_flag(const unsigned long long* __restrict__ sorted, int n, int max_occ, int occ_top, unsigned* __restrict__ flags,
                                                   unsigned* __restrict__ dropped) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool act = i < n;
    bool head_dropped = false;
    if (act) {
        const unsigned code = (unsigned)(sorted[i] >> 32);
        int back = 0, fwd = 0;                                                // equal codes in front and behind, at most max_occ each
        for (int s = occ_top; s > 0; s >>= 1)
            if (back + s <= max_occ && i - (back + s) >= 0 && (unsigned)(sorted[i - (back + s)] >> 32) == code) back += s;
        for (int s = occ_top; s > 0; s >>= 1)
            if (fwd + s <= max_occ && i + (fwd + s) < n && (unsigned)(sorted[i + (fwd + s)] >> 32) == code) fwd += s;
        const bool keep = back + fwd + 1 <= max_occ;
        flags[i] = keep ? 1u : 0u;
        head_dropped = !keep && back == 0;
    } else if (i == n) flags[i] = 0u;
    const unsigned long long bal = seed_ballot(head_dropped);
    if (threadIdx.x == 0 && bal != 0ull) idx_count_add(dropped, (unsigned)__builtin_popcountll(bal));
}

// grid: one workgroup per 64 entries.  scan[0 .. n]: the flags after the exclusive scan; cap = scan[n], as the host read it.
__global__ __launch_bounds__(64) void k_index_compact(const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ scan, int n, unsigned cap,
                                                      unsigned* __restrict__ codes, int* __restrict__ gpos) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const unsigned at = scan[i];
    if (scan[i + 1] == at || at >= cap) return;
    const unsigned long long v = sorted[i];
    codes[at] = (unsigned)(v >> 32);
    gpos[at] = (int)(unsigned)(v & 0xffffffffull);
}

}  // namespace hinge
