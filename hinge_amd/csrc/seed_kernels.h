// `hinge seed` on the GPU: k-mer placements of reads on the draft.  The first half of a mapper whose second
// half is hinge_trace_local (trace_kernels.h): it says "read r, strand s, contig c, about this diagonal" and aligns nothing.
// Stands where demo/ecoli_demo/run.sh:30-37 runs HPC.daligner's seeding; not a port of it.
//
// Index (index_kernels.h on the device; seed_index.h on the host): every k-mer of every contig at every position, none across two contigs, as (code, gpos) sorted by
// both; code = 2 bits per base, the first base on top; gpos = position in the concatenated contigs (< 2^31); a code with more than
// max_occ entries has none.
// Job = one (read, strand): B = the read in the strand's frame (CnsPair::B), blen its length.
//   hits      sampled positions p = 0, s, 2 s, ... <= blen - k, s = seed_stride() = the smallest multiple of `step` with at most
//             `list` positions.  Every entry of p's code is a hit (d, p, gpos), d = gpos - p + blen (>= 1), enumerated by p, then
//             gpos; hits beyond `list` are dropped in that order (OVERFLOW)
//   window    hits sorted by (d, p) - the key d << 32 | p, unique per hit.  cnt[i] = elements j >= i with d[j] < d[i] + window.
//             Pick: the element seed_better() prefers - the largest cnt, of equal ones the smallest i; its representative is
//             element i + cnt[i] / 2
//   more      picks 2 .. N: the same among elements whose d is at least `window` away from every chosen [d[i], d[i] + window):
//             d <= lo - window or d >= lo + 2 window.  cnt[] stays as it was (it counts all elements).  A pick below min_hits, or
//             below half the first one's (2 cnt < first), ends the picks
//   placement seed_project(): the whole read along the representative's diagonal, clamped to the contig that holds gpos, both
//             sequences cut alike; fewer than k bases left: none.  The host's (seed_capi.inc), as is the order of a read's placements
// HINGE_SEED_MIN_HITS = 3: the largest best-window count of 16 unrelated reads of 7 128 random bases on a random 4.6 Mb draft, both
// strands, at k 15, step 2, window 256 was 2 (30 of the 32 jobs: 1); plus half, rounded up (tools/seed_measure.py min-hits).
//
// Loops.  Every trip count is fixed before its loop from the job's blen and stride and the call's parameters: chunks of 64 sampled
// positions, k bases, the index search's log2 steps (P.search_top, from the index size), max_occ entries, the bitonic network of
// the power of two that holds the hit count, the window search's log2 steps, N picks, six cross-lane steps.  Nothing is read that
// another wavefront writes; jobs are assigned by blockIdx; no atomics; the only barrier is that of the one-wavefront workgroup,
// inside wavefront-uniform loops (the hit count nh is a sum of ballots: the same in every lane).
// Not claimed: chaining, a second stretch of a read on one diagonal, hits inside a repeat of more than max_occ copies, more
// than one GPU.  (Read-vs-read overlaps: overlap_kernels.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "consensus_kernels.h"

namespace hinge {

constexpr int SEED_ST_OK = 0;         // at least one pick
constexpr int SEED_ST_NONE = 1;       // the read is shorter than k, or no window holds min_hits hits
constexpr int SEED_ST_OVERFLOW = 2;   // as OK, but hits beyond `list` were dropped
constexpr int SEED_ST_POISON = -1;    // what the output slots hold before a launch
constexpr int SEED_K_MIN = 8, SEED_K_MAX = 16;
constexpr int SEED_LIST_MIN = 64, SEED_LIST_MAX = 4096;     // 12 bytes of LDS per slot: 24 KiB at the default 2048 (six workgroups per CU)
constexpr int SEED_WINDOW_MIN = 16, SEED_WINDOW_MAX = 65536;
constexpr int SEED_OCC_MAX = 256;
constexpr int SEED_N_MAX = 8;          // HINGE_SEED_MAX_PLACEMENTS_LIMIT of include/hinge_hip.h
constexpr int SEED_HEAD = 4;          // ints in front of a job's picks: status, picks, hits kept, 0

struct SeedJob { int b, comp, blen, stride; };
struct SeedParams {
    int k, window, max_occ, list, n_max, min_hits;
    int n_entries, search_top;        // the index: its entries; the largest power of two <= n_entries (0: none)
};
struct SeedPick { int cnt; unsigned d; int p; int gpos; };   // of the representative
__host__ __device__ inline int seed_out_ints(int n_max) { return SEED_HEAD + 4 * n_max; }
__host__ __device__ inline size_t seed_lds_bytes(int list) { return (size_t)list * (sizeof(unsigned long long) + sizeof(int)); }
__host__ __device__ inline int seed_stride(int blen, int k, int step, int list) {
    const int need = (blen - k) / list + 1;
    return step * ((need + step - 1) / step);
}
// the rule of a pick, for the kernel and the test model alike: the larger count, of equal ones the smaller element
__host__ __device__ inline bool seed_better(int c, int i, int c0, int i0) { return c > c0 || (c == c0 && i < i0); }
// off[0 .. n_contigs]: the contigs' first gpos.  The search: at most 32 halvings of [0, n_contigs)
__host__ __device__ inline bool seed_project(const long long* off, int n_contigs, int k, int gpos, int p, int blen, int* c, int* ab, int* ae, int* bb, int* be) {
    int lo = 0, hi = n_contigs;                                  // the last contig with off <= gpos
    for (int t = 0; t < 32; t++) {
        if (hi - lo <= 1) break;
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= gpos) lo = mid; else hi = mid;
    }
    const long long alen = off[lo + 1] - off[lo], dl = (long long)gpos - off[lo] - p;   // a = b + dl
    long long a0 = dl, a1 = dl + blen, b0 = 0, b1 = blen;
    if (a0 < 0) { b0 = -a0; a0 = 0; }
    if (a1 > alen) { b1 -= a1 - alen; a1 = alen; }
    if (a1 - a0 < k) return false;
    *c = lo; *ab = (int)a0; *ae = (int)a1; *bb = (int)b0; *be = (int)b1;
    return true;
}

#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ int seed_lane_xor(int v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ unsigned long long seed_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
#else   // a host build of the tests (tests/seed_host): the driver supplies the exchanges of its 64 threads
inline int (*seed_lane_xor_host)(int, int) = nullptr;
inline unsigned long long (*seed_ballot_host)(bool) = nullptr;
inline int seed_lane_xor(int v, int m) { return seed_lane_xor_host(v, m); }
inline unsigned long long seed_ballot(bool p) { return seed_ballot_host(p); }
#endif

// One WAVEFRONT (= one 64-thread workgroup) per job.  LDS: keys[list] (d << 32 | p), cnt[list].  out: seed_out_ints(n_max) ints per
// job - status, picks, hits kept, 0, then (cnt, d, p, gpos) per pick -, written by lane 0.
__global__ __launch_bounds__(64) void k_seed_vote(CnsSeqs SB, const SeedJob* __restrict__ jobs, int n_jobs, SeedParams P, const unsigned* __restrict__ codes,
                                                  const int* __restrict__ gpos, int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char seed_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const SeedJob J = jobs[job];
    int* __restrict__ my_out = out + (long long)job * seed_out_ints(P.n_max);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(seed_lds);
    int* cnt = reinterpret_cast<int*>(keys + P.list);
    auto head = [&](int status, int picks, int hits) {
        if (lane == 0) { my_out[0] = status; my_out[1] = picks; my_out[2] = hits; my_out[3] = 0; }
    };
    if (J.blen < P.k || J.stride < 1) { head(SEED_ST_NONE, 0, 0); return; }
    CnsPair Q;
    Q.abps = SB.bps; Q.aoff = 0; Q.bbps = SB.bps; Q.boff = SB.boff[J.b]; Q.comp = J.comp; Q.blen = J.blen;
    // ---- the hits ----------------------------------------------------------------------------------------------------------------
    const int n_pos = min((J.blen - P.k) / J.stride + 1, P.list);            // (the host's stride: never more than list)
    const int n_chunks = (n_pos + 63) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int nh = 0;
    bool over = false;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int x = (ch << 6) + lane;
        const bool act = x < n_pos;
        const int p = x * J.stride;
        unsigned code = 0u;
        for (int t = 0; t < P.k; t++)
            if (act) code = (code << 2) | (unsigned)Q.B(p + t);
        int lo = 0;                                                           // entries below the code
        for (int s = P.search_top; s > 0; s >>= 1)
            if (act && lo + s <= P.n_entries && codes[lo + s - 1] < code) lo += s;
        int occ = 0;                                                          // (sorted: entry o matches only behind entry o - 1)
        for (int o = 0; o < P.max_occ; o++)
            if (act && lo + o < P.n_entries && codes[lo + o] == code) occ++;
        int pre = 0, tot = 0;                                                 // hits of the lanes below; of the chunk
        for (int o = 0; o < P.max_occ; o++) {
            const unsigned long long bal = seed_ballot(occ > o);
            pre += __builtin_popcountll(bal & below);
            tot += __builtin_popcountll(bal);
        }
        for (int o = 0; o < P.max_occ; o++) {
            const int slot = nh + pre + o;
            if (o < occ && slot < P.list) {
                const unsigned d = (unsigned)(gpos[lo + o] - p + J.blen);
                keys[slot] = ((unsigned long long)d << 32) | (unsigned)p;
            }
        }
        if (nh + tot > P.list) over = true;
        nh = min(nh + tot, P.list);
    }
    if (nh == 0) { head(SEED_ST_NONE, 0, 0); return; }                       // (nh: the same in every lane)
    // ---- sorted by (d, p): a bitonic network over the power of two that holds nh, the rest padded with the largest key ------------
    int N = 64;
    for (int t = 0; t < 6; t++)
        if (N < nh) N <<= 1;                                                  // 64 .. 4096 >= nh (nh <= list <= SEED_LIST_MAX)
    for (int x = nh + lane; x < N; x += 64) keys[x] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= N; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (N >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const unsigned long long a = keys[i], b = keys[i + j];
                if ((a > b) == ((i & kk) == 0)) { keys[i] = b; keys[i + j] = a; }
            }
            __syncthreads();
        }
    // ---- cnt[i]: the first element at or behind d[i] + window, less i -------------------------------------------------------------
    for (int i = lane; i < N; i += 64)
        if (i < nh) {
            const unsigned long long target = (keys[i] >> 32) + (unsigned long long)P.window;
            int lo = 0;
            for (int s = N; s > 0; s >>= 1)
                if (lo + s <= nh && (keys[lo + s - 1] >> 32) < target) lo += s;
            cnt[i] = lo - i;
        }
    __syncthreads();
    // ---- the picks ---------------------------------------------------------------------------------------------------------------
    long long c_lo[SEED_N_MAX];
#pragma unroll
    for (int q = 0; q < SEED_N_MAX; q++) c_lo[q] = 0;
    int n_picks = 0, first = 0;
    bool live = true;
    const long long w = P.window;
    for (int n = 0; n < P.n_max; n++) {
        int b_c = -1, b_i = 0x7fffffff;
        for (int i = lane; i < N; i += 64)
            if (live && i < nh) {
                const long long d = (long long)(keys[i] >> 32);
                bool ok = true;
#pragma unroll
                for (int q = 0; q < SEED_N_MAX; q++)
                    if (q < n_picks && !(d <= c_lo[q] - w || d >= c_lo[q] + 2 * w)) ok = false;
                const int c = cnt[i];
                if (ok && seed_better(c, i, b_c, b_i)) { b_c = c; b_i = i; }
            }
        for (int m = 32; m >= 1; m >>= 1) {                                   // all 64 lanes are here: the loops above are wavefront-uniform
            const int o_c = seed_lane_xor(b_c, m), o_i = seed_lane_xor(b_i, m);
            if (seed_better(o_c, o_i, b_c, b_i)) { b_c = o_c; b_i = o_i; }
        }
        if (live && (b_c < max(P.min_hits, 1) || 2 * b_c < first)) live = false;
        if (live) {
            const unsigned long long rep = keys[b_i + b_c / 2];               // (i + cnt[i] - 1 < nh)
            const unsigned d = (unsigned)(rep >> 32);
            const int p = (int)(unsigned)rep;
            if (lane == 0) {
                int* o = my_out + SEED_HEAD + 4 * n_picks;
                o[0] = b_c; o[1] = (int)d; o[2] = p; o[3] = (int)((long long)d + p - J.blen);
            }
            const long long lo_d = (long long)(keys[b_i] >> 32);
#pragma unroll
            for (int q = 0; q < SEED_N_MAX; q++)
                if (q == n_picks) c_lo[q] = lo_d;
            if (n_picks == 0) first = b_c;
            n_picks++;
        }
    }
    head(n_picks == 0 ? SEED_ST_NONE : over ? SEED_ST_OVERFLOW : SEED_ST_OK, n_picks, nh);
}

}  // namespace hinge
