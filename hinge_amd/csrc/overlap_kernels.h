// `hinge overlap` on the GPU: read-vs-read overlap candidates by k-mer votes.  The all-vs-all search in
// front of hinge_trace_local (trace_kernels.h): it says "reads a and b, strand s, about this diagonal" and aligns nothing.
// Stands where the reference's run script calls DALIGNER on the read DB against itself; not a port of it.
//
// Index (index_kernels.h on the device or seed_index.h on the host; one per target BLOCK of consecutive reads): every k-mer of every read of the block at every position,
// none across two reads, as (code, gpos) sorted by both; gpos = position in the block's concatenated reads (< 2^31); a code with
// more than max_occ entries in the block has none.  One block is resident at a time.
// Job = (query read a, strand, the resident block): Q = read a in the strand's frame (CnsPair::B), alen its length; targets forward.
//   hits      sampled positions p as in k_seed_vote (seed_stride).  Every entry of p's code is a hit (b, d, p): b = the read of
//             the block that holds gpos, d = (gpos - off[b]) - p + alen (>= 1).  Hits with b == a are discarded BEFORE the list is
//             cut (they take no slot); the others are enumerated by p, then gpos; those beyond `list` are dropped (OVERFLOW)
//   groups    hits sorted by (b, d, p) - the key b << 41 | d << 20 | p, unique per hit.  cnt[i] = elements j >= i of the same b with
//             d[j] < d[i] + window.  Per b the pick is the element seed_better() prefers - the largest cnt, of equal ones the smallest
//             i; its representative is element i + cnt[i] / 2.  A pick of cnt >= min_hits is a candidate (b, cnt, d, p) of the
//             representative: one per (a, b, strand)
//   output    candidates in ascending b into max_partners slots; further ones are dropped (TRUNCATED)
// Key packing, and what the host checks before any launch (HINGE_E_CAPACITY): p in 20 bits - every read shorter than 2^20 bases
// (OVL_READ_MAX); d < alen + blen in 21 bits; b in 23 bits - at most 2^23 - 1 reads per block (the all-ones key pads the sort); a
// block below 2^31 bases.
// LDS: 16 bytes per slot - the 64-bit key and two 32-bit words (cnt packed with its element, ping and pong of the scan).  A
// workgroup may take the CU's 160 KiB: 10 240 slots, so the largest `list` (a power of two) is OVL_LIST_MAX = 8192 (128 KiB; one
// workgroup per CU).  The default 4096 takes 64 KiB (two per CU).  cnt <= list and the element both fit 16 bits up to that list.
// HINGE_OVERLAP_MIN_HITS = 6: the largest group count over all pairs of 400 unrelated reads of 7 128 random bases, both strands, at
// k 15, step 2, window 256 was 4; plus half (tools/overlap_measure.py min-hits).  max_occ = 64: see include/hinge_hip.h ("hinge overlap") and tools/overlap_measure.py.
//
// Loops.  Every trip count is fixed before its loop from the job's alen and stride and the call's parameters: chunks of 64 sampled
// positions, k bases, the index search's log2 steps, max_occ entries, the offset search's log2 steps (P.read_top), the bitonic
// network of the power of two N that holds the hit count, the window search's log2 steps, the segmented scan's log2 N steps (the
// per-group reduction: element i takes the better of itself and element i + s while both have the same b), N / 64 chunks of the
// candidate ranking.  Nothing is read that another wavefront writes; jobs are assigned by blockIdx; no atomics; the only barrier is
// that of the one-wavefront workgroup, inside wavefront-uniform loops (nh and N are sums of ballots: the same in every lane).
// Not claimed: chaining; a second stretch of the same pair (k_overlap_vote_multi, overlap_multi_kernels.h, finds those); k-mers of more than max_occ copies per block; reads of 2^20 or more
// bases; more than one GPU; parity with DALIGNER's record set.
#pragma once
#include "seed_kernels.h"

namespace hinge {

constexpr int OVL_ST_OK = 0;          // at least one candidate
constexpr int OVL_ST_NONE = 1;        // the read is shorter than k, or no group holds min_hits hits
constexpr int OVL_ST_OVERFLOW = 2;    // bit: hits beyond `list` were dropped
constexpr int OVL_ST_TRUNCATED = 4;   // bit: candidates beyond max_partners were dropped
constexpr int OVL_P_BITS = 20, OVL_D_BITS = 21, OVL_B_BITS = 23;
constexpr int OVL_READ_MAX = (1 << OVL_P_BITS) - 1;              // the longest read
constexpr int OVL_BLOCK_READS_MAX = (1 << OVL_B_BITS) - 1;       // the most reads of a block
constexpr int OVL_LDS_MAX = 160 * 1024;                          // what a workgroup may take of a gfx950 CU
constexpr int OVL_SLOT_BYTES = 16;
constexpr int OVL_LIST_MIN = 64, OVL_LIST_MAX = 8192;            // the largest power of two with list * OVL_SLOT_BYTES <= OVL_LDS_MAX
constexpr int OVL_PARTNERS_MAX = 4096;
constexpr int OVL_HEAD = 4;           // ints in front of a job's candidates: status, candidates, hits kept, 0
static_assert(OVL_P_BITS + OVL_D_BITS + OVL_B_BITS == 64, "the key is 64 bits");
static_assert((long long)OVL_LIST_MAX * OVL_SLOT_BYTES <= OVL_LDS_MAX && 2ll * OVL_LIST_MAX * OVL_SLOT_BYTES > OVL_LDS_MAX, "OVL_LIST_MAX follows from the LDS size");
static_assert(OVL_LIST_MAX <= 65535, "cnt and the element share a 32-bit word");

struct OvlJob { int a, comp, alen, stride; };
struct OvlParams {
    int k, window, max_occ, list, max_partners, min_hits;
    int n_entries, search_top;        // the block's index: its entries; the largest power of two <= n_entries (0: none)
    int first, n_reads, read_top;     // the block: its first read, its reads; the largest power of two <= n_reads
};
__host__ __device__ inline int ovl_out_ints(int max_partners) { return OVL_HEAD + 4 * max_partners; }
__host__ __device__ inline size_t ovl_lds_bytes(int list) { return (size_t)list * OVL_SLOT_BYTES; }
// The overlap of a candidate (d, p) as a record: A = read a forward, B = read b in the comp frame.  In the job's frame target base
// t of b lies under query base q = t - dl of a, dl = d - alen; the whole of both reads along that diagonal, clamped to both; fewer
// than k bases left: none.  *diag = bbpos - abpos.
__host__ __device__ inline bool overlap_project(int alen, int blen, int comp, long long d, int k, int* ab, int* ae, int* bb, int* be, int* diag) {
    const long long dl = d - alen;
    long long q0 = 0, q1 = alen;
    if (dl < 0) q0 = -dl;
    if (q1 + dl > blen) q1 = blen - dl;
    if (q1 - q0 < k) return false;
    const long long t0 = q0 + dl, t1 = q1 + dl;
    if (!comp) { *ab = (int)q0; *ae = (int)q1; *bb = (int)t0; *be = (int)t1; }
    else { *ab = (int)(alen - q1); *ae = (int)(alen - q0); *bb = (int)(blen - t1); *be = (int)(blen - t0); }
    *diag = *bb - *ab;
    return true;
}

// One WAVEFRONT (= one 64-thread workgroup) per job.  LDS: keys[list], va[list], vb[list].  out: ovl_out_ints(max_partners) ints per
// job - status, candidates, hits kept, 0, then (b, cnt, d, p) per candidate, b a read id of the DB.  off[0 .. n_reads]: the block's
// reads' first gpos.
__global__ __launch_bounds__(64) void k_overlap_vote(CnsSeqs SB, const OvlJob* __restrict__ jobs, int n_jobs, OvlParams P, const unsigned* __restrict__ codes,
                                                     const int* __restrict__ gpos, const long long* __restrict__ off, int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char ovl_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const OvlJob J = jobs[job];
    int* __restrict__ my_out = out + (long long)job * ovl_out_ints(P.max_partners);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ovl_lds);
    unsigned* va = reinterpret_cast<unsigned*>(keys + P.list);
    unsigned* vb = va + P.list;
    auto head = [&](int status, int cands, int hits) {
        if (lane == 0) { my_out[0] = status; my_out[1] = cands; my_out[2] = hits; my_out[3] = 0; }
    };
    if (J.alen < P.k || J.stride < 1) { head(OVL_ST_NONE, 0, 0); return; }
    CnsPair Q;
    Q.abps = SB.bps; Q.aoff = 0; Q.bbps = SB.bps; Q.boff = SB.boff[J.a]; Q.comp = J.comp; Q.blen = J.alen;
    const int a_loc = J.a - P.first;                                          // the query's place in the block, if it has one
    const bool a_in = a_loc >= 0 && a_loc < P.n_reads;
    const long long self_lo = a_in ? off[a_loc] : 0, self_hi = a_in ? off[a_loc + 1] : 0;
    // ---- the hits ----------------------------------------------------------------------------------------------------------------
    const int n_pos = min((J.alen - P.k) / J.stride + 1, P.list);            // (the host's stride: never more than list)
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
        int occ = 0;                                                          // the code's entries outside the query itself
        for (int o = 0; o < P.max_occ; o++)
            if (act && lo + o < P.n_entries && codes[lo + o] == code) {
                const long long g = gpos[lo + o];
                if (g < self_lo || g >= self_hi) occ++;
            }
        int pre = 0, tot = 0;                                                 // hits of the lanes below; of the chunk
        for (int o = 0; o < P.max_occ; o++) {
            const unsigned long long bal = seed_ballot(occ > o);
            pre += __builtin_popcountll(bal & below);
            tot += __builtin_popcountll(bal);
        }
        int mine = 0;
        for (int o = 0; o < P.max_occ; o++)
            if (act && lo + o < P.n_entries && codes[lo + o] == code) {
                const long long g = gpos[lo + o];
                if (g < self_lo || g >= self_hi) {
                    const int slot = nh + pre + mine;
                    mine++;
                    if (slot < P.list) {
                        int b = 0;                                            // the last read of the block with off <= g
                        for (int s = P.read_top; s > 0; s >>= 1)
                            if (b + s < P.n_reads && off[b + s] <= g) b += s;
                        const unsigned long long d = (unsigned long long)(g - off[b] - p + J.alen);
                        keys[slot] = ((unsigned long long)b << (OVL_D_BITS + OVL_P_BITS)) | (d << OVL_P_BITS) | (unsigned long long)p;
                    }
                }
            }
        if (nh + tot > P.list) over = true;
        nh = min(nh + tot, P.list);
    }
    if (nh == 0) { head(OVL_ST_NONE, 0, 0); return; }                        // (nh: the same in every lane)
    // ---- sorted by (b, d, p): a bitonic network over the power of two that holds nh, the rest padded with the largest key ---------
    int N = 64;
    for (int t = 0; t < 7; t++)
        if (N < nh) N <<= 1;                                                  // 64 .. 8192 >= nh (nh <= list <= OVL_LIST_MAX)
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
    // ---- cnt[i]: the first element at or behind (b, d[i] + window), less i; with its element in one word: the larger word is the
    //      pick seed_better() prefers (cnt on top, 65535 - i below) ---------------------------------------------------------------
    for (int i = lane; i < N; i += 64)
        if (i < nh) {
            const unsigned long long bd = keys[i] >> OVL_P_BITS;                                     // b and d
            const unsigned long long next_b = ((bd >> OVL_D_BITS) + 1ull) << OVL_D_BITS;
            const unsigned long long past = bd + (unsigned long long)P.window, target = past < next_b ? past : next_b;
            int lo = 0;
            for (int s = N; s > 0; s >>= 1)
                if (lo + s <= nh && (keys[lo + s - 1] >> OVL_P_BITS) < target) lo += s;
            va[i] = ((unsigned)(lo - i) << 16) | (unsigned)(65535 - i);
        }
    __syncthreads();
    // ---- per b: the segmented scan.  After the step of s, src[i] is the best of elements i .. i + 2 s - 1 of i's own b --------------
    unsigned* src = va;
    unsigned* dst = vb;
    for (int s = 1; s < N; s <<= 1) {
        for (int i = lane; i < N; i += 64)
            if (i < nh) {
                unsigned v = src[i];
                if (i + s < nh && (keys[i + s] >> (OVL_D_BITS + OVL_P_BITS)) == (keys[i] >> (OVL_D_BITS + OVL_P_BITS)) && src[i + s] > v) v = src[i + s];
                dst[i] = v;
            }
        __syncthreads();
        unsigned* const sw = src; src = dst; dst = sw;
    }
    // ---- the candidates: the first element of every b whose pick holds min_hits, ranked in ascending b -----------------------------
    int n_cand = 0;
    for (int ch = 0; ch < (N >> 6); ch++) {
        const int i = (ch << 6) + lane;
        bool is_c = false;
        unsigned v = 0u;
        if (i < nh) {
            const unsigned long long b = keys[i] >> (OVL_D_BITS + OVL_P_BITS);
            v = src[i];
            is_c = (i == 0 || (keys[i - 1] >> (OVL_D_BITS + OVL_P_BITS)) != b) && (int)(v >> 16) >= P.min_hits;
        }
        const unsigned long long bal = seed_ballot(is_c);
        const int rank = n_cand + __builtin_popcountll(bal & below);
        if (is_c && rank < P.max_partners) {
            const int c = (int)(v >> 16), e = 65535 - (int)(v & 0xffffu);
            const unsigned long long rep = keys[e + c / 2];                   // (e + cnt[e] - 1 < nh, of the same b)
            int* o = my_out + OVL_HEAD + 4 * rank;
            o[0] = P.first + (int)(rep >> (OVL_D_BITS + OVL_P_BITS));
            o[1] = c;
            o[2] = (int)((rep >> OVL_P_BITS) & ((1ull << OVL_D_BITS) - 1ull));
            o[3] = (int)(rep & ((1ull << OVL_P_BITS) - 1ull));
        }
        n_cand += __builtin_popcountll(bal);
    }
    const bool trunc = n_cand > P.max_partners;
    head(n_cand == 0 ? OVL_ST_NONE : (over ? OVL_ST_OVERFLOW : 0) | (trunc ? OVL_ST_TRUNCATED : 0), min(n_cand, P.max_partners), nh);
}

}  // namespace hinge
