// `hinge overlap --max-stretches S`: several candidates per (a, b, strand) by rounds of pick and suppress.
// The job, the hits, the self-hit rule, the cut at `list`, the key, the bitonic sort and cnt[i] are k_overlap_vote's
// (overlap_kernels.h, which stays as it is); what follows them runs S = max_stretches times, 1 .. OVL_STRETCHES_MAX.
//
// The round rule.  Every element starts live.  In round r the pick of partner b is the LIVE element seed_better() prefers - the
// largest cnt, of equal ones the smallest i - found by the segmented max-scan of k_overlap_vote over the packed words, a dead
// element's word being 0 (a live one's is >= 1 << 16).  A pick of cnt >= min_hits is round r's candidate of b, written as
// (b, cnt, d, p) of its representative, element e + cnt[e] / 2 - which may itself be dead and is the representative all the same.
// After the round every element i of b with d[e] - window < d[i] < d[e] + window is dead (e the picked element; both bounds
// exclusive: d[i] == d[e] +- window stays live).  A b without a pick of min_hits in round r has none later: its live set only
// shrinks and cnt does not change.
// cnt is NOT recomputed: a live element's window [d[i], d[i] + window) may count dead elements.  It never counts one that a pick's
// window [d[e], d[e] + window) claimed: a live i has d[i] <= d[e] - window, so its window ends at or before d[e], or
// d[i] >= d[e] + window, so it begins at or behind d[e] + window.  Two candidates of one b therefore never share a counted hit.
// How an element learns its partner's pick: a fixed-trip search for the first element of its b; the scan left b's best word there.
//
// Output per job, ovl_multi_out_ints(max_partners, S) ints: status, candidates written over all rounds, hits kept, 0, the number
// written in each of the S rounds; then S sections of max_partners slots of (b, cnt, d, p): section r holds round r's candidates in
// ascending b, ranked by ballots.  A round with more than max_partners candidates sets TRUNCATED and keeps the first ones;
// OVERFLOW and NONE as in k_overlap_vote.  The host poisons the output before the launch.
// LDS: k_overlap_vote's 16 bytes per slot - the keys and the two value arrays; the packed words are recomputed into va every
// round, so cnt needs no array of its own - and one dead bit per slot behind them: OVL_MULTI_SLOT_BITS = 129 bits per slot,
// 132 096 bytes at list 8192 (of the CU's 163 840).  The dead bits of 64 consecutive elements are one ballot, stored by lane 0 and
// lane 1 as two words: no two lanes write one word, no atomics.
// Loops: those of k_overlap_vote; S rounds; per round and element the window search's and the first-element search's log2 steps.
// The round loop ends early when a round had no candidate: that count is a sum of ballots, the same in every lane, and later
// rounds would have none.  Barriers only inside wavefront-uniform control flow; nothing read that another wavefront writes.
// Not claimed: two stretches on one diagonal (less than `window` apart: one candidate); a weaker stretch inside the band that a
// stronger one's alignment settles in; stretches of fewer than min_hits hits; what overlap_kernels.h does not claim.
#pragma once
#include "overlap_kernels.h"

namespace hinge {

constexpr int OVL_STRETCHES_MAX = 8;
constexpr int OVL_MULTI_SLOT_BITS = 8 * OVL_SLOT_BYTES + 1;
__host__ __device__ inline int ovl_multi_out_ints(int max_partners, int stretches) { return OVL_HEAD + stretches + 4 * stretches * max_partners; }
__host__ __device__ inline size_t ovl_multi_lds_bytes(int list) { return (size_t)list * OVL_SLOT_BYTES + (size_t)list / 8; }
static_assert((long long)OVL_LIST_MAX * OVL_MULTI_SLOT_BITS / 8 == 132096 && (long long)OVL_LIST_MAX * OVL_MULTI_SLOT_BITS / 8 <= OVL_LDS_MAX, "keys, two value arrays and the dead bits fit the CU's LDS at the largest list");
static_assert(OVL_LIST_MIN % 64 == 0, "a chunk of 64 elements is two whole words of dead bits");

// One WAVEFRONT (= one 64-thread workgroup) per job.  LDS: keys[list], va[list], vb[list], dead[list / 32].
__global__ __launch_bounds__(64) void k_overlap_vote_multi(CnsSeqs SB, const OvlJob* __restrict__ jobs, int n_jobs, OvlParams P, int stretches, const unsigned* __restrict__ codes,
                                                           const int* __restrict__ gpos, const long long* __restrict__ off, int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char ovl_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const OvlJob J = jobs[job];
    int* __restrict__ my_out = out + (long long)job * ovl_multi_out_ints(P.max_partners, stretches);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ovl_lds);
    unsigned* va = reinterpret_cast<unsigned*>(keys + P.list);
    unsigned* vb = va + P.list;
    unsigned* dead = vb + P.list;
    auto head = [&](int status, int cands, int hits) {
        if (lane == 0) { my_out[0] = status; my_out[1] = cands; my_out[2] = hits; my_out[3] = 0; }
    };
    auto none = [&]() {
        head(OVL_ST_NONE, 0, 0);
        if (lane < stretches) my_out[OVL_HEAD + lane] = 0;                    // (stretches <= 8 < 64)
    };
    if (J.alen < P.k || J.stride < 1) { none(); return; }
    CnsPair Q;
    Q.abps = SB.bps; Q.aoff = 0; Q.bbps = SB.bps; Q.boff = SB.boff[J.a]; Q.comp = J.comp; Q.blen = J.alen;
    const int a_loc = J.a - P.first;                                          // the query's place in the block, if it has one
    const bool a_in = a_loc >= 0 && a_loc < P.n_reads;
    const long long self_lo = a_in ? off[a_loc] : 0, self_hi = a_in ? off[a_loc + 1] : 0;
    // ---- the hits: as k_overlap_vote ---------------------------------------------------------------------------------------------
    const int n_pos = min((J.alen - P.k) / J.stride + 1, P.list);
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
    if (nh == 0) { none(); return; }                                          // (nh: the same in every lane)
    // ---- sorted by (b, d, p): as k_overlap_vote; the dead bits of the N slots cleared ---------------------------------------------
    int N = 64;
    for (int t = 0; t < 7; t++)
        if (N < nh) N <<= 1;                                                  // 64 .. 8192 >= nh (nh <= list <= OVL_LIST_MAX)
    for (int x = nh + lane; x < N; x += 64) keys[x] = ~0ull;
    for (int x = lane; x < (N >> 5); x += 64) dead[x] = 0u;                   // (N <= list: inside dead[list / 32])
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
    // ---- the rounds ---------------------------------------------------------------------------------------------------------------
    int total = 0;
    bool trunc = false;
    int r = 0;
    for (; r < stretches; r++) {
        // cnt[i] as in k_overlap_vote, packed with its element; a dead element's word is 0
        for (int i = lane; i < N; i += 64)
            if (i < nh) {
                const unsigned long long bd = keys[i] >> OVL_P_BITS;                                 // b and d
                const unsigned long long next_b = ((bd >> OVL_D_BITS) + 1ull) << OVL_D_BITS;
                const unsigned long long past = bd + (unsigned long long)P.window, target = past < next_b ? past : next_b;
                int lo = 0;
                for (int s = N; s > 0; s >>= 1)
                    if (lo + s <= nh && (keys[lo + s - 1] >> OVL_P_BITS) < target) lo += s;
                const bool is_dead = (dead[i >> 5] >> (i & 31)) & 1u;
                va[i] = is_dead ? 0u : ((unsigned)(lo - i) << 16) | (unsigned)(65535 - i);
            }
        __syncthreads();
        // per b: the segmented scan of k_overlap_vote
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
        // round r's candidates: the first element of every b whose pick holds min_hits, ranked in ascending b, into section r
        int* sec = my_out + OVL_HEAD + stretches + 4 * r * P.max_partners;
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
                const unsigned long long rep = keys[e + c / 2];               // (e + cnt[e] - 1 < nh, of the same b)
                int* o = sec + 4 * rank;
                o[0] = P.first + (int)(rep >> (OVL_D_BITS + OVL_P_BITS));
                o[1] = c;
                o[2] = (int)((rep >> OVL_P_BITS) & ((1ull << OVL_D_BITS) - 1ull));
                o[3] = (int)(rep & ((1ull << OVL_P_BITS) - 1ull));
            }
            n_cand += __builtin_popcountll(bal);
        }
        if (n_cand == 0) break;                                               // (a sum of ballots: the same in every lane)
        if (lane == 0) my_out[OVL_HEAD + r] = min(n_cand, P.max_partners);
        total += min(n_cand, P.max_partners);
        if (n_cand > P.max_partners) trunc = true;
        if (r + 1 == stretches) continue;
        // the picks' neighbourhoods die: element i finds the first element of its b (the last f with b[f - 1] < b[i]), where the
        // scan left b's best word.  64 elements' new bits are one ballot: two words, stored by lanes 0 and 1
        for (int ch = 0; ch < (N >> 6); ch++) {
            const int i = (ch << 6) + lane;
            bool dies = false;
            if (i < nh) {
                const unsigned long long b = keys[i] >> (OVL_D_BITS + OVL_P_BITS);
                int f = 0;                                                    // elements whose b is smaller
                for (int s = N; s > 0; s >>= 1)
                    if (f + s <= nh && (keys[f + s - 1] >> (OVL_D_BITS + OVL_P_BITS)) < b) f += s;
                const unsigned v = src[f];
                if ((int)(v >> 16) >= P.min_hits) {
                    const int e = 65535 - (int)(v & 0xffffu);
                    const long long de = (long long)((keys[e] >> OVL_P_BITS) & ((1ull << OVL_D_BITS) - 1ull));
                    const long long di = (long long)((keys[i] >> OVL_P_BITS) & ((1ull << OVL_D_BITS) - 1ull));
                    dies = di > de - P.window && di < de + P.window;
                }
            }
            const unsigned long long bal = seed_ballot(dies);
            if (lane < 2) dead[2 * ch + lane] |= (unsigned)(bal >> (32 * lane));
        }
        __syncthreads();                                                      // before va, which src may be, is written again
    }
    if (lane >= r && lane < stretches) my_out[OVL_HEAD + lane] = 0;            // the rounds that did not run, or had none
    head(total == 0 ? OVL_ST_NONE : (over ? OVL_ST_OVERFLOW : 0) | (trunc ? OVL_ST_TRUNCATED : 0), total, nh);
}

}  // namespace hinge
