// `hinge overlap --tile T --tile-stretches S`: several candidates per (a, b, strand) from query tiles.
// overlap_tile_kernels.h keeps one candidate per partner and overlap_multi_kernels.h takes a whole read as its job; both stay as
// they are.  Here every tile runs the rounds of section 3.13, and the reduce runs them again over the tiles' candidates.
//
// Per tile  k_overlap_vote_tile's job: the same sampled positions, self-hit rule, cut at `list`, key of 20 / 31 / 13 bits and sort by
//           (b, d, p).  On that k_overlap_vote_multi's S rounds: the pick of b is its LIVE element of the largest cnt, of equal ones
//           the smallest i; with cnt >= min_hits it is the round's candidate of b, (b, cnt, d, p) of element e + cnt / 2, dead or
//           not; then every element of b with d[e] - window < d < d[e] + window is dead.  cnt is not recomputed.  max_partners and
//           TRUNCATED hold per round.
// Tile row  ovl_multi_out_ints(max_partners, S) ints: status, candidates of all rounds, hits kept, 1 if hits beyond `list` were
//           dropped (also where the tile has no candidate); the S round counts; S sections of max_partners slots of (b, cnt, d, p),
//           p in the read's frame, each section in ascending b.
// Reduce    k_overlap_tile_reduce_multi, per (read, strand) over all sections of all its tile rows.  Round r's pick of partner b is
//           its LIVE tile candidate of the largest cnt, of equal ones the lowest tile's and within a tile the lowest section's; its
//           (b, cnt, d, p) is round r's candidate of b.  Then every tile candidate of b with |d - d_pick| < window is dead (one
//           exactly `window` away stays live).  S rounds; a b without a live candidate has none later.  Section r of the reduced
//           row holds round r's candidates in ascending b, the first max_partners of them.  NONE without any candidate; else
//           OVERFLOW if some tile dropped hits, TRUNCATED if some tile row was or some round has more than max_partners partners.
//           hits = the sum of the tiles' kept hits (held at 2^31 - 1).  The row has k_overlap_vote_multi's layout: the host's
//           parse is hinge_overlap_run_multi's.  A candidate is live iff it is `window` or more from each of the at most S - 1
//           earlier picks of its b, which a lane holds in registers: no list, any number of tiles.
//
// Loops.  Every trip count is fixed before its loop: the tile kernel's are k_overlap_vote_tile's and k_overlap_vote_multi's (the
// round loop ends early on a sum of ballots).  In the reduce: the chunks of 64 tiles, the S sections, the six cross-lane steps, the
// search's log2 steps over a section (part_top); the outer walk over ascending b has min(the rows' candidates, 2^30) trips and
// ends early on the wave-uniform "no b left"; per b up to S rounds, ended early on the wave-uniform "no live candidate".
// Nothing is read that another wavefront of the same launch writes; jobs are assigned by blockIdx; no atomics; the only barrier is
// that of the one-wavefront workgroup, in wavefront-uniform control flow.
// Not claimed: two stretches less than `window` apart (one candidate); a drifting overlap whose tiles' diagonals spread over
// `window` or more (it takes two of the pair's S slots; the program's duplicate rule drops the second record); chaining; more than
// one GPU.
#pragma once
#include "overlap_multi_kernels.h"
#include "overlap_tile_kernels.h"

namespace hinge {

static_assert((long long)OVL_LIST_MAX * OVL_MULTI_SLOT_BITS / 8 <= 163840, "keys, two value arrays and the dead bits fit the CU's LDS at the largest list");
static_assert(OVL_STRETCHES_MAX <= 64, "a lane per round writes the round counts");

// One WAVEFRONT (= one 64-thread workgroup) per (job, tile).  LDS: keys[list], va[list], vb[list], dead[list / 32].
__global__ __launch_bounds__(64) void k_overlap_vote_tile_multi(CnsSeqs SB, const OvlTileJob* __restrict__ jobs, int n_jobs, OvlParams P, OvlTileParams TP, int stretches,
                                                                const unsigned* __restrict__ codes, const int* __restrict__ gpos, const long long* __restrict__ off,
                                                                int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char ovl_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const OvlTileJob J = jobs[job];
    int* __restrict__ my_out = out + (long long)job * ovl_multi_out_ints(P.max_partners, stretches);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ovl_lds);
    unsigned* va = reinterpret_cast<unsigned*>(keys + P.list);
    unsigned* vb = va + P.list;
    unsigned* dead = vb + P.list;
    auto head = [&](int status, int cands, int hits, bool dropped) {
        if (lane == 0) { my_out[0] = status; my_out[1] = cands; my_out[2] = hits; my_out[3] = dropped ? 1 : 0; }
    };
    auto none = [&]() {
        head(OVL_ST_NONE, 0, 0, false);
        if (lane < stretches) my_out[OVL_HEAD + lane] = 0;                    // (stretches <= 8 < 64)
    };
    if (J.alen < P.k || J.t < 0) { none(); return; }
    CnsPair Q;
    Q.abps = SB.bps; Q.aoff = 0; Q.bbps = SB.bps; Q.boff = SB.boff[J.a]; Q.comp = J.comp; Q.blen = J.alen;
    const int a_loc = J.a - P.first;                                          // the query's place in the block, if it has one
    const bool a_in = a_loc >= 0 && a_loc < P.n_reads;
    const long long self_lo = a_in ? off[a_loc] : 0, self_hi = a_in ? off[a_loc + 1] : 0;
    // ---- the tile's sampled positions and hits: as k_overlap_vote_tile ----------------------------------------------------------------
    const long long t0 = (long long)J.t * TP.adv;
    const long long p_end = t0 + TP.tile < (long long)J.alen - P.k + 1 ? t0 + TP.tile : (long long)J.alen - P.k + 1;
    const long long p0 = (t0 + TP.step - 1) / TP.step * TP.step;              // the first sampled position of the tile
    const int n_pos = p0 < p_end ? (int)min((p_end - 1 - p0) / TP.step + 1, (long long)P.list) : 0;     // (T <= list * step: never more than list)
    const int n_chunks = (n_pos + 63) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int nh = 0;
    bool over = false;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int x = (ch << 6) + lane;
        const bool act = x < n_pos;
        const int p = (int)(p0 + (long long)x * TP.step);                     // (act: p < p_end <= alen - k + 1)
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
                        keys[slot] = ((unsigned long long)b << (OVT_D_BITS + OVT_P_BITS)) | (d << OVT_P_BITS) | (unsigned long long)(p - t0);
                    }
                }
            }
        if (nh + tot > P.list) over = true;
        nh = min(nh + tot, P.list);
    }
    if (nh == 0) { none(); return; }                                          // (nh: the same in every lane)
    // ---- sorted by (b, d, p): the bitonic network of k_overlap_vote_tile; the dead bits of the N slots cleared -------------------------
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
    // ---- the rounds: as k_overlap_vote_multi, on the tile's key ------------------------------------------------------------------------
    int total = 0;
    bool trunc = false;
    int r = 0;
    for (; r < stretches; r++) {
        // cnt[i] packed with its element (cnt on top, 65535 - i below); a dead element's word is 0
        for (int i = lane; i < N; i += 64)
            if (i < nh) {
                const unsigned long long bd = keys[i] >> OVT_P_BITS;                                 // b and d
                const unsigned long long next_b = ((bd >> OVT_D_BITS) + 1ull) << OVT_D_BITS;
                const unsigned long long past = bd + (unsigned long long)P.window, target = past < next_b ? past : next_b;
                int lo = 0;
                for (int s = N; s > 0; s >>= 1)
                    if (lo + s <= nh && (keys[lo + s - 1] >> OVT_P_BITS) < target) lo += s;
                const bool is_dead = (dead[i >> 5] >> (i & 31)) & 1u;
                va[i] = is_dead ? 0u : ((unsigned)(lo - i) << 16) | (unsigned)(65535 - i);
            }
        __syncthreads();
        // per b: the segmented scan.  After the step of s, src[i] is the best of elements i .. i + 2 s - 1 of i's own b
        unsigned* src = va;
        unsigned* dst = vb;
        for (int s = 1; s < N; s <<= 1) {
            for (int i = lane; i < N; i += 64)
                if (i < nh) {
                    unsigned v = src[i];
                    if (i + s < nh && (keys[i + s] >> (OVT_D_BITS + OVT_P_BITS)) == (keys[i] >> (OVT_D_BITS + OVT_P_BITS)) && src[i + s] > v) v = src[i + s];
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
                const unsigned long long b = keys[i] >> (OVT_D_BITS + OVT_P_BITS);
                v = src[i];
                is_c = (i == 0 || (keys[i - 1] >> (OVT_D_BITS + OVT_P_BITS)) != b) && (int)(v >> 16) >= P.min_hits;
            }
            const unsigned long long bal = seed_ballot(is_c);
            const int rank = n_cand + __builtin_popcountll(bal & below);
            if (is_c && rank < P.max_partners) {
                const int c = (int)(v >> 16), e = 65535 - (int)(v & 0xffffu);
                const unsigned long long rep = keys[e + c / 2];               // (e + cnt[e] - 1 < nh, of the same b)
                int* o = sec + 4 * rank;
                o[0] = P.first + (int)(rep >> (OVT_D_BITS + OVT_P_BITS));
                o[1] = c;
                o[2] = (int)((rep >> OVT_P_BITS) & ((1ull << OVT_D_BITS) - 1ull));
                o[3] = (int)(t0 + (long long)(rep & ((1ull << OVT_P_BITS) - 1ull)));
            }
            n_cand += __builtin_popcountll(bal);
        }
        if (n_cand == 0) break;                                               // (a sum of ballots: the same in every lane)
        if (lane == 0) my_out[OVL_HEAD + r] = min(n_cand, P.max_partners);
        total += min(n_cand, P.max_partners);
        if (n_cand > P.max_partners) trunc = true;
        if (r + 1 == stretches) continue;
        // the picks' neighbourhoods die: element i finds the first element of its b, where the scan left b's best word.  64
        // elements' new bits are one ballot: two words, stored by lanes 0 and 1
        for (int ch = 0; ch < (N >> 6); ch++) {
            const int i = (ch << 6) + lane;
            bool dies = false;
            if (i < nh) {
                const unsigned long long b = keys[i] >> (OVT_D_BITS + OVT_P_BITS);
                int f = 0;                                                    // elements whose b is smaller
                for (int s = N; s > 0; s >>= 1)
                    if (f + s <= nh && (keys[f + s - 1] >> (OVT_D_BITS + OVT_P_BITS)) < b) f += s;
                const unsigned v = src[f];
                if ((int)(v >> 16) >= P.min_hits) {
                    const int e = 65535 - (int)(v & 0xffffu);
                    const long long de = (long long)((keys[e] >> OVT_P_BITS) & ((1ull << OVT_D_BITS) - 1ull));
                    const long long di = (long long)((keys[i] >> OVT_P_BITS) & ((1ull << OVT_D_BITS) - 1ull));
                    dies = di > de - P.window && di < de + P.window;
                }
            }
            const unsigned long long bal = seed_ballot(dies);
            if (lane < 2) dead[2 * ch + lane] |= (unsigned)(bal >> (32 * lane));
        }
        __syncthreads();                                                      // before va, which src may be, is written again
    }
    if (lane >= r && lane < stretches) my_out[OVL_HEAD + lane] = 0;            // the rounds that did not run, or had none
    head(total == 0 ? OVL_ST_NONE : (over ? OVL_ST_OVERFLOW : 0) | (trunc ? OVL_ST_TRUNCATED : 0), total, nh, over);
}

// One WAVEFRONT per (read, strand): its tiles' rows of one k_overlap_vote_tile_multi launch (finished: another launch) reduced to one
// row of k_overlap_vote_multi's layout; top[job] = the largest hits kept of one of its tiles.  A lane takes the tiles lane,
// lane + 64, ...  The outer walk finds the smallest b above the last one - per section by a search, the sections are in ascending
// b - and runs up to S rounds on it; pd[] holds the d of b's earlier picks.  A row whose head is not a tile kernel's (the poison)
// leaves the job's output unwritten.  No LDS.
__global__ __launch_bounds__(64) void k_overlap_tile_reduce_multi(const int* __restrict__ rows, const OvlRedJob* __restrict__ jobs, int n_jobs, int max_partners, int part_top,
                                                                  int stretches, int window, int* __restrict__ out, int* __restrict__ top) {
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const OvlRedJob J = jobs[job];
    const int W = ovl_multi_out_ints(max_partners, stretches), body = OVL_HEAD + stretches;
    const int* __restrict__ my_rows = rows + (long long)J.row0 * W;
    int* __restrict__ my_out = out + (long long)job * W;
    const int n_chunks = (J.n_tiles + 63) >> 6;
    // ---- the heads: hits, candidates, flags --------------------------------------------------------------------------------------------
    long long hits = 0;
    int cands = 0, flags = 0, bad = 0, most = 0;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int t = (ch << 6) + lane;
        if (t < J.n_tiles) {
            const int* h = my_rows + (long long)t * W;
            const int st = h[0], nc = h[1], nh = h[2], dr = h[3];
            int sum = 0;
            bool rounds_ok = true;
            for (int r = 0; r < stretches; r++) {
                const int c = h[OVL_HEAD + r];
                if (c < 0 || c > max_partners) rounds_ok = false;
                else sum += c;
            }
            if (st < 0 || st > (OVL_ST_OVERFLOW | OVL_ST_TRUNCATED) || !rounds_ok || nc != sum || nh < 0 || nh > OVL_LIST_MAX || dr < 0 || dr > 1) bad = 1;
            else {
                hits += nh; cands = min(cands + nc, 1 << 24); most = max(most, nh);      // (a block has fewer than 2^20 reads: no more distinct b)
                if (dr) flags |= OVL_ST_OVERFLOW;
                if (st != OVL_ST_NONE && (st & OVL_ST_TRUNCATED)) flags |= OVL_ST_TRUNCATED;
            }
        }
    }
    bad = -ovl_wave_min(-bad);
    if (bad) return;                                                          // (the same in every lane)
    const int over = -ovl_wave_min(-(flags & OVL_ST_OVERFLOW)), trunc_t = -ovl_wave_min(-(flags & OVL_ST_TRUNCATED));
    most = -ovl_wave_min(-most);
    const int n_walk = ovl_wave_sum(cands);                                   // (64 lanes of at most 2^24: at most 2^30)
    const int hi = ovl_wave_sum((int)(hits >> 20)), lo = ovl_wave_sum((int)(hits & 0xfffff));      // (a lane's sum < 2^44; 64 low parts < 2^26)
    const long long all_hits = ((long long)hi << 20) + lo;
    // ---- the walk over ascending b ---------------------------------------------------------------------------------------------------------
    int nr[OVL_STRETCHES_MAX], pd[OVL_STRETCHES_MAX];                         // candidates of every round; the d of this b's picks (both indexed by unrolled loops only)
#pragma unroll
    for (int q = 0; q < OVL_STRETCHES_MAX; q++) { nr[q] = 0; pd[q] = 0; }
    int last_b = -1;
    for (int w = 0; w < n_walk; w++) {
        int b_next = 0x7fffffff;                                              // this lane's smallest b above last_b
        for (int ch = 0; ch < n_chunks; ch++) {
            const int t = (ch << 6) + lane;
            if (t < J.n_tiles) {
                const int* h = my_rows + (long long)t * W;
                for (int s = 0; s < stretches; s++) {
                    const int nc = h[OVL_HEAD + s];
                    const int* sec = h + body + 4 * s * max_partners;
                    int idx = 0;                                              // the section's candidates with b <= last_b
                    for (int z = part_top; z > 0; z >>= 1)
                        if (idx + z <= nc && sec[4 * (idx + z - 1)] <= last_b) idx += z;
                    if (idx < nc && sec[4 * idx] < b_next) b_next = sec[4 * idx];
                }
            }
        }
        const int w_b = ovl_wave_min(b_next);
        if (w_b == 0x7fffffff) break;                                         // (the same in every lane)
        for (int r = 0; r < stretches; r++) {
            int b_cnt = 0, b_tile = 0x7fffffff, b_d = 0;                      // this lane's best live candidate of w_b: the largest cnt, the lowest tile, the lowest section
            const int* b_pk = my_rows;
            for (int ch = 0; ch < n_chunks; ch++) {
                const int t = (ch << 6) + lane;
                if (t < J.n_tiles) {
                    const int* h = my_rows + (long long)t * W;
                    for (int s = 0; s < stretches; s++) {
                        const int nc = h[OVL_HEAD + s];
                        const int* sec = h + body + 4 * s * max_partners;
                        int idx = 0;                                          // the section's candidates with b < w_b
                        for (int z = part_top; z > 0; z >>= 1)
                            if (idx + z <= nc && sec[4 * (idx + z - 1)] < w_b) idx += z;
                        if (idx < nc && sec[4 * idx] == w_b) {
                            const int c = sec[4 * idx + 1], d = sec[4 * idx + 2];
                            bool live = true;
#pragma unroll
                            for (int q = 0; q < OVL_STRETCHES_MAX - 1; q++)
                                if (q < r && d > pd[q] - window && d < pd[q] + window) live = false;
                            if (live && c > b_cnt) { b_cnt = c; b_tile = t; b_d = d; b_pk = sec + 4 * idx; }      // (ascending t, then s: of equal ones the first stays)
                        }
                    }
                }
            }
            const int w_c = -ovl_wave_min(-b_cnt);
            if (w_c == 0) break;                                              // no live candidate (a candidate's cnt >= min_hits >= 1); the same in every lane
            const int w_t = ovl_wave_min(b_cnt == w_c ? b_tile : 0x7fffffff);
            const bool mine = b_cnt == w_c && b_tile == w_t;                  // one lane: a tile is one lane's
            const int w_d = ovl_wave_min(mine ? b_d : 0x7fffffff);
            int n_r = 0;
#pragma unroll
            for (int q = 0; q < OVL_STRETCHES_MAX; q++)
                if (q == r) { n_r = nr[q]; nr[q] = min(nr[q] + 1, max_partners + 1); pd[q] = w_d; }
            if (mine && n_r < max_partners) {
                int* o = my_out + body + 4 * (r * max_partners + n_r);
                o[0] = b_pk[0]; o[1] = b_pk[1]; o[2] = b_pk[2]; o[3] = b_pk[3];
            }
        }
        last_b = w_b;
    }
    int total = 0;
    bool trunc = trunc_t != 0;
#pragma unroll
    for (int q = 0; q < OVL_STRETCHES_MAX; q++) {
        if (nr[q] > max_partners) trunc = true;
        total += min(nr[q], max_partners);
        if (lane == 0 && q < stretches) my_out[OVL_HEAD + q] = min(nr[q], max_partners);
    }
    if (lane == 0) {
        my_out[0] = total == 0 ? OVL_ST_NONE : over | (trunc ? OVL_ST_TRUNCATED : 0);
        my_out[1] = total;
        my_out[2] = (int)(all_hits < 0x7fffffffll ? all_hits : 0x7fffffffll);
        my_out[3] = 0;
        top[job] = most;
    }
}

}  // namespace hinge
