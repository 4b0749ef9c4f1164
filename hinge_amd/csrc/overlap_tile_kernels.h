// `hinge overlap --tile`: the query of a job cut into half-overlapping tiles.  k_overlap_vote
// (overlap_kernels.h) takes a whole read as one job and widens its sampling step until the read has at most `list` sampled
// positions; here the step is the call's at any read length, and the position is stored relative to its tile, which leaves room for
// a 31-bit d: reads of up to 2^30 - 1 bases.
//
// Tiles     T = the tile, a power of two in 64 .. 8192 with T <= list * step (a tile never has more than `list` sampled positions);
//           adv = T / 2.  The sampled positions of a read are the global ones, p = j * step <= alen - k: a tile does not restart
//           the phase.  Tile t of a (read, strand) job holds the sampled p with t * adv <= p < t * adv + T; ovl_tile_count() tiles.
//           A stretch of at most adv bases lies whole in one tile, a longer one has at least adv of its bases in one tile: min_hits
//           holds per tile without a loss at the seams.
// Per tile  k_overlap_vote's rule: hits (b, d, p) with d = (gpos - off[b]) - p + alen in the whole read's frame, so that tiles are
//           comparable; self hits are counted out before slots are assigned; enumerated by p then gpos and cut at `list`; sorted by
//           (b, d, p); window counts; per b the pick seed_better() prefers; representative i + cnt / 2; a candidate needs
//           cnt >= min_hits; ascending b, the first max_partners.
// Key       b << 44 | d << 13 | (p - t * adv): 20, 31 and 13 bits.  The host checks before any launch (HINGE_E_CAPACITY): every read
//           below 2^30 bases (d < alen + blen < 2^31), at most 2^20 - 1 reads per block (the all-ones key pads the sort), a block
//           below 2^31 bases.
// Tile row  ovl_out_ints(max_partners) ints: status, candidates, hits kept, 1 if hits beyond `list` were dropped (also where the
//           tile has no candidate), then (b, cnt, d, p) per candidate, p in the read's frame.
// Reduce    k_overlap_tile_reduce, per (read, strand) over its tiles' rows: per b the tile candidate of the largest cnt, of equal
//           ones the lowest tile; ascending b, the first max_partners.  NONE without a candidate; else OVERFLOW if any tile dropped
//           hits, TRUNCATED if any tile was or more than max_partners distinct b remain.  hits = the sum of the tiles' kept hits
//           (held at 2^31 - 1).  The row has k_overlap_vote's layout: the host's parse is hinge_overlap_run's.
//
// Loops.  Every trip count is fixed before its loop: as in k_overlap_vote for the tile kernel (the chunks come from the tile's
// sampled positions); in the reduce the chunks of 64 tiles, the six cross-lane steps, the search's log2 steps over a row's
// candidates (part_top) and min(max_partners + 1, the rows' candidates) rounds.  Nothing is read that another wavefront of the
// same launch writes; jobs are assigned by blockIdx; no atomics; the only barrier is that of the one-wavefront workgroup.
// Not claimed: more than one stretch per pair together with tiles; chaining; more than one GPU.
#pragma once
#include "overlap_kernels.h"

namespace hinge {

constexpr int OVT_P_BITS = 13, OVT_D_BITS = 31, OVT_B_BITS = 20;
constexpr int OVT_TILE_MIN = 64, OVT_TILE_MAX = 1 << OVT_P_BITS;
constexpr int OVT_READ_MAX = (1 << 30) - 1;                       // the longest read: d < alen + blen < 2^31
constexpr int OVT_BLOCK_READS_MAX = (1 << OVT_B_BITS) - 1;        // the most reads of a block
static_assert(OVT_TILE_MAX - 1 < (1 << OVT_P_BITS), "a position relative to its tile fits OVT_P_BITS");
static_assert(2ll * OVT_READ_MAX < (1ll << OVT_D_BITS), "d < alen + blen fits OVT_D_BITS");
static_assert(OVT_BLOCK_READS_MAX < (1 << OVT_B_BITS), "a read of the block fits OVT_B_BITS, below the padding key");
static_assert(OVT_P_BITS + OVT_D_BITS + OVT_B_BITS == 64, "the key is 64 bits");

struct OvlTileJob { int a, comp, alen, t; };         // tile t of the job (a, comp)
struct OvlRedJob { int row0, n_tiles; };             // the job's tile rows: row0 .. row0 + n_tiles - 1 of the batch
struct OvlTileParams { int step, tile, adv, part_top; };   // part_top: the largest power of two <= max_partners

__host__ __device__ inline long long ovl_tile_count(int alen, int k, int tile) {
    const long long L = (long long)alen - k + 1, adv = tile / 2;
    if (alen < k || L <= tile) return 1;
    return (L - tile + adv - 1) / adv + 1;
}

// One WAVEFRONT (= one 64-thread workgroup) per (job, tile).  LDS: keys[list], va[list], vb[list], as k_overlap_vote.
__global__ __launch_bounds__(64) void k_overlap_vote_tile(CnsSeqs SB, const OvlTileJob* __restrict__ jobs, int n_jobs, OvlParams P, OvlTileParams TP,
                                                          const unsigned* __restrict__ codes, const int* __restrict__ gpos, const long long* __restrict__ off, int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char ovl_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const OvlTileJob J = jobs[job];
    int* __restrict__ my_out = out + (long long)job * ovl_out_ints(P.max_partners);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ovl_lds);
    unsigned* va = reinterpret_cast<unsigned*>(keys + P.list);
    unsigned* vb = va + P.list;
    auto head = [&](int status, int cands, int hits, bool dropped) {
        if (lane == 0) { my_out[0] = status; my_out[1] = cands; my_out[2] = hits; my_out[3] = dropped ? 1 : 0; }
    };
    if (J.alen < P.k || J.t < 0) { head(OVL_ST_NONE, 0, 0, false); return; }
    CnsPair Q;
    Q.abps = SB.bps; Q.aoff = 0; Q.bbps = SB.bps; Q.boff = SB.boff[J.a]; Q.comp = J.comp; Q.blen = J.alen;
    const int a_loc = J.a - P.first;                                          // the query's place in the block, if it has one
    const bool a_in = a_loc >= 0 && a_loc < P.n_reads;
    const long long self_lo = a_in ? off[a_loc] : 0, self_hi = a_in ? off[a_loc + 1] : 0;
    // ---- the tile's sampled positions: the multiples of step in [t * adv, min(t * adv + T, alen - k + 1)) ----------------------------
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
    if (nh == 0) { head(OVL_ST_NONE, 0, 0, false); return; }                 // (nh: the same in every lane)
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
    // ---- cnt[i]: the first element at or behind (b, d[i] + window), less i; with its element in one word (cnt on top, 65535 - i
    //      below): the larger word is the pick seed_better() prefers ----------------------------------------------------------------
    for (int i = lane; i < N; i += 64)
        if (i < nh) {
            const unsigned long long bd = keys[i] >> OVT_P_BITS;                                     // b and d
            const unsigned long long next_b = ((bd >> OVT_D_BITS) + 1ull) << OVT_D_BITS;
            const unsigned long long past = bd + (unsigned long long)P.window, target = past < next_b ? past : next_b;
            int lo = 0;
            for (int s = N; s > 0; s >>= 1)
                if (lo + s <= nh && (keys[lo + s - 1] >> OVT_P_BITS) < target) lo += s;
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
                if (i + s < nh && (keys[i + s] >> (OVT_D_BITS + OVT_P_BITS)) == (keys[i] >> (OVT_D_BITS + OVT_P_BITS)) && src[i + s] > v) v = src[i + s];
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
            const unsigned long long b = keys[i] >> (OVT_D_BITS + OVT_P_BITS);
            v = src[i];
            is_c = (i == 0 || (keys[i - 1] >> (OVT_D_BITS + OVT_P_BITS)) != b) && (int)(v >> 16) >= P.min_hits;
        }
        const unsigned long long bal = seed_ballot(is_c);
        const int rank = n_cand + __builtin_popcountll(bal & below);
        if (is_c && rank < P.max_partners) {
            const int c = (int)(v >> 16), e = 65535 - (int)(v & 0xffffu);
            const unsigned long long rep = keys[e + c / 2];                   // (e + cnt[e] - 1 < nh, of the same b)
            int* o = my_out + OVL_HEAD + 4 * rank;
            o[0] = P.first + (int)(rep >> (OVT_D_BITS + OVT_P_BITS));
            o[1] = c;
            o[2] = (int)((rep >> OVT_P_BITS) & ((1ull << OVT_D_BITS) - 1ull));
            o[3] = (int)(t0 + (long long)(rep & ((1ull << OVT_P_BITS) - 1ull)));
        }
        n_cand += __builtin_popcountll(bal);
    }
    const bool trunc = n_cand > P.max_partners;
    head(n_cand == 0 ? OVL_ST_NONE : (over ? OVL_ST_OVERFLOW : 0) | (trunc ? OVL_ST_TRUNCATED : 0), min(n_cand, P.max_partners), nh, over);
}

// the smaller of two ints over the wavefront (six cross-lane steps; all 64 lanes are here)
__device__ inline int ovl_wave_min(int v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = seed_lane_xor(v, m);
        if (o < v) v = o;
    }
    return v;
}
__device__ inline int ovl_wave_sum(int v) {
    for (int m = 32; m >= 1; m >>= 1) v += seed_lane_xor(v, m);
    return v;
}

// One WAVEFRONT per (read, strand): its tiles' rows of one k_overlap_vote_tile launch (finished: another launch) reduced to one row
// of k_overlap_vote's layout; top[job] = the largest hits kept of one of its tiles.  A lane takes the tiles lane, lane + 64, ...; a
// round finds the smallest b above the last one written - per row by a search, the rows are in ascending b - and of its tile
// candidates the one of the largest cnt, of equal ones the lowest tile.  A row whose head is not a tile kernel's (the poison) leaves
// the job's output unwritten.
__global__ __launch_bounds__(64) void k_overlap_tile_reduce(const int* __restrict__ rows, const OvlRedJob* __restrict__ jobs, int n_jobs, int max_partners, int part_top,
                                                            int* __restrict__ out, int* __restrict__ top) {
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const OvlRedJob J = jobs[job];
    const int W = ovl_out_ints(max_partners);
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
            if (st < 0 || st > (OVL_ST_OVERFLOW | OVL_ST_TRUNCATED) || nc < 0 || nc > max_partners || nh < 0 || nh > OVL_LIST_MAX || dr < 0 || dr > 1) bad = 1;
            else {
                hits += nh; cands = min(cands + nc, max_partners + 1); most = max(most, nh);
                if (dr) flags |= OVL_ST_OVERFLOW;
                if (st != OVL_ST_NONE && (st & OVL_ST_TRUNCATED)) flags |= OVL_ST_TRUNCATED;
            }
        }
    }
    bad = -ovl_wave_min(-bad);
    if (bad) return;                                                          // (the same in every lane)
    const int over = -ovl_wave_min(-(flags & OVL_ST_OVERFLOW)), trunc_t = -ovl_wave_min(-(flags & OVL_ST_TRUNCATED));
    most = -ovl_wave_min(-most);
    cands = ovl_wave_sum(cands);                                              // (the rounds need min(sum, max_partners + 1): a lane's sum is held there)
    const int hi = ovl_wave_sum((int)(hits >> 20)), lo = ovl_wave_sum((int)(hits & 0xfffff));      // (a lane's sum < 2^44; 64 low parts < 2^26)
    const long long all_hits = ((long long)hi << 20) + lo;
    const int n_rounds = min(cands, max_partners + 1);
    // ---- the rounds --------------------------------------------------------------------------------------------------------------------
    int last_b = -1, n_dist = 0;
    bool live = true;
    for (int r = 0; r < n_rounds; r++) {
        int b_key = 0x7fffffff, b_cnt = 0, b_tile = 0x7fffffff, b_idx = 0;    // this lane's best: the smallest b, the largest cnt, the lowest tile
        for (int ch = 0; ch < n_chunks; ch++) {
            const int t = (ch << 6) + lane;
            if (live && t < J.n_tiles) {
                const int* h = my_rows + (long long)t * W;
                const int nc = h[1];
                int idx = 0;                                                  // the row's candidates with b <= last_b
                for (int s = part_top; s > 0; s >>= 1)
                    if (idx + s <= nc && h[OVL_HEAD + 4 * (idx + s - 1)] <= last_b) idx += s;
                if (idx < nc) {
                    const int b = h[OVL_HEAD + 4 * idx], c = h[OVL_HEAD + 4 * idx + 1];
                    if (b < b_key || (b == b_key && c > b_cnt)) { b_key = b; b_cnt = c; b_tile = t; b_idx = idx; }      // (ascending t: of equal ones the lowest tile stays)
                }
            }
        }
        const int w_b = ovl_wave_min(b_key);
        const int w_c = -ovl_wave_min(b_key == w_b ? -b_cnt : 1);
        const int w_t = ovl_wave_min(b_key == w_b && b_cnt == w_c ? b_tile : 0x7fffffff);
        if (w_b == 0x7fffffff) live = false;                                  // (the same in every lane)
        if (live) {
            if (n_dist < max_partners && b_key == w_b && b_cnt == w_c && b_tile == w_t) {
                const int* pk = my_rows + (long long)b_tile * W + OVL_HEAD + 4 * b_idx;
                int* o = my_out + OVL_HEAD + 4 * n_dist;
                o[0] = pk[0]; o[1] = pk[1]; o[2] = pk[2]; o[3] = pk[3];
            }
            n_dist++;
            last_b = w_b;
        }
    }
    if (lane == 0) {
        my_out[0] = n_dist == 0 ? OVL_ST_NONE : over | ((trunc_t || n_dist > max_partners) ? OVL_ST_TRUNCATED : 0);
        my_out[1] = min(n_dist, max_partners);
        my_out[2] = (int)(all_hits < 0x7fffffffll ? all_hits : 0x7fffffffll);
        my_out[3] = 0;
        top[job] = most;
    }
}

}  // namespace hinge
