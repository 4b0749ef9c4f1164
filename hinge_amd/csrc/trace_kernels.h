// `hinge paf2las` on the GPU: DALIGNER-form trace points for placements whose end points are given.
// Stands in for the trace output of DALIGNER's Local_Alignment as LAInterface::recoverAlignment consumes it
// (lib/LAInterface.cpp:4125-4244; the record: include/align.h:98-110) - NOT for its seeding or its local extension.
//
// One placement = A = contig[ab, ae), B = read[bb, be) in the strand frame of hinge_cns_alignment, half-width W.
//   k_trace_fill   one WAVEFRONT (= one 64-thread workgroup) per placement: banded global edit distance in anti-diagonal order,
//                  the two previous anti-diagonals in LDS rings, one 2-bit direction per cell to device scratch
//   k_trace_walk   one LANE per placement: the path back from the end cell, (edit operations, B bases) per tspace block of A
//   k_trace_clip   in the walk's place when the end points are approximate (hinge_trace_refine): the best-scoring stretch of the path
//   k_trace_fill_local, k_trace_walk_local   in the place of both when the diagonal is approximate too (hinge_trace_local): the
//                  best local alignment inside the band - see the comment in front of them
//
// The band.  Cell (i, j) = i bases of A and j bases of B consumed, 0 <= i <= alen, 0 <= j <= blen.  Row i's centre diagonal is
//   c(i) = floor((2 i (blen - alen) + alen) / (2 alen))            [= round(i (blen - alen) / alen), halves up]
// and the cell is inside the band when k = j - i - c(i) + W lies in [0, 2 W): 2 W diagonals around the straight line from
// (0, 0) to (alen, blen).  Cells outside are +infinity.  trace_centre() below is that formula; the kernels step it from row to
// row without a division (TraceStep: quotient and remainder of the numerator's increment).
// Tie order of a cell: diagonal, then the gap in B (an A base against nothing: from (i - 1, j)), then the gap in A (from (i, j - 1)).
//
// Loops.  Every loop's trip count is fixed before it starts from the job's four coordinates, W and the ring size: the fill's
// alen + blen + 1 anti-diagonals with their chunks of 64 cells, the walk's at most alen + blen + 1 steps.  Nothing waits on memory
// another wavefront writes; jobs are assigned by blockIdx (fill) and by global lane (walk); the workgroup barrier of the fill
// is that of a one-wavefront workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "consensus_kernels.h"

namespace hinge {

constexpr int TRACE_ST_OK = 0;        // a path, nowhere on the band's first or last diagonal
constexpr int TRACE_ST_TOUCHED = 1;   // the path used a cell on the first or the last diagonal: optimal only for this band
constexpr int TRACE_ST_NO_PATH = 2;   // |blen - alen| > W, or the end cell was not reached inside the band
constexpr int TRACE_ST_WIDE = 3;      // a segment's diffs or B advance exceeds what a trace value holds
constexpr int TRACE_ST_STEPS = 4;     // the walk did not arrive at (0, 0) in alen + blen + 1 steps, or its diffs are not the fill's cost
constexpr int TRACE_ST_EMPTY = 5;     // k_trace_clip: no run of the path's columns sums to max(1, min_score); k_trace_walk_local: no cell of the band scores it
constexpr int TRACE_ST_POISON = -1;  // what the status slots hold before a launch
constexpr unsigned short TRACE_POISON16 = 0xffffu;   // ... and the trace slots
constexpr int TRACE_INF = 0x3fffffff;
constexpr int TRACE_BAND_MIN = 8, TRACE_BAND_LIMIT = 2048;   // W: a multiple of 8 in this range (16 cells per direction word; the LDS rings)

struct TraceJob {
    int a, b, comp;
    int ab, ae, bb, be;            // as hinge_cns_alignment: B in the complemented frame when comp
    int blen;                      // the whole read's length (the complemented frame's mirror)
    int nseg, pad;
    long long dir_off;             // first 32-bit word of its directions in the batch's scratch
    long long trace_off;           // first 16-bit value of its trace in the batch's trace buffer
};

__host__ __device__ inline long long trace_floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    if ((a % b) != 0 && a < 0) q--;
    return q;
}
// c(i) of the header comment
__host__ __device__ inline int trace_centre(int i, int alen, int blen) {
    return (int)trace_floor_div(2ll * i * ((long long)blen - alen) + alen, 2ll * alen);
}
// trace points of A[ab, ae): the first ends at the next multiple of tspace, the last at ae (align.h:98-110)
__host__ __device__ inline int trace_segments(int ab, int ae, int tspace) { return (ae - 1) / tspace - ab / tspace + 1; }
// 32-bit direction words of one row / of one job
__host__ __device__ inline int trace_row_words(int W) { return W / 8; }
__host__ __device__ inline long long trace_dir_words(int alen, int W) { return (long long)alen * trace_row_words(W); }
// entries of an LDS ring: a power of two that holds an anti-diagonal's cells (at most 2 W) and one margin cell on either side
__host__ __device__ inline int trace_ring(int W) {
    int n = 64;
    while (n < 2 * W + 2) n <<= 1;
    return n;
}
__host__ __device__ inline size_t trace_lds_bytes(int W) { return (size_t)trace_ring(W) * (4 * sizeof(int) + sizeof(short)); }

// c(i + 1) - c(i) without a division: 2 i d + alen = c(i) den + r(i), 0 <= r < den; one row on adds 2 d = q den + m.
struct TraceStep {
    long long den, m;
    int q;
    __device__ __forceinline__ void init(int alen, int blen) {
        den = 2ll * alen;
        const long long d2 = 2ll * ((long long)blen - alen);
        q = (int)trace_floor_div(d2, den);
        m = d2 - (long long)q * den;
    }
    __device__ __forceinline__ void fwd(int& c, long long& r) const { c += q; r += m; if (r >= den) { r -= den; c++; } }
    __device__ __forceinline__ void back(int& c, long long& r) const { c -= q; r -= m; if (r < 0) { r += den; c--; } }
};

// Direction codes (2 bits): 0 diagonal on equal bases, 1 gap in B, 2 gap in A, 3 diagonal on different bases (the walk counts
// its diffs without fetching bases again).
__global__ __launch_bounds__(64) void k_trace_fill(CnsSeqs SA, CnsSeqs SB, const TraceJob* __restrict__ jobs, int n_jobs, int W, unsigned* __restrict__ dirs,
                                                   int* __restrict__ end_cost) {
    extern __shared__ __align__(16) unsigned char trace_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const TraceJob J = jobs[job];
    const int alen = J.ae - J.ab, blen = J.be - J.bb;
    if (alen <= 0 || blen <= 0 || abs(blen - alen) > W) {       // (the host never sends these; the walk reports NO_PATH)
        if (lane == 0) end_cost[job] = TRACE_INF;
        return;
    }
    const int N = trace_ring(W), mask = N - 1;
    int* cur = reinterpret_cast<int*>(trace_lds);
    int* p1 = cur + N;                                           // anti-diagonal t - 1
    int* p2 = p1 + N;                                            // anti-diagonal t - 2
    unsigned* acc = reinterpret_cast<unsigned*>(p2 + N);         // per row: the direction word being filled
    short* cr = reinterpret_cast<short*>(acc + N);               // per row inside the band: c(i) (|c| <= W)
    for (int x = lane; x < N; x += 64) { cur[x] = TRACE_INF; p1[x] = TRACE_INF; p2[x] = TRACE_INF; acc[x] = 0u; cr[x] = 0; }
    __syncthreads();
    CnsPair P;
    P.abps = SA.bps; P.aoff = SA.boff[J.a]; P.bbps = SB.bps; P.boff = SB.boff[J.b]; P.comp = J.comp; P.blen = J.blen;
    TraceStep S;
    S.init(alen, blen);
    // the band's rows on anti-diagonal t: f(i) = 2 i + c(i) is strictly increasing, the cells are those with t - W + 1 <= f(i) <= t + W
    int lo_i = 0, lo_c = 0, hi_i = 0, hi_c = 0;
    long long lo_r = alen, hi_r = alen;
    for (int s = 0; s <= W; s++) {                               // rows of anti-diagonal 0: f grows by at least one per row, so at most W more
        if (hi_i >= alen) break;
        int c = hi_c; long long r = hi_r;
        S.fwd(c, r);
        if (2 * (hi_i + 1) + c > W) break;
        hi_i++; hi_c = c; hi_r = r;
        if (lane == 0) cr[hi_i & mask] = (short)c;
    }
    __syncthreads();
    const int wpr = trace_row_words(W);
    unsigned* __restrict__ my_dirs = dirs + J.dir_off;
    const int T = alen + blen;
    for (int t = 0; t <= T; t++) {
        const int lo_e = max(max(lo_i, t - blen), 0), hi_e = min(hi_i, t);
        const int first = lo_e - 1, count = hi_e - lo_e + 3;     // one margin cell on either side is written as +infinity
        const int n_chunks = count > 0 ? (count + 63) >> 6 : 0;
        for (int ch = 0; ch < n_chunks; ch++) {
            const int i = first + (ch << 6) + lane;
            if (i <= hi_e + 1) {
                int val = TRACE_INF;
                if (i >= lo_e && i <= hi_e) {
                    const int j = t - i;
                    unsigned dir = 0u;
                    if (i == 0 && j == 0) val = 0;
                    else {
                        int best = TRACE_INF;
                        if (i >= 1 && j >= 1) {
                            const int ne = P.A(J.ab + i - 1) != P.B(J.bb + j - 1);
                            best = p2[(i - 1) & mask] + ne;
                            dir = ne ? 3u : 0u;
                        }
                        if (i >= 1) { const int g = p1[(i - 1) & mask] + 1; if (g < best) { best = g; dir = 1u; } }
                        if (j >= 1) { const int g = p1[i & mask] + 1; if (g < best) { best = g; dir = 2u; } }
                        val = min(best, TRACE_INF);
                    }
                    if (i >= 1) {
                        const int k = t - (2 * i + (int)cr[i & mask]) + W;
                        if ((unsigned)k < (unsigned)(2 * W)) {
                            unsigned a = acc[i & mask] | (dir << (2 * (k & 15)));
                            if ((k & 15) == 15 || j == blen) { my_dirs[(long long)(i - 1) * wpr + (k >> 4)] = a; a = 0u; }   // the word is complete / the row ends
                            acc[i & mask] = a;
                        }
                    }
                    if (i == alen && j == blen) end_cost[job] = val;
                }
                cur[i & mask] = val;
            }
        }
        // the band's rows on anti-diagonal t + 1: each bound moves by at most one row
        if (lo_i < alen && 2 * lo_i + lo_c < t + 2 - W) { lo_i++; S.fwd(lo_c, lo_r); }
        if (hi_i < alen) {
            int c = hi_c; long long r = hi_r;
            S.fwd(c, r);
            if (2 * (hi_i + 1) + c <= t + 1 + W) {
                hi_i++; hi_c = c; hi_r = r;
                if (lane == 0) cr[hi_i & mask] = (short)c;
            }
        }
        int* const tmp = p2; p2 = p1; p1 = cur; cur = tmp;
        __syncthreads();                                          // (one wavefront: orders this anti-diagonal's LDS writes before the next one's reads)
    }
}

// tmax: the largest value a trace entry holds (255 at tspace <= 125, else 65534: 65535 is the poison).
__global__ __launch_bounds__(64) void k_trace_walk(const TraceJob* __restrict__ jobs, int n_jobs, int W, int tspace, int tmax, const unsigned* __restrict__ dirs,
                                                   const int* __restrict__ end_cost, unsigned short* __restrict__ trace, int* __restrict__ diffs, int* __restrict__ status) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= n_jobs) return;
    const TraceJob J = jobs[x];
    const int alen = J.ae - J.ab, blen = J.be - J.bb;
    const int cost = end_cost[x];
    if (alen <= 0 || blen <= 0 || abs(blen - alen) > W || cost >= TRACE_INF || cost < 0) {
        diffs[x] = 0;
        status[x] = TRACE_ST_NO_PATH;
        return;
    }
    TraceStep S;
    S.init(alen, blen);
    const int wpr = trace_row_words(W);
    const unsigned* __restrict__ my_dirs = dirs + J.dir_off;
    unsigned short* __restrict__ my_trace = trace + J.trace_off;
    const int seg_base = J.ab / tspace;
    int i = alen, j = blen, c = blen - alen;
    long long r = alen;
    int seg = J.nseg - 1, sd = 0, sb = 0, total = 0;
    bool touched = false, wide = false, bad = false;
    auto emit = [&]() {
        if (seg >= 0 && seg < J.nseg) {
            my_trace[2 * seg] = (unsigned short)min(sd, tmax);
            my_trace[2 * seg + 1] = (unsigned short)min(sb, tmax);
        } else bad = true;
        if (sd > tmax || sb > tmax) wide = true;
        total += sd;
    };
    const int max_steps = alen + blen + 1;
    for (int step = 0; step < max_steps; step++) {
        if (i == 0 && j == 0) break;
        const int k = j - i - c + W;
        if (k == 0 || k == 2 * W - 1) touched = true;
        unsigned dir = 2u;
        if (i > 0) {
            if ((unsigned)k >= (unsigned)(2 * W)) { bad = true; break; }
            dir = (my_dirs[(long long)(i - 1) * wpr + (k >> 4)] >> (2 * (k & 15))) & 3u;
        }
        if ((dir == 2u && j == 0) || ((dir == 0u || dir == 3u) && j == 0)) { bad = true; break; }
        const int s = i > 0 ? (J.ab + i - 1) / tspace - seg_base : 0;   // a B-only step belongs to the segment of the A base in front of it
        if (s != seg) { emit(); seg = s; sd = 0; sb = 0; }
        if (dir == 0u) { i--; j--; sb++; S.back(c, r); }
        else if (dir == 3u) { i--; j--; sb++; sd++; S.back(c, r); }
        else if (dir == 1u) { i--; sd++; S.back(c, r); }
        else { j--; sb++; sd++; }
    }
    emit();
    if (i != 0 || j != 0 || seg != 0 || total != cost) bad = true;
    diffs[x] = total;
    status[x] = bad ? TRACE_ST_STEPS : touched ? TRACE_ST_TOUCHED : wide ? TRACE_ST_WIDE : TRACE_ST_OK;
}

// Refined end points (hinge_trace_refine): the walk's place when the job's box is the given one widened.  One LANE per placement.
// The path from (alen, blen) back to (0, 0) is a list of columns, one per step; a column lies on the cell it ends in (where its
// direction is stored) and scores +match on direction 0, -diff on 1, 2 and 3.  Kept: the contiguous run of columns with the
// largest sum; among equal sums the run that starts latest, among those the one that ends latest.
//   walk 1   q = the sum of the columns behind the cell the walk stands on, qmin = the smallest q so far with its cell (replaced
//            on q < qmin: of equal minima the first met, i.e. the latest end), best = the largest q - qmin with both cells
//            (replaced on >: of equal sums the first met, i.e. the latest start).  The run begins and ends with a match column:
//            a -diff column at either end would leave a larger sum without it.
//   walk 2   from the kept end cell (its c and r were saved with it) to the kept start cell: k_trace_walk's body; the segment
//            slots are those of the job's (widened) layout, so the kept segments are slots first .. first + n - 1 of it.
// touched: only cells of kept columns count.  clip[4 x ..] = i0, j0, i1, j1 (cells of the job's box), score[x] = the sum.
// Both loops: at most alen + blen + 1 trips, fixed before they start; nothing read that another wavefront writes.
__global__ __launch_bounds__(64) void k_trace_clip(const TraceJob* __restrict__ jobs, int n_jobs, int W, int tspace, int tmax, int match, int diff, int min_score,
                                                   const unsigned* __restrict__ dirs, const int* __restrict__ end_cost, unsigned short* __restrict__ trace, int* __restrict__ diffs,
                                                   int* __restrict__ status, int* __restrict__ clip, int* __restrict__ score) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= n_jobs) return;
    const TraceJob J = jobs[x];
    const int alen = J.ae - J.ab, blen = J.be - J.bb;
    const int cost = end_cost[x];
    int i0 = 0, j0 = 0, i1 = 0, j1 = 0, best = 0;
    auto done = [&](int code, int d) {
        clip[4ll * x] = i0; clip[4ll * x + 1] = j0; clip[4ll * x + 2] = i1; clip[4ll * x + 3] = j1;
        score[x] = best;
        diffs[x] = d;
        status[x] = code;
    };
    if (alen <= 0 || blen <= 0 || abs(blen - alen) > W || cost >= TRACE_INF || cost < 0) { done(TRACE_ST_NO_PATH, 0); return; }
    TraceStep S;
    S.init(alen, blen);
    const int wpr = trace_row_words(W);
    const unsigned* __restrict__ my_dirs = dirs + J.dir_off;
    const int max_steps = alen + blen + 1;
    bool bad = false;
    // ---- walk 1: the kept run ----------------------------------------------------------------------------------------------------
    int i = alen, j = blen, c = blen - alen;
    long long r = alen;
    int q = 0, qmin = 0, mi = alen, mj = blen, mc = c, c1 = c, total = 0;
    long long mr = r, r1 = r;
    for (int step = 0; step < max_steps; step++) {
        if (i == 0 && j == 0) break;
        const int k = j - i - c + W;
        unsigned dir = 2u;
        if (i > 0) {
            if ((unsigned)k >= (unsigned)(2 * W)) { bad = true; break; }
            dir = (my_dirs[(long long)(i - 1) * wpr + (k >> 4)] >> (2 * (k & 15))) & 3u;
        }
        if (dir != 1u && j == 0) { bad = true; break; }
        if (dir == 0u) { i--; j--; q += match; S.back(c, r); }
        else if (dir == 3u) { i--; j--; q -= diff; total++; S.back(c, r); }
        else if (dir == 1u) { i--; q -= diff; total++; S.back(c, r); }
        else { j--; q -= diff; total++; }
        if (q - qmin > best) { best = q - qmin; i0 = i; j0 = j; i1 = mi; j1 = mj; c1 = mc; r1 = mr; }
        if (q < qmin) { qmin = q; mi = i; mj = j; mc = c; mr = r; }
    }
    if (i != 0 || j != 0 || total != cost) bad = true;
    if (bad) { done(TRACE_ST_STEPS, 0); return; }
    if (best < max(1, min_score)) { done(TRACE_ST_EMPTY, 0); return; }
    // ---- walk 2: the kept run's segments -----------------------------------------------------------------------------------------
    unsigned short* __restrict__ my_trace = trace + J.trace_off;
    const int seg_base = J.ab / tspace;
    const int seg_first = (J.ab + i0) / tspace - seg_base;
    i = i1; j = j1; c = c1; r = r1;
    int seg = (J.ab + i1 - 1) / tspace - seg_base, sd = 0, sb = 0, kept = 0, cols = 0;
    bool touched = false, wide = false;
    auto emit = [&]() {
        if (seg >= seg_first && seg < J.nseg) {
            my_trace[2 * seg] = (unsigned short)min(sd, tmax);
            my_trace[2 * seg + 1] = (unsigned short)min(sb, tmax);
        } else bad = true;
        if (sd > tmax || sb > tmax) wide = true;
        kept += sd;
    };
    for (int step = 0; step < max_steps; step++) {
        if (i == i0 && j == j0) break;
        if (i <= i0 || j < j0) { bad = true; break; }               // (every kept column has an A base in front of it)
        const int k = j - i - c + W;
        if ((unsigned)k >= (unsigned)(2 * W)) { bad = true; break; }
        if (k == 0 || k == 2 * W - 1) touched = true;
        const unsigned dir = (my_dirs[(long long)(i - 1) * wpr + (k >> 4)] >> (2 * (k & 15))) & 3u;
        const int s = (J.ab + i - 1) / tspace - seg_base;
        if (s != seg) { emit(); seg = s; sd = 0; sb = 0; }
        cols++;
        if (dir == 0u) { i--; j--; sb++; S.back(c, r); }
        else if (dir == 3u) { i--; j--; sb++; sd++; S.back(c, r); }
        else if (dir == 1u) { i--; sd++; S.back(c, r); }
        else { j--; sb++; sd++; }
    }
    emit();
    if (i != i0 || j != j0 || seg != seg_first || match * (cols - kept) - diff * kept != best) bad = true;
    done(bad ? TRACE_ST_STEPS : touched ? TRACE_ST_TOUCHED : wide ? TRACE_ST_WIDE : TRACE_ST_OK, kept);
}

// ---- local alignment inside the band (hinge_trace_local) -----------------------------------------------------------------------
// For end points whose DIAGONAL is off as well: nothing has to reach the box's corners.  Smith-Waterman with linear gap cost in the
// band of k_trace_fill:  H(i, j) = max(0, H(i - 1, j - 1) + (equal ? +match : -diff), H(i - 1, j) - diff, H(i, j - 1) - diff);
// row 0, column 0 and every cell outside the band read as 0.  Tie rule of a cell: 0 wins (the direction of an H = 0 cell is never
// read); among positive candidates diagonal, then the gap in B, then the gap in A.  Kept: the path from the best cell back to the
// first cell with H = 0.  The best cell is the one trace_local_better() prefers - the rule, for the kernel and the test model alike:
// the largest score, of equal scores the smallest anti-diagonal t = i + j, of those the smallest i.
// Claimed: the optimal local alignment WITHIN THE BAND under a linear gap cost, one stretch per placement.  Not claimed: seeding, a
// second stretch, affine gaps, anything outside the band (a stretch the band cuts is reported TOUCHED through the margin below).
__host__ __device__ inline bool trace_local_better(int s, int t, int i, int s0, int t0, int i0) {
    return s > s0 || (s == s0 && (t < t0 || (t == t0 && i < i0)));
}
// TOUCHED in local mode: a kept column within this many diagonals of the band's first or last one.  A stretch the band cuts ends on
// its last match BEFORE the edge, so the edge diagonals alone would let it pass as OK.  The figure: DESIGN.md section 3.9, "Local"
// (the sweep that measured it).  Capped at W / 2, so that the W diagonals in the band's middle are never "touched" (at the legal
// W >= 8 the cap does not bind while the margin is at most 4).
constexpr int TRACE_LOCAL_MARGIN = 3;
__host__ __device__ inline int trace_local_margin(int W) { return TRACE_LOCAL_MARGIN < W / 2 ? TRACE_LOCAL_MARGIN : W / 2; }
// the value lane (own ^ m) of the wavefront holds
#if defined(__HIP__) || defined(__HIPCC__)
__device__ __forceinline__ int trace_lane_xor(int v, int m) { return __shfl_xor(v, m, 64); }
#else   // a host build of the tests (tests/trace_host): the driver that runs k_trace_fill_local supplies the exchange of its 64 threads
inline int (*trace_lane_xor_host)(int, int) = nullptr;
inline int trace_lane_xor(int v, int m) { return trace_lane_xor_host(v, m); }
#endif

// k_trace_fill with another cell: the same band, anti-diagonal order, three rings + acc + cr (all entries 0, margins included: no
// sentinel), the same direction words in the same scratch.  best[3 x ..] = score, i1, j1 (score 0: nothing positive in the band).
// Every lane keeps the first cell it met with its largest score; lanes meet their cells in (t, i) order, so one wavefront reduction
// under trace_local_better() gives the rule's cell.  Loops: k_trace_fill's, then six cross-lane steps.
__global__ __launch_bounds__(64) void k_trace_fill_local(CnsSeqs SA, CnsSeqs SB, const TraceJob* __restrict__ jobs, int n_jobs, int W, int match, int diff,
                                                         unsigned* __restrict__ dirs, int* __restrict__ best) {
    extern __shared__ __align__(16) unsigned char trace_lds[];
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int lane = threadIdx.x;
    const TraceJob J = jobs[job];
    const int alen = J.ae - J.ab, blen = J.be - J.bb;
    if (alen <= 0 || blen <= 0 || abs(blen - alen) > W) {       // (the host never sends these; the walk reports NO_PATH)
        if (lane == 0) { best[3ll * job] = 0; best[3ll * job + 1] = 0; best[3ll * job + 2] = 0; }
        return;
    }
    const int N = trace_ring(W), mask = N - 1;
    int* cur = reinterpret_cast<int*>(trace_lds);
    int* p1 = cur + N;                                           // anti-diagonal t - 1
    int* p2 = p1 + N;                                            // anti-diagonal t - 2
    unsigned* acc = reinterpret_cast<unsigned*>(p2 + N);         // per row: the direction word being filled
    short* cr = reinterpret_cast<short*>(acc + N);               // per row inside the band: c(i) (|c| <= W)
    for (int x = lane; x < N; x += 64) { cur[x] = 0; p1[x] = 0; p2[x] = 0; acc[x] = 0u; cr[x] = 0; }
    __syncthreads();
    CnsPair P;
    P.abps = SA.bps; P.aoff = SA.boff[J.a]; P.bbps = SB.bps; P.boff = SB.boff[J.b]; P.comp = J.comp; P.blen = J.blen;
    TraceStep S;
    S.init(alen, blen);
    int lo_i = 0, lo_c = 0, hi_i = 0, hi_c = 0;
    long long lo_r = alen, hi_r = alen;
    for (int s = 0; s <= W; s++) {                               // rows of anti-diagonal 0 (as k_trace_fill)
        if (hi_i >= alen) break;
        int c = hi_c; long long r = hi_r;
        S.fwd(c, r);
        if (2 * (hi_i + 1) + c > W) break;
        hi_i++; hi_c = c; hi_r = r;
        if (lane == 0) cr[hi_i & mask] = (short)c;
    }
    __syncthreads();
    const int wpr = trace_row_words(W);
    unsigned* __restrict__ my_dirs = dirs + J.dir_off;
    const int T = alen + blen;
    int b_s = 0, b_t = 0, b_i = 0;                               // this lane's best cell
    for (int t = 0; t <= T; t++) {
        const int lo_e = max(max(lo_i, t - blen), 0), hi_e = min(hi_i, t);
        const int first = lo_e - 1, count = hi_e - lo_e + 3;     // one margin cell on either side is written as 0
        const int n_chunks = count > 0 ? (count + 63) >> 6 : 0;
        for (int ch = 0; ch < n_chunks; ch++) {
            const int i = first + (ch << 6) + lane;
            if (i <= hi_e + 1) {
                int val = 0;
                if (i >= lo_e && i <= hi_e) {
                    const int j = t - i;
                    unsigned dir = 0u;
                    if (i >= 1 && j >= 1) {
                        const int eq = P.A(J.ab + i - 1) == P.B(J.bb + j - 1);
                        int h = p2[(i - 1) & mask] + (eq ? match : -diff);
                        dir = eq ? 0u : 3u;
                        { const int g = p1[(i - 1) & mask] - diff; if (g > h) { h = g; dir = 1u; } }
                        { const int g = p1[i & mask] - diff; if (g > h) { h = g; dir = 2u; } }
                        val = max(h, 0);
                        if (val > b_s) { b_s = val; b_t = t; b_i = i; }
                    }
                    if (i >= 1) {
                        const int k = t - (2 * i + (int)cr[i & mask]) + W;
                        if ((unsigned)k < (unsigned)(2 * W)) {
                            unsigned a = acc[i & mask] | (dir << (2 * (k & 15)));
                            if ((k & 15) == 15 || j == blen) { my_dirs[(long long)(i - 1) * wpr + (k >> 4)] = a; a = 0u; }   // the word is complete / the row ends
                            acc[i & mask] = a;
                        }
                    }
                }
                cur[i & mask] = val;
            }
        }
        if (lo_i < alen && 2 * lo_i + lo_c < t + 2 - W) { lo_i++; S.fwd(lo_c, lo_r); }
        if (hi_i < alen) {
            int c = hi_c; long long r = hi_r;
            S.fwd(c, r);
            if (2 * (hi_i + 1) + c <= t + 1 + W) {
                hi_i++; hi_c = c; hi_r = r;
                if (lane == 0) cr[hi_i & mask] = (short)c;
            }
        }
        int* const tmp = p2; p2 = p1; p1 = cur; cur = tmp;
        __syncthreads();
    }
    for (int m = 32; m >= 1; m >>= 1) {                          // all 64 lanes are here: the loops above are wavefront-uniform
        const int o_s = trace_lane_xor(b_s, m), o_t = trace_lane_xor(b_t, m), o_i = trace_lane_xor(b_i, m);
        if (trace_local_better(o_s, o_t, o_i, b_s, b_t, b_i)) { b_s = o_s; b_t = o_t; b_i = o_i; }
    }
    if (lane == 0) { best[3ll * job] = b_s; best[3ll * job + 1] = b_i; best[3ll * job + 2] = b_t - b_i; }
}

// One LANE per placement: from the best cell (i1, j1) back while q = H of the cell it stands on is positive: q -= match on direction
// 0, q += diff on 1, 2 and 3.  0 wins a cell's ties, so the cell where q reaches 0 is the start cell (i0, j0); no direction is read
// there, and it may lie one diagonal outside the band, in row 0 or in column 0.  The kept run begins and ends with a match column,
// so every kept B-only step has an A base in front of it: the segment slots are those of the job's layout, as in k_trace_clip's
// walk 2.  STEPS: q still positive after alen + blen + 1 trips, a direction wanted outside the band or below row 1, or
// match x (columns - diffs) - diff x diffs is not the score.  margin: trace_local_margin(W).  The loop: at most alen + blen + 1 trips.
__global__ __launch_bounds__(64) void k_trace_walk_local(const TraceJob* __restrict__ jobs, int n_jobs, int W, int tspace, int tmax, int match, int diff, int min_score, int margin,
                                                         const unsigned* __restrict__ dirs, const int* __restrict__ best, unsigned short* __restrict__ trace,
                                                         int* __restrict__ diffs, int* __restrict__ status, int* __restrict__ clip, int* __restrict__ score) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= n_jobs) return;
    const TraceJob J = jobs[x];
    const int alen = J.ae - J.ab, blen = J.be - J.bb;
    int i0 = 0, j0 = 0, i1 = 0, j1 = 0, sc = 0;
    auto done = [&](int code, int d) {
        clip[4ll * x] = i0; clip[4ll * x + 1] = j0; clip[4ll * x + 2] = i1; clip[4ll * x + 3] = j1;
        score[x] = sc;
        diffs[x] = d;
        status[x] = code;
    };
    if (alen <= 0 || blen <= 0 || abs(blen - alen) > W) { done(TRACE_ST_NO_PATH, 0); return; }
    const int b_s = best[3ll * x], b_i = best[3ll * x + 1], b_j = best[3ll * x + 2];
    if (b_s < 0 || b_i < 0 || b_i > alen || b_j < 0 || b_j > blen) { done(TRACE_ST_STEPS, 0); return; }   // (never written)
    sc = b_s;
    if (sc < max(1, min_score)) { done(TRACE_ST_EMPTY, 0); return; }
    i1 = b_i; j1 = b_j; i0 = i1; j0 = j1;
    TraceStep S;
    S.init(alen, blen);
    const int wpr = trace_row_words(W);
    const unsigned* __restrict__ my_dirs = dirs + J.dir_off;
    unsigned short* __restrict__ my_trace = trace + J.trace_off;
    const int seg_base = J.ab / tspace;
    int i = i1, j = j1, c = trace_centre(i1, alen, blen);
    long long r = 2ll * i1 * ((long long)blen - alen) + alen - 2ll * alen * c;
    int seg = i1 > 0 ? (J.ab + i1 - 1) / tspace - seg_base : 0, sd = 0, sb = 0, kept = 0, cols = 0, q = sc;
    bool touched = false, wide = false, bad = false;
    auto emit = [&]() {
        if (seg >= 0 && seg < J.nseg) {
            my_trace[2 * seg] = (unsigned short)min(sd, tmax);
            my_trace[2 * seg + 1] = (unsigned short)min(sb, tmax);
        } else bad = true;
        if (sd > tmax || sb > tmax) wide = true;
        kept += sd;
    };
    const int max_steps = alen + blen + 1;
    for (int step = 0; step < max_steps; step++) {
        if (q == 0) break;
        if (i < 1 || j < 0) { bad = true; break; }
        const int k = j - i - c + W;
        if ((unsigned)k >= (unsigned)(2 * W)) { bad = true; break; }
        if (k < margin || k >= 2 * W - margin) touched = true;
        const unsigned dir = (my_dirs[(long long)(i - 1) * wpr + (k >> 4)] >> (2 * (k & 15))) & 3u;
        if (dir != 1u && j == 0) { bad = true; break; }
        const int s = (J.ab + i - 1) / tspace - seg_base;
        if (s != seg) { emit(); seg = s; sd = 0; sb = 0; }
        cols++;
        if (dir == 0u) { i--; j--; sb++; q -= match; S.back(c, r); }
        else if (dir == 3u) { i--; j--; sb++; sd++; q += diff; S.back(c, r); }
        else if (dir == 1u) { i--; sd++; q += diff; S.back(c, r); }
        else { j--; sb++; sd++; q += diff; }
    }
    emit();
    i0 = i; j0 = j;
    if (q != 0 || i0 >= i1 || j0 >= j1 || seg != (J.ab + i0) / tspace - seg_base || match * (cols - kept) - diff * kept != sc) bad = true;
    done(bad ? TRACE_ST_STEPS : touched ? TRACE_ST_TOUCHED : wide ? TRACE_ST_WIDE : TRACE_ST_OK, kept);
}

}  // namespace hinge
