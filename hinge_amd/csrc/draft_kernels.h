// `hinge draft` on the GPU (second half; reference: src/consensus/draft.cpp:125-715 with lib/DW_banded.c and
// lib/falcon.c under it).  Included by hinge_capi.hip after consensus_kernels.h (the realignment between trace points is the same
// kernel, k_cns_realign: recoverAlignment, LAInterface.cpp:4125-4244).
//
//   k_draft_map     one thread per trace-point segment: its indel list -> get_mapping (draft.cpp:70-87) of the alignment's forward
//                   tags: for every A base of the alignment the number of B bases in front of its column (+ bit 31: its column
//                   holds a gap in B - what the host needs to turn the map around for a strand-1 edge)
//   k_draft_align   one WAVEFRONT per (ladder, member): falcon's banded O(ND) alignment of the member against the ladder's
//                   template (DW_banded.c:97-311) - the diagonals of one d across the lanes, V / U in LDS, the (d, k) records 4 bytes
//                   each in HBM, the trace-back by lane 0, then the alignment tags (falcon.c:68-125, with the leading 'T' column of
//                   draft.cpp:646-655) written run by run, a run's columns across the lanes
//   k_draft_align_long  the same for members of 32768+ bases or V / U beyond the LDS: 32-bit cells in HBM.  Both are
//                   ONE body, draft_align<P>.  The cell policies DraftCellsLds / DraftCellsHbm hold what differs: where a job's
//                   V / U / staged sequences live and how wide a cell is, how a (d, k) record is packed, which cursor draws the
//                   jobs.  The host sizes a job's scratch with the same policies (draft_capi.inc)
//   k_draft_cns     one WAVEFRONT per ladder, one LANE per member: falcon's consensus over the members' tags (falcon.c:246-517) -
//                   the columns (t_pos, delta, base) are visited in the reference's order, the members that share a column vote with
//                   ballots (a link = the member's previous column; equal links are found with readlane + ballot, in member order =
//                   the reference's insertion order, so ties fall the same way), scores as doubled integers (the reference adds
//                   link counts and halves of the coverage: exact in either form), the best-predecessor table in HBM, the
//                   trace-back by lane 0 - including the reference's habit of deciding the LAST base by a link index
//   k_draft_cns_deep    k_draft_cns for ladders of 65 .. 65535 members: 64-lane chunks, links numbered in global member order.  The
//                   voting is its own; the score store (draft_s2_put) and the trace-back (draft_cns_emit) are shared
//
// Everything is integer work on 2-bit bases; nothing here is GEMM-shaped.  Bound: latency (dependent look-ups along one
// alignment path), hidden by running thousands of ladders' wavefronts side by side.
#pragma once

namespace hinge {

struct DraftSeq { long long boff; int rlen, strand, start, len; };     // bases [start, start + len) of the read in its strand frame

__device__ __forceinline__ int draft_base(const unsigned char* __restrict__ bps, const DraftSeq& s, int x) {
    const int p = s.start + x;
    return s.strand ? 3 - cns_base(bps, s.boff, s.rlen - 1 - p) : cns_base(bps, s.boff, p);
}

// 16 consecutive bases x .. x + 15 of a sequence in ITS frame as one word, the first base in the top two bits (cns_window's form; the
// complemented strand as CnsPair::winB makes it).  What lies behind the sequence's end is whatever follows: callers bound their use.
__device__ __forceinline__ unsigned draft_window(const unsigned char* __restrict__ bps, const DraftSeq& s, int x) {
    const int p0 = s.start + x;
    if (!s.strand) return cns_window(bps, s.boff, p0);
    const int p = s.rlen - 1 - p0;            // base x + t is the complement of read base p - t
    unsigned v;
    if (p >= 15) v = cns_window(bps, s.boff, p - 15);
    else { v = 0; for (int t = 0; t <= p; t++) v |= (unsigned)cns_base(bps, s.boff, t) << (2 * (p - t)); }
    v = __brev(v);
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    return ~v;
}
// words of a staged sequence: bases 16 i .. 16 i + 15 in word i, one spare word behind the last base's word
__host__ __device__ inline int draft_words(int len) { return (len + 15) / 16 + 1; }
// bases x .. x + 15 out of the staged words (x < len)
__device__ __forceinline__ unsigned draft_lds_window(const unsigned* W, int x) {
    const int i = x >> 4;
    const unsigned long long two = ((unsigned long long)W[i] << 32) | W[i + 1];
    return (unsigned)((two << (2 * (x & 15))) >> 32);
}
__device__ __forceinline__ int draft_lds_base(const unsigned* W, int x) { return (int)((W[x >> 4] >> (30 - 2 * (x & 15))) & 3u); }
// stages a sequence across the lanes: the words that start inside it from draft_window, the spare word 0 - nothing is loaded from a
// window at or past the sequence's end (behind the last read of the base buffer that is memory nobody allocated)
__device__ __forceinline__ void draft_stage(unsigned* W, const unsigned char* __restrict__ bps, const DraftSeq& s, int lane) {
    for (int i = lane; i < draft_words(s.len); i += 64) W[i] = 16 * i < s.len ? draft_window(bps, s, 16 * i) : 0u;
}

constexpr unsigned DRAFT_GAP = 0x80000000u;

__global__ __launch_bounds__(CNS_BLOCK) void k_draft_map(const CnsAln* __restrict__ alns, const CnsSeg* __restrict__ segs, int n_seg, const int* __restrict__ indels,
                                                         const int* __restrict__ n_indel, const long long* __restrict__ map_off, unsigned* __restrict__ mapping) {
    const int s = blockIdx.x * CNS_BLOCK + threadIdx.x;
    if (s >= n_seg) return;
    const CnsSeg g = segs[s];
    const CnsAln al = alns[g.aln];
    unsigned* __restrict__ m = mapping + map_off[g.aln];
    cns_walk(g, indels + g.out_off, n_indel[s], [&](int kind, int i, int j, int cnt) {
        if (kind == 0) { for (int t = 0; t < cnt; t++) m[i - 1 + t - al.ab] = (unsigned)(j - 1 + t - al.bb); }
        else if (kind == 2) m[i - 1 - al.ab] = (unsigned)(j - 1 - al.bb) | DRAFT_GAP;
        return true;
    });
}

// ---- falcon's aligner, one wavefront per job ---------------------------------------------------------------------------------
struct DraftJob {
    DraftSeq q, t;              // query = the member, target = the ladder's template
    long long ent_off;          // its (d, k) records: ent_cap words
    long long dtab_off;         // per d: first record, min_k  (2 * (max_d + 1) ints)
    long long tag_off;          // its tags (q.len + t.len + 2 words) ...
    int ent_cap, max_d;
};
constexpr int DRAFT_ST_CAP = 1;      // a record / tag buffer too small (host sizing bug)
constexpr int DRAFT_ST_DELTA = 2;    // a run of 255+ inserted bases: the reference's tags are undefined there (falcon.c:96)
constexpr int DRAFT_ST_BASE = 4;
// the words of `status`: the DRAFT_ST_* flags of a call, then one cursor per kernel that draws its work (cleared per batch)
enum { DRAFT_SLOT_FLAGS, DRAFT_SLOT_ALIGN, DRAFT_SLOT_CNS, DRAFT_SLOT_ALIGN_LONG, DRAFT_SLOT_CNS_DEEP, DRAFT_SLOTS };

// a tag: t_pos << 11 | delta << 3 | base (0-3 A C G T, 4 '-')
__device__ __forceinline__ unsigned draft_tag(int t_pos, int delta, int base) { return ((unsigned)t_pos << 11) | ((unsigned)delta << 3) | (unsigned)base; }

__host__ __device__ inline int draft_dtab_words(int max_d) { return 2 * (max_d + 1); }      // a job's per-d table (DraftJob::dtab_off)

// A job's scratch, the ONE place that lays it out - the kernels place it, the host sizes it with words(): V and U, [2 * max_d + 2]
// cells each, then both sequences staged 16 bases per word.  The trace-back's path (the record index of every d on it: at most max_d
// ints) reuses the V / U words, which nobody needs by then.
template <class Cell> struct DraftScratch {
    Cell *V, *U;
    unsigned *Wq, *Wt;
    int* vu;                    // the V / U words as ints: cleared at the start of a job, the path's at its end
    int n_vu;
    __host__ __device__ static int vu_words(int max_d) { return 2 * (2 * max_d + 2) * (int)sizeof(Cell) / (int)sizeof(int); }
    __host__ __device__ static int words(int max_d, int q_len, int t_len) { return vu_words(max_d) + draft_words(q_len) + draft_words(t_len); }
    __device__ __forceinline__ DraftScratch(int* at, int max_d, int q_len)
        : V(reinterpret_cast<Cell*>(at)), U(V + (2 * max_d + 2)), Wq(reinterpret_cast<unsigned*>(at + vu_words(max_d))), Wt(Wq + draft_words(q_len)), vu(at), n_vu(vu_words(max_d)) {}
};
struct DraftRec { int x1, x2; bool x_step; };      // a (d, k) record: the snake x1 .. x2, reached from k - 1 (a query base against a gap)

// The two cell policies of draft_align: what k_draft_align and k_draft_align_long differ in, and nothing else.
// V / U as 16-bit cells in LDS (x < 32768: a member has fewer bases; x + y < 65536): half the LDS of 32-bit cells, i.e. twice the
// wavefronts per CU for a kernel whose wavefronts wait half their cycles (a latency chain per round).  A record is one word:
// x1 (15 bits) | came from k - 1 | x2 (16 bits).
struct DraftCellsLds {
    typedef unsigned short cell;
    typedef int count;                                        // records and columns of a job
    typedef DraftScratch<cell> scratch;
    static constexpr int CURSOR = DRAFT_SLOT_ALIGN, REC_WORDS = 1;
    __device__ __forceinline__ static scratch place(int* lds, int* DT, int max_d, int q_len) { return scratch(lds, max_d, q_len); }
    __device__ __forceinline__ static void put(unsigned* __restrict__ E, count at, int x1, unsigned pre_minus, int x2) { E[at] = ((unsigned)x1 << 17) | (pre_minus << 16) | (unsigned)x2; }
    __device__ __forceinline__ static DraftRec get(const unsigned* __restrict__ E, count at) { const unsigned e = E[at]; return DraftRec{(int)(e >> 17), (int)(e & 0xffffu), (bool)((e >> 16) & 1u)}; }
    __device__ __forceinline__ static bool x_step(const unsigned* __restrict__ E, count at) { return (E[at] >> 16) & 1u; }
};
// Long jobs (members of 32768+ bases, or a scratch beyond the LDS): 32-bit cells, the scratch in the job's stretch of
// dtab behind its per-d table, a record as two words (x1, then came from k - 1 << 31 | x2), 64-bit record and column counts.
struct DraftCellsHbm {
    typedef int cell;
    typedef long long count;
    typedef DraftScratch<cell> scratch;
    static constexpr int CURSOR = DRAFT_SLOT_ALIGN_LONG, REC_WORDS = 2;
    __device__ __forceinline__ static scratch place(int* lds, int* DT, int max_d, int q_len) { return scratch(DT + draft_dtab_words(max_d), max_d, q_len); }
    __device__ __forceinline__ static void put(unsigned* __restrict__ E, count at, int x1, unsigned pre_minus, int x2) { E[2 * at] = (unsigned)x1; E[2 * at + 1] = (pre_minus << 31) | (unsigned)x2; }
    __device__ __forceinline__ static DraftRec get(const unsigned* __restrict__ E, count at) { const unsigned w = E[2 * at + 1]; return DraftRec{(int)E[2 * at], (int)(w & 0x7fffffffu), (bool)(w >> 31)}; }
    __device__ __forceinline__ static bool x_step(const unsigned* __restrict__ E, count at) { return E[2 * at + 1] >> 31; }
};

// Jobs jb_base .. jb_base + n_jobs - 1, one wavefront each.  `lds` is the launch's dynamic LDS where the policy keeps its cells there.
template <class P>
__device__ __forceinline__ void draft_align(int* lds, const unsigned char* __restrict__ bps, const DraftJob* __restrict__ jobs, int jb_base, int n_jobs, int band_tol,
                                            unsigned* __restrict__ ents, int* __restrict__ dtab, unsigned* __restrict__ tags, int* __restrict__ n_tags, int* __restrict__ status) {
    typedef typename P::cell cell;
    typedef typename P::count count;
    const int lane = threadIdx.x;
    // jobs are DRAWN (status[P::CURSOR] is the cursor, zero at launch): an alignment's time follows its edit distance - the template
    // against itself is over at d = 0, a diverged member takes 250 rounds - and with a fixed stride the launch waited for its
    // unluckiest wavefront at twice the mean (SQ_WAVE_CYCLES / waves = 51 % of the launch, profiles/r6f_draft_*)
    while (true) {
        int jb = 0;
        if (lane == 0) jb = atomicAdd(status + P::CURSOR, 1);
        jb = __builtin_amdgcn_readfirstlane(jb);
        if (jb >= n_jobs) break;
        jb += jb_base;
        const DraftJob J = jobs[jb];
        const int q_len = J.q.len, t_len = J.t.len, max_d = J.max_d;
        int* __restrict__ DT = dtab + J.dtab_off;
        const typename P::scratch S = P::place(lds, DT, max_d, q_len);
        cell* const V = S.V;
        cell* const U = S.U;
        // Round 6: both sequences staged, 16 bases per word in their own frame (strand applied once here, not per base), so a
        // snake compares 16 base pairs per step - two staged words per side, one XOR, one count of leading zeros - instead of two
        // dependent byte loads from global memory per base pair (12 % errors: a snake is ~8 bases, i.e. ONE step).
        unsigned* const Wq = S.Wq;
        unsigned* const Wt = S.Wt;
        for (int i = lane; i < S.n_vu; i += 64) S.vu[i] = 0;
        draft_stage(Wq, bps, J.q, lane);
        draft_stage(Wt, bps, J.t, lane);
        __syncthreads();
        const int k_off = max_d, band_size = band_tol * 2;
        unsigned* __restrict__ E = ents + J.ent_off;
        unsigned* __restrict__ TG = tags + J.tag_off;
        int best_m = -1, min_k = 0, max_k = 0;
        count n_ent = 0;
        int fin_d = -1, fin_k = 0;
        bool overflow = false;
        for (int d = 0; d < max_d; d++) {
            if (max_k - min_k > band_size) break;
            const int nk = (max_k - min_k) / 2 + 1;
            if (n_ent + nk > J.ent_cap) { overflow = true; break; }
            if (lane == 0) { DT[2 * d] = (int)n_ent; DT[2 * d + 1] = min_k; }
            int my_best = -1;
            unsigned long long done_any = 0ull;
            int done_at = 0;
            for (int it = 0; it * 64 < nk && !done_any; it++) {
                const int idx = it * 64 + lane;
                const bool on = idx < nk;
                const int k = min_k + 2 * idx;
                int x = 0, y = 0;
                bool fin = false;
                if (on) {
                    unsigned pre_minus;
                    if (k == min_k || (k != max_k && V[k - 1 + k_off] < V[k + 1 + k_off])) { pre_minus = 0u; x = (int)V[k + 1 + k_off]; }
                    else { pre_minus = 1u; x = (int)V[k - 1 + k_off] + 1; }
                    y = x - k;
                    const int x1 = x;
                    while (true) {          // the snake, 16 base pairs at a time
                        const int rem = min(q_len - x, t_len - y);
                        if (rem <= 0) break;
                        const unsigned df = draft_lds_window(Wq, x) ^ draft_lds_window(Wt, y);
                        const int m = min(df ? (int)(__clz(df) >> 1) : 16, rem);
                        x += m; y += m;
                        if (m < 16) break;
                    }
                    P::put(E, n_ent + idx, x1, pre_minus, x);
                    fin = x >= q_len || y >= t_len;
                }
                __syncthreads();            // (one wavefront: orders the reads of V above before the writes below; for cells in HBM its fence makes them visible across lanes)
                if (on) { V[k + k_off] = (cell)x; U[k + k_off] = (cell)(x + y); my_best = max(my_best, x + y); }
                done_any = __ballot(on && fin);
                if (done_any) done_at = it * 64 + (int)__builtin_ctzll(done_any);
                __syncthreads();
            }
            if (done_any) {                 // the reference breaks at the first k (ascending) that reaches an end
                fin_d = d; fin_k = min_k + 2 * done_at;
                n_ent += done_at + 1;
                break;
            }
            n_ent += nk;
            best_m = max(best_m, wave_max(my_best));          // (DPP reduction; the kernel issues 0.71 of the vector peak: instructions count)
            // the band's new ends: first / last diagonal within band_tol of the best anti-diagonal - one ballot per 64 diagonals, the
            // ends read off the mask on the scalar side (was: two 64-lane shuffle reductions per round)
            int lo = max_k, hi = min_k;
            for (int c = 0; c * 64 < nk; c++) {
                const int idx = c * 64 + lane;
                const bool ok = idx < nk && (int)U[min_k + 2 * idx + k_off] >= best_m - band_tol;
                const unsigned long long Bm = __ballot(ok);
                if (Bm) {
                    lo = min(lo, min_k + 2 * (c * 64 + (int)__builtin_ctzll(Bm)));
                    hi = max(hi, min_k + 2 * (c * 64 + 63 - (int)__builtin_clzll(Bm)));
                }
            }
            max_k = hi + 1; min_k = lo - 1;
            __syncthreads();
        }
        if (overflow && lane == 0) atomicOr(status + DRAFT_SLOT_FLAGS, DRAFT_ST_CAP);
        // ---- tags: the leading 'T' column, then the path's columns (falcon.c:68-125 on the rows of DW_banded.c:245-300) ---------------
        if (lane == 0) TG[0] = draft_tag(0, 0, 3);
        count n_col = 1;
        if (fin_d >= 0 && !overflow) {
            // trace-back: record index of every d on the path, kept in the V / U words (no longer needed; d < max_d ints)
            int* path = S.vu;
            __syncthreads();
            if (lane == 0) {
                int ck = fin_k;
                for (int cd = fin_d; cd >= 0; cd--) {
                    const int at = DT[2 * cd] + (ck - DT[2 * cd + 1]) / 2;
                    path[cd] = at;
                    ck = P::x_step(E, at) ? ck - 1 : ck + 1;
                }
            }
            __syncthreads();
            int jj = 0;                     // consecutive inserted bases in front of the next column
            int py = 0;                     // target bases consumed so far
            int px = 0;
            bool bad_delta = false;
            const count col_cap = (count)q_len + t_len + 2;
            for (int cd = 0; cd <= fin_d; cd++) {
                const DraftRec e = P::get(E, path[cd]);
                if (cd > 0) {               // the edit step from (px, py): one column (y1 follows from the step kind)
                    if (n_col + 1 > col_cap) { overflow = true; break; }
                    if (e.x_step) {              // came from k - 1: a query base against a gap
                        jj += 1;
                        if (jj >= 255) bad_delta = true;
                        if (lane == 0) TG[n_col] = draft_tag(py, jj & 255, draft_lds_base(Wq, px));
                        px += 1;
                    } else {
                        jj = 0;
                        py += 1;
                        if (lane == 0) TG[n_col] = draft_tag(py, 0, 4);
                    }
                    n_col += 1;
                }
                const int run = e.x2 - e.x1;  // the snake: run matched pairs
                if (run > 0) {
                    if (n_col + run > col_cap) { overflow = true; break; }
                    for (int t = lane; t < run; t += 64) TG[n_col + t] = draft_tag(py + 1 + t, 0, draft_lds_base(Wq, px + t));
                    n_col += run; px += run; py += run; jj = 0;
                }
            }
            if (lane == 0 && bad_delta) atomicOr(status + DRAFT_SLOT_FLAGS, DRAFT_ST_DELTA);
            if (lane == 0 && overflow) atomicOr(status + DRAFT_SLOT_FLAGS, DRAFT_ST_CAP);
        }
        if (lane == 0) n_tags[jb] = (int)n_col;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_draft_align(const unsigned char* __restrict__ bps, const DraftJob* __restrict__ jobs, int n_jobs, int band_tol,
                                                    unsigned* __restrict__ ents, int* __restrict__ dtab, unsigned* __restrict__ tags, int* __restrict__ n_tags,
                                                    int* __restrict__ status) {
    extern __shared__ int lds[];
    draft_align<DraftCellsLds>(lds, bps, jobs, 0, n_jobs, band_tol, ents, dtab, tags, n_tags, status);
}
// jobs jb_base .. jb_base + n_jobs - 1: in a batch the long ladders' jobs lie behind the short ones'
__global__ __launch_bounds__(64) void k_draft_align_long(const unsigned char* __restrict__ bps, const DraftJob* __restrict__ jobs, int jb_base, int n_jobs, int band_tol,
                                                         unsigned* __restrict__ ents, int* __restrict__ dtab, unsigned* __restrict__ tags, int* __restrict__ n_tags,
                                                         int* __restrict__ status) {
    draft_align<DraftCellsHbm>(nullptr, bps, jobs, jb_base, n_jobs, band_tol, ents, dtab, tags, n_tags, status);
}

// ---- falcon's consensus, one wavefront per ladder ---------------------------------------------------------------------------
struct DraftLadder {
    int job0, n;                // its jobs (members), n <= 64
    int t_len;                  // template length + 1
    long long col_off;          // best-predecessor table: col_cap words
    long long tb_off;           // per t: first (t, delta) slot, coverage  (2 * t_len ints)
    long long out_off;          // its consensus: up to 2 * t_len characters
    int col_cap;
};
constexpr unsigned DRAFT_NONE = 0xffffffffu;
constexpr int DRAFT_S2_LDS = 32;     // deltas (consecutive inserted bases in front of a template position) whose column scores live in LDS

// where the column (t, delta, base) leaves its doubled score: the current and the previous template position are kept, by parity.
// (The look-up of a predecessor's score - the same index from a tag word - stays written out in the two kernels: as a shared function
// it changed k_draft_cns_deep's instruction order and cost it 2.3 %, profiles/r8a_draft_refactor_ab.json.)
__device__ __forceinline__ void draft_s2_put(int (*S2)[DRAFT_S2_LDS][5], int* __restrict__ S2F, int t, int delta, int base, int score) {
    // (the LDS store through an LDS-typed pointer: two stores of one value through generic pointers are folded into ONE flat store at
    // a selected address - five of them per column in k_draft_cns - where the kernels had a ds_write and a global store)
    typedef __attribute__((address_space(3))) int lds_int;
    if (delta < DRAFT_S2_LDS) *(lds_int*)&S2[t & 1][delta][base] = score; else S2F[((t & 1) * 256 + delta) * 5 + base] = score;
}

// The sequence of a ladder, back to front from its best column (falcon.c:440-478), then turned around; returns its length.  One lane.
// C = the best-predecessor table, TB = per t its first slot and coverage, (g_col, g_ck, g_t) = the best column, the LINK index its
// score came from - the reference decides the last base by it - and its template position.
__device__ __forceinline__ int draft_cns_emit(const DraftLadder& L, const unsigned* __restrict__ C, const int* __restrict__ TB, char* __restrict__ o, unsigned g_col, int g_ck,
                                              int g_t, bool cap_hit, unsigned min_cov, int* __restrict__ status) {
    int len = 0;
    if (g_col != DRAFT_NONE && !cap_hit) {
        char bb = '$';
        int ck = g_ck, i = g_t;
        unsigned col = g_col;
        while (true) {
            if (ck >= 0 && ck < 5) bb = (unsigned)TB[2 * i + 1] > min_cov ? "ACGT-"[ck] : "acgt-"[ck];
            const unsigned bp = C[col];
            if (bp == DRAFT_NONE || len >= 2 * L.t_len) break;
            i = (int)(bp >> 11);
            const int j = (int)((bp >> 3) & 255u);
            ck = (int)(bp & 7u);
            col = (unsigned)((TB[2 * i] + j) * 5 + ck);
            if (bb != '-') o[len++] = bb;
        }
        for (int a = 0, b = len - 1; a < b; a++, b--) { const char c = o[a]; o[a] = o[b]; o[b] = c; }
    } else if (!cap_hit) {
        atomicOr(status + DRAFT_SLOT_FLAGS, DRAFT_ST_BASE);       // (the reference's assert(g_best_score != -1))
    }
    return len;
}

__global__ __launch_bounds__(64) void k_draft_cns(const DraftJob* __restrict__ jobs, const DraftLadder* __restrict__ ladders, int n_ladders, const unsigned* __restrict__ tags,
                                                  const int* __restrict__ n_tags, unsigned* __restrict__ cols, int* __restrict__ tbase, char* __restrict__ out,
                                                  int* __restrict__ out_len, unsigned min_cov, int* __restrict__ status, int* __restrict__ s2_far) {
    // doubled scores of the columns of the current and the previous template position.  Round 6: the columns of the first
    // DRAFT_S2_LDS deltas in LDS (1.3 instead of 10 KiB per wavefront: 32 instead of 16 wavefronts per CU for a kernel that is one
    // dependent chain per ladder), the rest - 32+ inserted bases in a row - in a per-workgroup stretch of s2_far
    __shared__ int S2[2][DRAFT_S2_LDS][5];
    int* __restrict__ const S2F = s2_far + (size_t)blockIdx.x * (2 * 256 * 5);
    const int lane = threadIdx.x;
    while (true) {                           // ladders are drawn (status[DRAFT_SLOT_CNS], zero at launch): their times differ with their members
        int ld = 0;
        if (lane == 0) ld = atomicAdd(status + DRAFT_SLOT_CNS, 1);
        ld = __builtin_amdgcn_readfirstlane(ld);
        if (ld >= n_ladders) break;
        const DraftLadder L = ladders[ld];
        const bool member = lane < L.n;
        const unsigned* __restrict__ TG = member ? tags + jobs[L.job0 + lane].tag_off : tags;
        const int nt = member ? n_tags[L.job0 + lane] : 0;
        unsigned* __restrict__ C = cols + L.col_off;
        int* __restrict__ TB = tbase + L.tb_off;
        int p = 0;                           // next tag of this lane
        unsigned prev = DRAFT_NONE;          // this lane's previous column (a tag word), DRAFT_NONE in front of its first
        int slot = 0;                        // (t, delta) slots so far
        int g_best = -2, g_ck = 0, g_t = 0;
        unsigned g_col = DRAFT_NONE;         // slot * 5 + base of the best column
        int best_ck = -1;
        bool cap_hit = false;
        for (int t = 0; t < L.t_len; t++) {
            int cov = 0;
            if (lane == 0) TB[2 * t] = slot;
            for (int delta = 0;; delta++) {
                const unsigned tg = p < nt ? TG[p] : DRAFT_NONE;
                const bool has = tg != DRAFT_NONE && (int)(tg >> 11) == t && (int)((tg >> 3) & 255u) == delta;
                const unsigned long long H = __ballot(has);
                if (delta == 0) { cov = __popcll(H); if (lane == 0) TB[2 * t + 1] = cov; }
                if (!H) break;
                if ((slot + 1) * 5 > L.col_cap || delta > 255) { cap_hit = true; break; }
                const int base = (int)(tg & 7u);
                // this lane's predecessor score (doubled); a first tag has none
                int ps = 0;
                if (has && prev != DRAFT_NONE) {
                    const unsigned pt = (prev >> 11) & 1u, pd = (prev >> 3) & 255u, pb = prev & 7u;
                    ps = pd < (unsigned)DRAFT_S2_LDS ? S2[pt][pd][pb] : S2F[(pt * 256 + pd) * 5 + pb];
                }
                for (int kk = 0; kk < 5; kk++) {
                    unsigned long long M = __ballot(has && base == kk);
                    int best = -2;
                    unsigned best_p = 0u;            // (the reference leaves best_p_* of a column without links at zero)
                    int ck = 0;
                    while (M) {
                        const int lead = (int)__builtin_ctzll(M);
                        const unsigned lp = __shfl(prev, lead);
                        const int ls = __shfl(ps, lead);
                        const unsigned long long same = __ballot(has && base == kk && prev == lp);
                        const int score = (lp == DRAFT_NONE ? 0 : ls) + 2 * __popcll(same) - cov;
                        if (score > best) { best = score; best_p = lp; best_ck = ck; }
                        ck++;
                        M &= ~same;
                    }
                    if (lane == 0) {
                        draft_s2_put(S2, S2F, t, delta, kk, best);
                        C[slot * 5 + kk] = best_p;
                    }
                    if (best > g_best) { g_best = best; g_col = (unsigned)(slot * 5 + kk); g_ck = best_ck; g_t = t; }
                }
                __syncthreads();
                if (has) { prev = tg; p++; }
                slot++;
            }
            if (cap_hit) break;
        }
        if (cap_hit && lane == 0) atomicOr(status + DRAFT_SLOT_FLAGS, DRAFT_ST_CAP);
        if (lane == 0) out_len[ld] = draft_cns_emit(L, C, TB, out + L.out_off, g_col, g_ck, g_t, cap_hit, min_cov, status);
        __syncthreads();
    }
}

// ---- ladders of 65 .. 65535 members ----------------------------------------------------------------------------
// k_draft_cns over the members in 64-lane chunks, lane i of chunk c = member 64 c + i.  Per member a cursor in HBM (its next tag,
// its last column); per column (t, delta) one pass over the chunks reads every member's next tag and leaves, per base, a mask of
// the members that carry it (R, LDS); then per base the links are enumerated in GLOBAL member order - the lowest member not
// counted yet names the next link, one pass over the chunks from its chunk on counts (and clears) the members with that link.
// So a link's number is the lowest member index that carries it, as update_col numbers them (falcon.c tag loop), the counts are
// the sums over the chunks, and the strict `score > best` breaks ties as k_draft_cns does.  Everything else - scores, S2 / S2F,
// the best-predecessor table, the trace-back with its link-index quirk (draft_cns_emit) - is k_draft_cns'.
struct DraftMember { long long p, end; unsigned prev; int pad; };

__global__ __launch_bounds__(64) void k_draft_cns_deep(const DraftJob* __restrict__ jobs, const DraftLadder* __restrict__ ladders, int n_ladders, const unsigned* __restrict__ tags,
                                                       const int* __restrict__ n_tags, unsigned* __restrict__ cols, int* __restrict__ tbase, char* __restrict__ out,
                                                       int* __restrict__ out_len, unsigned min_cov, int* __restrict__ status, int* __restrict__ s2_far,
                                                       DraftMember* __restrict__ mstate, unsigned* __restrict__ mlink) {
    __shared__ int S2[2][DRAFT_S2_LDS][5];
    extern __shared__ unsigned long long R[];     // [5][chunks]: the launch's largest ladder sets the size
    int* __restrict__ const S2F = s2_far + (size_t)blockIdx.x * (2 * 256 * 5);
    const int lane = threadIdx.x;
    while (true) {
        int ld = 0;
        if (lane == 0) ld = atomicAdd(status + DRAFT_SLOT_CNS_DEEP, 1);
        ld = __builtin_amdgcn_readfirstlane(ld);
        if (ld >= n_ladders) break;
        const DraftLadder L = ladders[ld];
        const int nc = (L.n + 63) / 64;
        // a lane reads and writes the state of its own members only (64 c + lane): no ordering across lanes is needed for it
        DraftMember* __restrict__ MS = mstate + L.job0;
        unsigned* __restrict__ ML = mlink + L.job0;         // the link (previous column) of a member whose tag is at the current column
        for (int m = lane; m < L.n; m += 64) {
            const long long o = jobs[L.job0 + m].tag_off;
            MS[m] = DraftMember{o, o + n_tags[L.job0 + m], DRAFT_NONE, 0};
        }
        unsigned* __restrict__ C = cols + L.col_off;
        int* __restrict__ TB = tbase + L.tb_off;
        int slot = 0;
        int g_best = -2, g_ck = 0, g_t = 0;
        unsigned g_col = DRAFT_NONE;
        int best_ck = -1;
        bool cap_hit = false;
        for (int t = 0; t < L.t_len; t++) {
            int cov = 0;
            if (lane == 0) TB[2 * t] = slot;
            for (int delta = 0;; delta++) {
                // the members' next tags: who is at (t, delta), with which base; their cursors move on
                int h = 0;
                for (int c = 0; c < nc; c++) {
                    const int m = c * 64 + lane;
                    bool has = false;
                    int base = 7;
                    if (m < L.n) {
                        const DraftMember st = MS[m];
                        const unsigned tg = st.p < st.end ? tags[st.p] : DRAFT_NONE;
                        has = tg != DRAFT_NONE && (int)(tg >> 11) == t && (int)((tg >> 3) & 255u) == delta;
                        if (has) {
                            base = (int)(tg & 7u);
                            ML[m] = st.prev;
                            MS[m] = DraftMember{st.p + 1, st.end, tg, 0};
                        }
                    }
                    h += __popcll(__ballot(has));
                    for (int kk = 0; kk < 5; kk++) {
                        const unsigned long long B = __ballot(base == kk);
                        if (lane == 0) R[kk * nc + c] = B;
                    }
                }
                if (delta == 0) { cov = h; if (lane == 0) TB[2 * t + 1] = cov; }
                if (!h) break;
                if ((slot + 1) * 5 > L.col_cap || delta > 255) { cap_hit = true; break; }
                __syncthreads();
                for (int kk = 0; kk < 5; kk++) {
                    int best = -2;
                    unsigned best_p = 0u;
                    int ck = 0;
                    int c0 = 0;
                    while (true) {
                        while (c0 < nc && R[kk * nc + c0] == 0ull) c0++;
                        if (c0 == nc) break;
                        const int lead = (int)__builtin_ctzll(R[kk * nc + c0]);
                        unsigned lp = 0u;
                        int cnt = 0;
                        for (int c = c0; c < nc; c++) {
                            const unsigned long long Mc = R[kk * nc + c];
                            if (!Mc) continue;
                            const bool mine = (Mc >> lane) & 1ull;
                            const unsigned pv = mine ? ML[c * 64 + lane] : DRAFT_NONE;
                            if (c == c0) lp = __shfl(pv, lead);
                            const unsigned long long same = __ballot(mine && pv == lp);
                            cnt += __popcll(same);
                            if (lane == 0) R[kk * nc + c] = Mc & ~same;
                            __syncthreads();
                        }
                        int ls = 0;
                        if (lp != DRAFT_NONE) {
                            const unsigned pt = (lp >> 11) & 1u, pd = (lp >> 3) & 255u, pb = lp & 7u;
                            ls = pd < (unsigned)DRAFT_S2_LDS ? S2[pt][pd][pb] : S2F[(pt * 256 + pd) * 5 + pb];
                        }
                        const int score = ls + 2 * cnt - cov;
                        if (score > best) { best = score; best_p = lp; best_ck = ck; }
                        ck++;
                    }
                    if (lane == 0) {
                        draft_s2_put(S2, S2F, t, delta, kk, best);
                        C[slot * 5 + kk] = best_p;
                    }
                    if (best > g_best) { g_best = best; g_col = (unsigned)(slot * 5 + kk); g_ck = best_ck; g_t = t; }
                }
                __syncthreads();
                slot++;
            }
            if (cap_hit) break;
        }
        if (cap_hit && lane == 0) atomicOr(status + DRAFT_SLOT_FLAGS, DRAFT_ST_CAP);
        if (lane == 0) out_len[ld] = draft_cns_emit(L, C, TB, out + L.out_off, g_col, g_ck, g_t, cap_hit, min_cov, status);
        __syncthreads();
    }
}

}  // namespace hinge
