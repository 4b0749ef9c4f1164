// C ABI of `hinge overlap` (include/hinge_hip.h, "hinge overlap").  Included by hinge_capi.hip.
// Host work here: the parameters' defaults and ranges, the limits of the key packing, the target blocks and the calls of their k-mer
// indexes (index_capi.inc: built on the device from the resident bases, or by seed_index.h on the host; one block resident at a time), the
// jobs (two per read) in batches under the scratch budget against every block, a candidate's projection in the record's frame
// (overlap_project) and the order of the result.  The kernels: overlap_kernels.h (one candidate per (a, b, strand)) and
// overlap_multi_kernels.h (hinge_overlap_run_multi: up to max_stretches of them); overlap_tile_kernels.h (hinge_overlap_run_tiled: the
// query in half-overlapping tiles, a reduce per job; DESIGN.md 3.14); overlap_tile_multi_kernels.h (hinge_overlap_run_tiled_multi: tiles
// with up to max_stretches candidates per pair; DESIGN.md 3.15).  All entry points are overlap_run_impl.

static_assert(OVL_STRETCHES_MAX == HINGE_OVERLAP_MAX_STRETCHES_LIMIT, "the header's limit is the kernel's");
static_assert(OVT_TILE_MAX == HINGE_OVERLAP_TILE_MAX, "the header's limit is the kernel's");
struct OverlapCand { hinge_cns_alignment r; int32_t cnt, diag, d, p, round; };
struct OverlapState {
    DevBuf jobs, out, codes, gpos, off;
    DevBuf tjobs, tout, top;                       // hinge_overlap_run_tiled: the tile jobs, their rows, the reduce's largest tile per job
    std::vector<OverlapCand> cand;                 // of the last hinge_overlap_run / _run_multi, sorted by (a, b, comp, round)
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hinge_overlap_last_stats
    int64_t tstats[4] = {0, 0, 0, 0};              // hinge_overlap_tile_stats
};

static void overlap_release(hinge_ctx* ctx) {
    OverlapState* t = ctx->ovl_st;
    if (!t) return;
    DevBuf* all[] = {&t->jobs, &t->out, &t->codes, &t->gpos, &t->off, &t->tjobs, &t->tout, &t->top};
    for (DevBuf* b : all) release(*b);
    delete t;
    ctx->ovl_st = nullptr;
}

// One batch: jobs[0..nj) against the resident block; h_out = W ints per job.  S == 0: k_overlap_vote, W = ovl_out_ints(max_partners);
// S >= 1: k_overlap_vote_multi with S rounds, W = ovl_multi_out_ints(max_partners, S).
static int overlap_batch(hinge_ctx* ctx, const OvlJob* jobs, size_t nj, const OvlParams& P, int S, std::vector<int>& h_out) {
    OverlapState* t = ctx->ovl_st;
    CnsState* s = ctx->cns;
    const size_t out_ints = nj * (size_t)(S ? ovl_multi_out_ints(P.max_partners, S) : ovl_out_ints(P.max_partners));
    int rc;
    if ((rc = ensure(ctx, t->jobs, sizeof(OvlJob) * nj))) return rc;
    if ((rc = ensure(ctx, t->out, sizeof(int) * out_ints))) return rc;
    CK(hipMemcpyAsync(t->jobs.p, jobs, sizeof(OvlJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(t->out.p, 0xff, sizeof(int) * out_ints, ctx->stream));   // poison: a slot the kernel did not write is seen as such
    CnsSeqs SB{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
    if (S == 0) {
        ProfScope _ps(ctx, KID_OVERLAP_VOTE);
        hipLaunchKernelGGL(k_overlap_vote, dim3((unsigned)nj), dim3(64), ovl_lds_bytes(P.list), ctx->stream, SB, (const OvlJob*)t->jobs.p, (int)nj, P, (const unsigned*)t->codes.p,
                           (const int*)t->gpos.p, (const long long*)t->off.p, (int*)t->out.p);
    } else {
        ProfScope _ps(ctx, KID_OVERLAP_VOTE_MULTI);
        hipLaunchKernelGGL(k_overlap_vote_multi, dim3((unsigned)nj), dim3(64), ovl_multi_lds_bytes(P.list), ctx->stream, SB, (const OvlJob*)t->jobs.p, (int)nj, P, S,
                           (const unsigned*)t->codes.p, (const int*)t->gpos.p, (const long long*)t->off.p, (int*)t->out.p);
    }
    CK(hipGetLastError());
    h_out.resize(out_ints);
    CK(hipMemcpyAsync(h_out.data(), t->out.p, sizeof(int) * out_ints, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return HINGE_OK;
}

// One batch of hinge_overlap_run_tiled: jobs[0..nj) (each whole, tiles of `tile` bases) against the resident block: k_overlap_vote_tile
// over all their tiles, then k_overlap_tile_reduce per job; h_out = ovl_out_ints(max_partners) ints per job, h_top = one per job.
// S >= 1 (hinge_overlap_run_tiled_multi): k_overlap_vote_tile_multi and k_overlap_tile_reduce_multi with S rounds; a tile row and a
// job's row are ovl_multi_out_ints(max_partners, S) ints.
static int overlap_batch_tiled(hinge_ctx* ctx, const OvlJob* jobs, size_t nj, const OvlParams& P, const OvlTileParams& TP, int S, std::vector<OvlTileJob>& tj, std::vector<OvlRedJob>& rj,
                               std::vector<int>& h_out, std::vector<int>& h_top) {
    OverlapState* t = ctx->ovl_st;
    CnsState* s = ctx->cns;
    tj.clear(); rj.clear();
    for (size_t j = 0; j < nj; j++) {
        const int nt = (int)ovl_tile_count(jobs[j].alen, P.k, TP.tile);
        rj.push_back(OvlRedJob{(int)tj.size(), nt});
        for (int x = 0; x < nt; x++) tj.push_back(OvlTileJob{jobs[j].a, jobs[j].comp, jobs[j].alen, x});
    }
    const size_t W = (size_t)(S ? ovl_multi_out_ints(P.max_partners, S) : ovl_out_ints(P.max_partners)), nt = tj.size(), row_ints = nt * W, out_ints = nj * W;
    int rc;
    if ((rc = ensure(ctx, t->tjobs, sizeof(OvlTileJob) * nt))) return rc;
    if ((rc = ensure(ctx, t->tout, sizeof(int) * row_ints))) return rc;
    if ((rc = ensure(ctx, t->jobs, sizeof(OvlRedJob) * nj))) return rc;
    if ((rc = ensure(ctx, t->out, sizeof(int) * out_ints))) return rc;
    if ((rc = ensure(ctx, t->top, sizeof(int) * nj))) return rc;
    CK(hipMemcpyAsync(t->tjobs.p, tj.data(), sizeof(OvlTileJob) * nt, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(t->jobs.p, rj.data(), sizeof(OvlRedJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(t->tout.p, 0xff, sizeof(int) * row_ints, ctx->stream));   // poison: a row the tile kernel did not write leaves the job's output unwritten
    CK(hipMemsetAsync(t->out.p, 0xff, sizeof(int) * out_ints, ctx->stream));
    CK(hipMemsetAsync(t->top.p, 0xff, sizeof(int) * nj, ctx->stream));
    CnsSeqs SB{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
    if (S == 0) {
        ProfScope _ps(ctx, KID_OVERLAP_VOTE_TILE);
        hipLaunchKernelGGL(k_overlap_vote_tile, dim3((unsigned)nt), dim3(64), ovl_lds_bytes(P.list), ctx->stream, SB, (const OvlTileJob*)t->tjobs.p, (int)nt, P, TP,
                           (const unsigned*)t->codes.p, (const int*)t->gpos.p, (const long long*)t->off.p, (int*)t->tout.p);
    } else {
        ProfScope _ps(ctx, KID_OVERLAP_VOTE_TILE_MULTI);
        hipLaunchKernelGGL(k_overlap_vote_tile_multi, dim3((unsigned)nt), dim3(64), ovl_multi_lds_bytes(P.list), ctx->stream, SB, (const OvlTileJob*)t->tjobs.p, (int)nt, P, TP, S,
                           (const unsigned*)t->codes.p, (const int*)t->gpos.p, (const long long*)t->off.p, (int*)t->tout.p);
    }
    CK(hipGetLastError());
    if (S == 0) {
        ProfScope _ps(ctx, KID_OVERLAP_TILE_REDUCE);
        hipLaunchKernelGGL(k_overlap_tile_reduce, dim3((unsigned)nj), dim3(64), 0, ctx->stream, (const int*)t->tout.p, (const OvlRedJob*)t->jobs.p, (int)nj, P.max_partners, TP.part_top,
                           (int*)t->out.p, (int*)t->top.p);
    } else {
        ProfScope _ps(ctx, KID_OVERLAP_TILE_REDUCE_MULTI);
        hipLaunchKernelGGL(k_overlap_tile_reduce_multi, dim3((unsigned)nj), dim3(64), 0, ctx->stream, (const int*)t->tout.p, (const OvlRedJob*)t->jobs.p, (int)nj, P.max_partners,
                           TP.part_top, S, P.window, (int*)t->out.p, (int*)t->top.p);
    }
    CK(hipGetLastError());
    h_out.resize(out_ints);
    h_top.resize(nj);
    CK(hipMemcpyAsync(h_out.data(), t->out.p, sizeof(int) * out_ints, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_top.data(), t->top.p, sizeof(int) * nj, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    t->tstats[0] += (int64_t)nt;
    t->tstats[3]++;
    return HINGE_OK;
}

// hinge_overlap_run (S == 0: k_overlap_vote, one round) and hinge_overlap_run_multi (S = 1 .. 8 rounds of k_overlap_vote_multi).
// T > 0: hinge_overlap_run_tiled (S == 0) and hinge_overlap_run_tiled_multi (S = 1 .. 8) with tiles of T bases - other limits, the call's
// step for every read, batches by tile count.
static int overlap_run_impl(hinge_ctx* ctx, const hinge_overlap_params* params, int S, int T, int32_t* status, int32_t* hits, int64_t* n_out) {
    if (!ctx || !ctx->cns || !n_out || (ctx->cns->n_seq[0] > 0 && !status))
        return fail(ctx, HINGE_E_ARG, "hinge_overlap_run / _run_multi: bad arguments (call hinge_consensus_set_db with the read DB for both DBs first)");
    hinge_overlap_params q = params ? *params : hinge_overlap_params{0, 0, 0, 0, 0, 0, 0, 0};
    if (q.k == 0) q.k = (int32_t)seed_env("HINGE_OVERLAP_K", 15);
    if (q.step == 0) q.step = (int32_t)seed_env("HINGE_OVERLAP_STEP", 2);
    if (q.window == 0) q.window = (int32_t)seed_env("HINGE_OVERLAP_WINDOW", 256);
    if (q.max_occ == 0) q.max_occ = (int32_t)seed_env("HINGE_OVERLAP_MAX_OCC", HINGE_OVERLAP_MAX_OCC);
    if (q.list == 0) q.list = (int32_t)seed_env("HINGE_OVERLAP_LIST", 4096);
    if (q.max_partners == 0) q.max_partners = (int32_t)seed_env("HINGE_OVERLAP_MAX_PARTNERS", 64);
    if (q.min_hits == 0) q.min_hits = (int32_t)seed_env("HINGE_OVERLAP_MIN_HITS", HINGE_OVERLAP_MIN_HITS);
    if (q.block_bases == 0) q.block_bases = (int64_t)seed_env("HINGE_OVERLAP_BLOCK_BASES", 16ll << 20);
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (q.k < SEED_K_MIN || q.k > SEED_K_MAX || q.step < 1 || q.step > 65536 || !pow2(q.window) || q.window < SEED_WINDOW_MIN || q.window > SEED_WINDOW_MAX || q.max_occ < 1 ||
        q.max_occ > SEED_OCC_MAX || !pow2(q.list) || q.list < OVL_LIST_MIN || q.list > OVL_LIST_MAX || q.max_partners < 1 || q.max_partners > OVL_PARTNERS_MAX || q.min_hits < 1 ||
        q.block_bases < 1 || q.block_bases >= (1ll << 31))
        return fail(ctx, HINGE_E_ARG, "hinge_overlap_run / _run_multi: k 8..16, step 1..65536, window a power of two 16..65536, max_occ 1..256, list a power of two 64..8192, max_partners 1..4096, min_hits >= 1, block_bases 1..2^31-1 (0 = the default)");
    if (T > 0 && (!pow2(T) || T < OVT_TILE_MIN || T > OVT_TILE_MAX || (long long)T > (long long)q.list * q.step))
        return fail(ctx, HINGE_E_ARG, "hinge_overlap_run_tiled: tile a power of two 64..8192, at most list * step (0 = HINGE_OVERLAP_TILE, else 8192)");
    CnsState* s = ctx->cns;
    const int n = s->n_seq[0];
    if (s->n_seq[1] != n || s->h_rlen[1] != s->h_rlen[0]) return fail(ctx, HINGE_E_ARG, "hinge_overlap_run / _run_multi: both DBs of hinge_consensus_set_db must be the read DB");
    // ---- the limits of the key packing, before any launch; the blocks: consecutive reads of at most block_bases bases (a longer read: alone) -------------------
    std::vector<int> bfirst;                        // [n_blocks + 1]
    {
        long long bases = 0;
        int reads = 0;
        for (int r = 0; r < n; r++) {
            const int len = s->h_rlen[0][(size_t)r];
            if (T > 0 && len > OVT_READ_MAX) return fail(ctx, HINGE_E_CAPACITY, "hinge_overlap_run_tiled: a read of 2^30 or more bases (the hit key holds a diagonal in 31 bits)");
            if (T == 0 && len > OVL_READ_MAX) return fail(ctx, HINGE_E_CAPACITY, "hinge_overlap_run / _run_multi: a read of 2^20 or more bases (the hit key holds a position in 20 bits)");
            if (r == 0 || bases + len > q.block_bases || reads == (T > 0 ? OVT_BLOCK_READS_MAX : OVL_BLOCK_READS_MAX)) { bfirst.push_back(r); bases = 0; reads = 0; }
            bases += len; reads++;
            if (bases >= (1ll << 31)) return fail(ctx, HINGE_E_CAPACITY, "hinge_overlap_run / _run_multi: a block of 2^31 or more bases");
        }
        bfirst.push_back(n);
    }
    const int n_blocks = (int)bfirst.size() - 1;
    CK(hipSetDevice(ctx->device));
    if (!ctx->ovl_st) ctx->ovl_st = new OverlapState();
    OverlapState* t = ctx->ovl_st;
    for (int64_t& v : t->stats) v = 0;
    for (int64_t& v : t->tstats) v = 0;
    t->cand.clear();
    *n_out = 0;
    for (int r = 0; r < 2 * n; r++) { status[r] = OVL_ST_NONE; if (hits) hits[r] = 0; }
    if (n == 0) return HINGE_OK;
    const size_t lds = ovl_lds_bytes(q.list);
    if (T > 0 && S == 0 && lds > 48 * 1024) CK(hipFuncSetAttribute((const void*)k_overlap_vote_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (T > 0 && S > 0 && ovl_multi_lds_bytes(q.list) > 48 * 1024)
        CK(hipFuncSetAttribute((const void*)k_overlap_vote_tile_multi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovl_multi_lds_bytes(q.list)));
    if (S == 0 && T == 0 && lds > 48 * 1024) CK(hipFuncSetAttribute((const void*)k_overlap_vote, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (S > 0 && T == 0 && ovl_multi_lds_bytes(q.list) > 48 * 1024)
        CK(hipFuncSetAttribute((const void*)k_overlap_vote_multi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ovl_multi_lds_bytes(q.list)));
    OvlParams P;
    P.k = q.k; P.window = q.window; P.max_occ = q.max_occ; P.list = q.list; P.max_partners = q.max_partners; P.min_hits = q.min_hits;
    // ---- the jobs: two per read, the same for every block ------------------------------------------------------------------------------------
    std::vector<OvlJob> jobs((size_t)(2 * n));
    for (int a = 0; a < n; a++) {
        const int alen = s->h_rlen[0][(size_t)a];
        for (int comp = 0; comp < 2; comp++) jobs[(size_t)(2 * a + comp)] = OvlJob{a, comp, alen, alen >= q.k && T == 0 ? seed_stride(alen, q.k, q.step, q.list) : q.step};
    }
    // ---- tiles: every job's count (the same for every block); the jobs with more than one ----------------------------------------------------
    OvlTileParams TP;
    TP.step = q.step; TP.tile = T; TP.adv = T / 2; TP.part_top = 1;
    while (2 * TP.part_top <= q.max_partners) TP.part_top *= 2;
    std::vector<long long> n_tiles;
    if (T > 0) {
        n_tiles.resize((size_t)(2 * n));
        for (size_t j = 0; j < n_tiles.size(); j++) n_tiles[j] = ovl_tile_count(jobs[j].alen, q.k, T);
    }
    std::vector<OvlTileJob> tj;
    std::vector<OvlRedJob> rj;
    std::vector<int> h_top;
    long long budget = std::max(1ll, seed_env("HINGE_OVERLAP_SCRATCH_MB", 256)) << 20;
    budget = std::max(1ll, seed_env("HINGE_OVERLAP_SCRATCH_BYTES", budget));
    const int W = S ? ovl_multi_out_ints(q.max_partners, S) : ovl_out_ints(q.max_partners);       // (a job of S rounds is S times as wide: batches shrink)
    const int rounds = std::max(S, 1), head = OVL_HEAD + S;
    const long long per_job = (long long)sizeof(OvlJob) + (long long)sizeof(int) * W;
    const int64_t per_batch = std::min<long long>(std::max<long long>(budget / per_job, 1), 1 << 20);
    const long long per_tile = (long long)sizeof(OvlTileJob) + (long long)sizeof(int) * W;       // tiled: a batch's jobs by their tiles; a job's tiles stay together
    const long long per_red = (long long)sizeof(OvlRedJob) + (long long)sizeof(int) * (W + 1);
    std::vector<int> h_out;
    std::vector<long long> ix_off;
    int rc;
    index_stats_reset(ctx);
    for (int blk = 0; blk < n_blocks; blk++) {
        // ---- the block's index (index_capi.inc): on the device from the resident bases, or on the host and up ----------------------------------------------------
        const int first = bfirst[(size_t)blk], nr = bfirst[(size_t)blk + 1] - first;
        int64_t ne64 = 0, ix_dropped = 0;
        if ((rc = index_build(ctx, first, nr, q.k, q.max_occ, -1, t->codes, t->gpos, t->off, ix_off, &ne64, &ix_dropped))) return rc;
        const size_t ne = (size_t)ne64;
        t->stats[2]++;
        t->stats[3] += (int64_t)ne;
        t->stats[4] += ix_dropped;
        t->stats[7] = ctx->idx_st->stats[6];
        P.n_entries = (int)ne;
        P.search_top = 0;
        for (long long v = 1; v <= (long long)ne; v <<= 1) P.search_top = (int)v;      // the searches' trip counts: fixed here, from the block
        P.first = first; P.n_reads = nr;
        P.read_top = 0;
        for (long long v = 1; v <= (long long)nr; v <<= 1) P.read_top = (int)v;
        // ---- every job against it, in batches under the scratch budget -------------------------------------------------------------------------------
        for (int64_t j0 = 0, j1 = 0; j0 < 2 * (int64_t)n; j0 = j1) {
            j1 = std::min<int64_t>(2 * (int64_t)n, j0 + per_batch);
            if (T > 0) {                                                    // as many whole jobs as the budget holds; one at the least
                long long bytes = 0, tiles = 0;
                for (j1 = j0; j1 < 2 * (int64_t)n; j1++) {
                    const long long nt = n_tiles[(size_t)j1];
                    if (j1 > j0 && (bytes + nt * per_tile + per_red > budget || tiles + nt > (1 << 20) || j1 - j0 == (1 << 20))) break;
                    bytes += nt * per_tile + per_red; tiles += nt;
                }
                if (tiles > 0x7fffffffll / W) return fail(ctx, HINGE_E_CAPACITY, "hinge_overlap_run_tiled: one read's tile rows beyond 2^31 ints (a larger tile, or fewer max_partners)");
                if ((rc = overlap_batch_tiled(ctx, jobs.data() + j0, (size_t)(j1 - j0), P, TP, S, tj, rj, h_out, h_top))) return rc;
            } else if ((rc = overlap_batch(ctx, jobs.data() + j0, (size_t)(j1 - j0), P, S, h_out))) return rc;
            t->stats[0] += j1 - j0;
            t->stats[1]++;
            for (int64_t j = j0; j < j1; j++) {
                const int* o = h_out.data() + (size_t)(j - j0) * (size_t)W;
                const OvlJob& J = jobs[(size_t)j];
                const bool st_ok = o[0] == OVL_ST_OK || o[0] == OVL_ST_NONE || o[0] == OVL_ST_OVERFLOW || o[0] == OVL_ST_TRUNCATED || o[0] == (OVL_ST_OVERFLOW | OVL_ST_TRUNCATED);
                int round_sum = S ? 0 : o[1];                               // the head of S rounds: the number written in each
                bool rounds_ok = true;
                for (int r = 0; r < S; r++) {
                    if (o[OVL_HEAD + r] < 0 || o[OVL_HEAD + r] > q.max_partners || (r > 0 && o[OVL_HEAD + r] > 0 && o[OVL_HEAD + r - 1] == 0)) rounds_ok = false;
                    round_sum += o[OVL_HEAD + r];
                }
                const long long hits_max = T > 0 ? std::min<long long>(n_tiles[(size_t)j] * q.list, 0x7fffffffll) : q.list;      // tiled: the sum of the tiles' lists
                if (T > 0) {
                    const int top = h_top[(size_t)(j - j0)];
                    if (top < 0 || top > q.list || top > o[2]) return fail(ctx, HINGE_E_DEVICE, "hinge_overlap_run_tiled: a job's reduce slot was never written");
                    t->tstats[2] = std::max<int64_t>(t->tstats[2], top);
                    if (n_tiles[(size_t)j] > 1) t->tstats[1]++;
                }
                if (!st_ok || !rounds_ok || round_sum != o[1] || o[1] < 0 || o[1] > rounds * q.max_partners || o[2] < 0 || o[2] > hits_max || (o[1] > 0 && (o[2] < 1 || o[0] == OVL_ST_NONE)) || o[3] != 0)
                    return fail(ctx, HINGE_E_DEVICE, "hinge_overlap_run / _run_multi: a job's status slot was never written");
                if (hits) hits[j] += o[2];
                if (o[0] != OVL_ST_NONE) status[j] = (status[j] == OVL_ST_NONE ? 0 : status[j]) | o[0];
                if (o[0] != OVL_ST_NONE && (o[0] & OVL_ST_OVERFLOW)) t->stats[5]++;
                if (o[0] != OVL_ST_NONE && (o[0] & OVL_ST_TRUNCATED)) t->stats[6]++;
                for (int x = 0, r = 0, c0 = 0; x < o[1]; x++) {                    // the x-th candidate: slot c of section r
                    while (S && x - c0 == o[OVL_HEAD + r]) { c0 = x; r++; }   // (the sections' counts sum to o[1]: checked above)
                    const int c = x - c0;
                    const int* pk = o + head + 4 * (r * q.max_partners + c);
                    const int b = pk[0];
                    const bool b_ok = b >= first && b < first + nr && b != J.a;
                    const int blen = b_ok ? s->h_rlen[0][(size_t)b] : 0;
                    OverlapCand oc;
                    if (!b_ok || pk[1] < q.min_hits || pk[1] > o[2] || pk[2] < 1 || pk[2] >= J.alen + blen || pk[3] < 0 || pk[3] > J.alen - q.k ||
                        !overlap_project(J.alen, blen, J.comp, pk[2], q.k, &oc.r.abpos, &oc.r.aepos, &oc.r.bbpos, &oc.r.bepos, &oc.diag))
                        return fail(ctx, HINGE_E_DEVICE, "hinge_overlap_run / _run_multi: a candidate's slot was never written");
                    oc.r.aread = J.a; oc.r.bread = b; oc.r.comp = J.comp; oc.r.tlen = 0; oc.r.trace_off = 0;
                    oc.cnt = pk[1]; oc.d = pk[2]; oc.p = pk[3]; oc.round = r;
                    t->cand.push_back(oc);
                }
            }
        }
    }
    std::sort(t->cand.begin(), t->cand.end(), [](const OverlapCand& u, const OverlapCand& v) {
        if (u.r.aread != v.r.aread) return u.r.aread < v.r.aread;
        if (u.r.bread != v.r.bread) return u.r.bread < v.r.bread;
        if (u.r.comp != v.r.comp) return u.r.comp < v.r.comp;
        return u.round < v.round;
    });
    *n_out = (int64_t)t->cand.size();
    return HINGE_OK;
}

extern "C" {

int hinge_overlap_run(hinge_ctx* ctx, const hinge_overlap_params* params, int32_t* status, int32_t* hits, int64_t* n_out) {
    return overlap_run_impl(ctx, params, 0, 0, status, hits, n_out);
}

int hinge_overlap_run_multi(hinge_ctx* ctx, const hinge_overlap_params* params, int32_t max_stretches, int32_t* status, int32_t* hits, int64_t* n_out) {
    if (max_stretches == 0) max_stretches = (int32_t)seed_env("HINGE_OVERLAP_MAX_STRETCHES", 1);
    if (max_stretches < 1 || max_stretches > OVL_STRETCHES_MAX) return fail(ctx, HINGE_E_ARG, "hinge_overlap_run_multi: max_stretches 1..8 (0 = HINGE_OVERLAP_MAX_STRETCHES, else 1)");
    return overlap_run_impl(ctx, params, max_stretches, 0, status, hits, n_out);
}

int hinge_overlap_run_tiled(hinge_ctx* ctx, const hinge_overlap_params* params, int32_t tile, int32_t* status, int32_t* hits, int64_t* n_out) {
    if (tile == 0) tile = (int32_t)seed_env("HINGE_OVERLAP_TILE", HINGE_OVERLAP_TILE_MAX);
    if (tile < 1) return fail(ctx, HINGE_E_ARG, "hinge_overlap_run_tiled: tile a power of two 64..8192, at most list * step (0 = HINGE_OVERLAP_TILE, else 8192)");
    return overlap_run_impl(ctx, params, 0, tile, status, hits, n_out);
}

int hinge_overlap_run_tiled_multi(hinge_ctx* ctx, const hinge_overlap_params* params, int32_t tile, int32_t max_stretches, int32_t* status, int32_t* hits, int64_t* n_out) {
    if (tile == 0) tile = (int32_t)seed_env("HINGE_OVERLAP_TILE", HINGE_OVERLAP_TILE_MAX);
    if (tile < 1) return fail(ctx, HINGE_E_ARG, "hinge_overlap_run_tiled_multi: tile a power of two 64..8192, at most list * step (0 = HINGE_OVERLAP_TILE, else 8192)");
    if (max_stretches == 0) max_stretches = (int32_t)seed_env("HINGE_OVERLAP_TILE_STRETCHES", 1);
    if (max_stretches < 1 || max_stretches > OVL_STRETCHES_MAX)
        return fail(ctx, HINGE_E_ARG, "hinge_overlap_run_tiled_multi: max_stretches 1..8 (0 = HINGE_OVERLAP_TILE_STRETCHES, else 1)");
    return overlap_run_impl(ctx, params, max_stretches, tile, status, hits, n_out);
}

int hinge_overlap_tile_stats(hinge_ctx* ctx, int64_t* out) {
    if (!ctx || !ctx->ovl_st || !out) return fail(ctx, HINGE_E_ARG, "hinge_overlap_tile_stats: no hinge_overlap_run yet");
    for (int k = 0; k < 4; k++) out[k] = ctx->ovl_st->tstats[k];
    return HINGE_OK;
}

int hinge_overlap_fetch_round(hinge_ctx* ctx, int64_t cap, int32_t* round) {
    if (!ctx || !ctx->ovl_st || cap < 0 || (cap > 0 && !round)) return fail(ctx, HINGE_E_ARG, "hinge_overlap_fetch_round: no hinge_overlap_run yet, or bad arguments");
    const std::vector<OverlapCand>& c = ctx->ovl_st->cand;
    if ((int64_t)c.size() > cap) return fail(ctx, HINGE_E_CAPACITY, "hinge_overlap_fetch_round: the output array must hold what the run counted");
    for (size_t x = 0; x < c.size(); x++) round[x] = c[x].round;
    return HINGE_OK;
}

int hinge_overlap_fetch(hinge_ctx* ctx, int64_t cap, hinge_cns_alignment* out, int32_t* count, int32_t* diag, int32_t* rep) {
    if (!ctx || !ctx->ovl_st || cap < 0 || (cap > 0 && (!out || !count || !diag))) return fail(ctx, HINGE_E_ARG, "hinge_overlap_fetch: no hinge_overlap_run yet, or bad arguments");
    const std::vector<OverlapCand>& c = ctx->ovl_st->cand;
    if ((int64_t)c.size() > cap) return fail(ctx, HINGE_E_CAPACITY, "hinge_overlap_fetch: the output arrays must hold what hinge_overlap_run counted");
    for (size_t x = 0; x < c.size(); x++) {
        out[x] = c[x].r; count[x] = c[x].cnt; diag[x] = c[x].diag;
        if (rep) { rep[2 * x] = c[x].d; rep[2 * x + 1] = c[x].p; }
    }
    return HINGE_OK;
}

int hinge_overlap_last_stats(hinge_ctx* ctx, int64_t* out) {
    if (!ctx || !ctx->ovl_st || !out) return fail(ctx, HINGE_E_ARG, "hinge_overlap_last_stats: no hinge_overlap_run yet");
    for (int k = 0; k < 8; k++) out[k] = ctx->ovl_st->stats[k];
    return HINGE_OK;
}

}  // extern "C"
