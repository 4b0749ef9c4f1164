// C ABI of `hinge seed` (include/hinge_hip.h, "hinge seed").  Included by hinge_capi.hip.
// Host work here: the parameters' defaults and ranges, the call of the draft's k-mer index (index_capi.inc: built on the device from
// the resident bases, or by seed_index.h from the host copy hinge_consensus_set_db keeps), the jobs (two per read) in batches under the scratch
// budget, the launches, a pick's projection onto its contig (seed_project) and the order of a read's placements.  The kernel:
// seed_kernels.h.
struct SeedState {
    DevBuf jobs, out, codes, gpos, off;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hinge_seed_last_stats
};

static void seed_release(hinge_ctx* ctx) {
    SeedState* t = ctx->seed_st;
    if (!t) return;
    DevBuf* all[] = {&t->jobs, &t->out, &t->codes, &t->gpos, &t->off};
    for (DevBuf* b : all) release(*b);
    delete t;
    ctx->seed_st = nullptr;
}

static long long seed_env(const char* name, long long def) {
    const char* g = getenv(name);
    return (g && *g) ? atoll(g) : def;
}

// One batch: jobs[0..nj) through k_seed_vote; h_out = seed_out_ints(n_max) ints per job.
static int seed_batch(hinge_ctx* ctx, const std::vector<SeedJob>& jobs, const SeedParams& P, std::vector<int>& h_out) {
    SeedState* t = ctx->seed_st;
    CnsState* s = ctx->cns;
    const size_t nj = jobs.size(), out_ints = nj * (size_t)seed_out_ints(P.n_max);
    int rc;
    if ((rc = ensure(ctx, t->jobs, sizeof(SeedJob) * nj))) return rc;
    if ((rc = ensure(ctx, t->out, sizeof(int) * out_ints))) return rc;
    CK(hipMemcpyAsync(t->jobs.p, jobs.data(), sizeof(SeedJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(t->out.p, 0xff, sizeof(int) * out_ints, ctx->stream));   // poison: a slot the kernel did not write is seen as such
    CnsSeqs SB{(const unsigned char*)s->bps[1].p, (const long long*)s->boff[1].p, (const int*)s->rlen[1].p};
    {
        ProfScope _ps(ctx, KID_SEED_VOTE);
        hipLaunchKernelGGL(k_seed_vote, dim3((unsigned)nj), dim3(64), seed_lds_bytes(P.list), ctx->stream, SB, (const SeedJob*)t->jobs.p, (int)nj, P, (const unsigned*)t->codes.p,
                           (const int*)t->gpos.p, (int*)t->out.p);
    }
    CK(hipGetLastError());
    h_out.resize(out_ints);
    CK(hipMemcpyAsync(h_out.data(), t->out.p, sizeof(int) * out_ints, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return HINGE_OK;
}

extern "C" {

int hinge_seed_run(hinge_ctx* ctx, const hinge_seed_params* params, int64_t n_reads, const int32_t* read_ids, int64_t cap, hinge_cns_alignment* out, int32_t* count, int32_t* diag,
                   int32_t* n_placed, int32_t* status, int64_t* n_out) {
    if (!ctx || !ctx->cns || n_reads < -1 || (n_reads == -1 && read_ids) || cap < 0 || !n_out || (n_reads != 0 && (!n_placed || !status)) || (cap > 0 && (!out || !count || !diag)))
        return fail(ctx, HINGE_E_ARG, "hinge_seed_run: bad arguments (call hinge_consensus_set_db for both DBs first)");
    hinge_seed_params q = params ? *params : hinge_seed_params{0, 0, 0, 0, 0, 0, 0};
    if (q.k == 0) q.k = (int32_t)seed_env("HINGE_SEED_K", 15);
    if (q.step == 0) q.step = (int32_t)seed_env("HINGE_SEED_STEP", 2);
    if (q.window == 0) q.window = (int32_t)seed_env("HINGE_SEED_WINDOW", 256);
    if (q.max_occ == 0) q.max_occ = (int32_t)seed_env("HINGE_SEED_MAX_OCC", 16);
    if (q.list == 0) q.list = (int32_t)seed_env("HINGE_SEED_LIST", 2048);
    if (q.max_placements == 0) q.max_placements = (int32_t)seed_env("HINGE_SEED_MAX_PLACEMENTS", 1);
    if (q.min_hits == 0) q.min_hits = (int32_t)seed_env("HINGE_SEED_MIN_HITS", HINGE_SEED_MIN_HITS);
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (q.k < SEED_K_MIN || q.k > SEED_K_MAX || q.step < 1 || q.step > 65536 || !pow2(q.window) || q.window < SEED_WINDOW_MIN || q.window > SEED_WINDOW_MAX || q.max_occ < 1 ||
        q.max_occ > SEED_OCC_MAX || !pow2(q.list) || q.list < SEED_LIST_MIN || q.list > SEED_LIST_MAX || q.max_placements < 1 || q.max_placements > SEED_N_MAX || q.min_hits < 1)
        return fail(ctx, HINGE_E_ARG, "hinge_seed_run: k 8..16, step 1..65536, window a power of two 16..65536, max_occ 1..256, list a power of two 64..4096, max_placements 1..8, min_hits >= 1 (0 = the default)");
    CnsState* s = ctx->cns;
    const int n_contigs = s->n_seq[0], n_db = s->n_seq[1], N = q.max_placements;
    if (n_reads == -1) n_reads = n_db;
    if (!read_ids && n_reads != n_db) return fail(ctx, HINGE_E_ARG, "hinge_seed_run: without read ids, n_reads must be -1 or the read DB's count");
    for (int64_t x = 0; read_ids && x < n_reads; x++)
        if (read_ids[x] < 0 || read_ids[x] >= n_db) return fail(ctx, HINGE_E_RANGE, "hinge_seed_run: read id outside the read DB");
    long long total = 0;
    for (int c = 0; c < n_contigs; c++) total += s->h_rlen[0][(size_t)c];
    if (total >= (1ll << 31)) return fail(ctx, HINGE_E_CAPACITY, "hinge_seed_run: a draft of 2^31 or more bases");
    if (n_reads * N > cap) return fail(ctx, HINGE_E_CAPACITY, "hinge_seed_run: the output arrays must hold max_placements records per read");
    CK(hipSetDevice(ctx->device));
    if (!ctx->seed_st) ctx->seed_st = new SeedState();
    SeedState* t = ctx->seed_st;
    for (int64_t& v : t->stats) v = 0;
    *n_out = 0;
    // ---- the index (index_capi.inc): on the device from the resident bases, or on the host and up -----------------------------------------------------------
    std::vector<long long> ix_off;
    int64_t ne64 = 0, ix_dropped = 0;
    int rc;
    index_stats_reset(ctx);
    if ((rc = index_build(ctx, 0, n_contigs, q.k, q.max_occ, -1, t->codes, t->gpos, t->off, ix_off, &ne64, &ix_dropped))) return rc;
    const size_t ne = (size_t)ne64;
    t->stats[2] = (int64_t)ne;
    t->stats[3] = ix_dropped;
    t->stats[6] = ctx->idx_st->stats[6];
    SeedParams P;
    P.k = q.k; P.window = q.window; P.max_occ = q.max_occ; P.list = q.list; P.n_max = N; P.min_hits = q.min_hits;
    P.n_entries = (int)ne;
    P.search_top = 0;
    for (long long v = 1; v <= (long long)ne; v <<= 1) P.search_top = (int)v;     // the search's trip count: fixed here, from the index size
    // ---- the jobs, in batches under the scratch budget ----------------------------------------------------------------------------------
    long long budget = std::max(1ll, seed_env("HINGE_SEED_SCRATCH_MB", 256)) << 20;
    budget = std::max(1ll, seed_env("HINGE_SEED_SCRATCH_BYTES", budget));
    const int W = seed_out_ints(N);
    const long long per_job = (long long)sizeof(SeedJob) + (long long)sizeof(int) * W;
    const int64_t per_batch = std::min<long long>(std::max<long long>(budget / per_job, 2), 1 << 20) & ~1ll;   // whole reads: both strands in one batch
    std::vector<SeedJob> jobs;
    std::vector<int> h_out;
    struct Cand { int cnt, comp; unsigned d; int p, gpos; };
    std::vector<Cand> cand;
    int64_t n_total = 0;
    for (int64_t r0 = 0; r0 < n_reads; r0 += per_batch / 2) {
        const int64_t r1 = std::min<int64_t>(n_reads, r0 + per_batch / 2);
        jobs.clear();
        for (int64_t x = r0; x < r1; x++) {
            const int b = read_ids ? read_ids[x] : (int)x, blen = s->h_rlen[1][(size_t)b];
            for (int comp = 0; comp < 2; comp++) jobs.push_back(SeedJob{b, comp, blen, blen >= q.k ? seed_stride(blen, q.k, q.step, q.list) : q.step});
        }
        if ((rc = seed_batch(ctx, jobs, P, h_out))) return rc;
        t->stats[0] += (int64_t)jobs.size();
        t->stats[1]++;
        for (int64_t x = r0; x < r1; x++) {
            cand.clear();
            const int b = jobs[(size_t)(2 * (x - r0))].b, blen = jobs[(size_t)(2 * (x - r0))].blen;
            for (int comp = 0; comp < 2; comp++) {
                const int* o = h_out.data() + (size_t)(2 * (x - r0) + comp) * (size_t)W;
                if (o[0] < SEED_ST_OK || o[0] > SEED_ST_OVERFLOW || o[1] < 0 || o[1] > N || o[2] < 0 || o[2] > q.list || (o[1] > 0 && o[2] < 1) || o[3] != 0) return fail(ctx, HINGE_E_DEVICE, "hinge_seed_run: a job's status slot was never written");
                status[2 * x + comp] = o[0];
                if (o[0] == SEED_ST_OVERFLOW) t->stats[4]++;
                for (int k = 0; k < o[1]; k++) {
                    const int* pk = o + SEED_HEAD + 4 * k;
                    if (pk[0] < 1 || pk[0] > o[2] || pk[2] < 0 || pk[3] < 0 || (long long)pk[3] >= total || (long long)(unsigned)pk[1] != (long long)pk[3] - pk[2] + blen) return fail(ctx, HINGE_E_DEVICE, "hinge_seed_run: a pick's slot was never written");
                    cand.push_back(Cand{pk[0], comp, (unsigned)pk[1], pk[2], pk[3]});
                }
            }
            // a read's placements: by count descending, forward before complement, d ascending; the first N that project onto their contig
            std::sort(cand.begin(), cand.end(), [](const Cand& u, const Cand& v) {
                if (u.cnt != v.cnt) return u.cnt > v.cnt;
                if (u.comp != v.comp) return u.comp < v.comp;
                return u.d < v.d;
            });
            int placed = 0;
            for (const Cand& c : cand) {
                if (placed == N) break;
                int a, ab, ae, bb, be;
                if (!seed_project(ix_off.data(), n_contigs, q.k, c.gpos, c.p, blen, &a, &ab, &ae, &bb, &be)) continue;
                hinge_cns_alignment& o = out[n_total];
                o.aread = a; o.bread = b; o.comp = c.comp; o.abpos = ab; o.aepos = ae; o.bbpos = bb; o.bepos = be; o.tlen = 0; o.trace_off = 0;
                count[n_total] = c.cnt;
                diag[n_total] = c.gpos - c.p;
                n_total++; placed++;
            }
            n_placed[x] = placed;
            if (!placed) t->stats[5]++;
        }
    }
    *n_out = n_total;
    return HINGE_OK;
}

int hinge_seed_db_reads(hinge_ctx* ctx, int64_t* n_reads) {
    if (!ctx || !ctx->cns || !n_reads) return fail(ctx, HINGE_E_ARG, "hinge_seed_db_reads: call hinge_consensus_set_db first");
    *n_reads = ctx->cns->n_seq[1];
    return HINGE_OK;
}

int hinge_seed_last_stats(hinge_ctx* ctx, int64_t* out) {
    if (!ctx || !ctx->seed_st || !out) return fail(ctx, HINGE_E_ARG, "hinge_seed_last_stats: no hinge_seed_run yet");
    for (int k = 0; k < 8; k++) out[k] = ctx->seed_st->stats[k];
    return HINGE_OK;
}

}  // extern "C"
