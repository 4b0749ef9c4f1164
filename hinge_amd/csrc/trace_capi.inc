// C ABI of `hinge paf2las` (include/hinge_hip.h, "hinge paf2las").  Included by hinge_capi.hip.
// Host work here: range checks, the widening rounds (W, 2 W, ... while it stays within band_max: four with the defaults, never more
// than TRACE_ROUNDS = the doublings from the smallest to the largest legal band), the batches of one
// round under the direction-scratch budget, the launches, the results back in the caller's order.  The kernels: trace_kernels.h.
constexpr int TRACE_ROUNDS = 9;

struct TraceState {
    DevBuf jobs, dirs, trace, status, diffs, cost;
    size_t lds_attr = 0;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hinge_trace_last_stats
};

static void trace_release(hinge_ctx* ctx) {
    TraceState* t = ctx->trace_st;
    if (!t) return;
    DevBuf* all[] = {&t->jobs, &t->dirs, &t->trace, &t->status, &t->diffs, &t->cost};
    for (DevBuf* b : all) release(*b);
    delete t;
    ctx->trace_st = nullptr;
}

static long long trace_env(const char* name, long long def) {
    const char* g = getenv(name);
    return (g && *g) ? atoll(g) : def;
}

// One batch: jobs[0..nj) (dir_off / trace_off laid out by the caller) at half-width W.  Results to the host vectors.
static int trace_batch(hinge_ctx* ctx, const std::vector<TraceJob>& jobs, long long dir_words, long long n_vals, int W, int tspace, std::vector<unsigned short>& h_trace,
                       std::vector<int>& h_status, std::vector<int>& h_diffs) {
    TraceState* t = ctx->trace_st;
    CnsState* s = ctx->cns;
    const size_t nj = jobs.size();
    int rc;
    if ((rc = ensure(ctx, t->jobs, sizeof(TraceJob) * nj))) return rc;
    if ((rc = ensure(ctx, t->dirs, sizeof(unsigned) * (size_t)std::max<long long>(dir_words, 1)))) return rc;
    if ((rc = ensure(ctx, t->trace, sizeof(unsigned short) * (size_t)std::max<long long>(n_vals, 1)))) return rc;
    if ((rc = ensure(ctx, t->status, sizeof(int) * nj))) return rc;
    if ((rc = ensure(ctx, t->diffs, sizeof(int) * nj))) return rc;
    if ((rc = ensure(ctx, t->cost, sizeof(int) * nj))) return rc;
    CK(hipMemcpyAsync(t->jobs.p, jobs.data(), sizeof(TraceJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    // poison: a slot no kernel wrote is seen as such, never as data (0xff bytes: status / diffs / cost -1, trace 0xffff)
    CK(hipMemsetAsync(t->trace.p, 0xff, sizeof(unsigned short) * (size_t)std::max<long long>(n_vals, 1), ctx->stream));
    CK(hipMemsetAsync(t->status.p, 0xff, sizeof(int) * nj, ctx->stream));
    CK(hipMemsetAsync(t->diffs.p, 0xff, sizeof(int) * nj, ctx->stream));
    CK(hipMemsetAsync(t->cost.p, 0xff, sizeof(int) * nj, ctx->stream));
    const size_t lds = trace_lds_bytes(W);
    if (lds > 48 * 1024 && lds > t->lds_attr) {
        CK(hipFuncSetAttribute((const void*)k_trace_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        t->lds_attr = lds;
    }
    CnsSeqs SA{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
    CnsSeqs SB{(const unsigned char*)s->bps[1].p, (const long long*)s->boff[1].p, (const int*)s->rlen[1].p};
    {
        ProfScope _ps(ctx, KID_TRACE_FILL);
        hipLaunchKernelGGL(k_trace_fill, dim3((unsigned)nj), dim3(64), lds, ctx->stream, SA, SB, (const TraceJob*)t->jobs.p, (int)nj, W, (unsigned*)t->dirs.p, (int*)t->cost.p);
    }
    {
        ProfScope _ps(ctx, KID_TRACE_WALK);
        hipLaunchKernelGGL(k_trace_walk, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, ctx->stream, (const TraceJob*)t->jobs.p, (int)nj, W, tspace, tspace <= 125 ? 255 : 65534,
                           (const unsigned*)t->dirs.p, (const int*)t->cost.p, (unsigned short*)t->trace.p, (int*)t->diffs.p, (int*)t->status.p);
    }
    CK(hipGetLastError());
    h_trace.resize((size_t)std::max<long long>(n_vals, 1));
    h_status.resize(nj);
    h_diffs.resize(nj);
    if (n_vals) CK(hipMemcpyAsync(h_trace.data(), t->trace.p, sizeof(unsigned short) * (size_t)n_vals, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_status.data(), t->status.p, sizeof(int) * nj, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_diffs.data(), t->diffs.p, sizeof(int) * nj, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return HINGE_OK;
}

extern "C" {

int hinge_trace_run(hinge_ctx* ctx, int64_t n, const hinge_cns_alignment* placements, int32_t tspace, int32_t band, int32_t band_max, hinge_cns_alignment* out_alns,
                    uint16_t* trace, int64_t trace_cap, int64_t* n_trace, int32_t* diffs, int32_t* status) {
    if (!ctx || !ctx->cns || n < 0 || (n > 0 && (!placements || !out_alns || !diffs || !status)) || !n_trace || trace_cap < 0 || (trace_cap > 0 && !trace) || tspace <= 0 || tspace > 32767)
        return fail(ctx, HINGE_E_ARG, "hinge_trace_run: bad arguments (call hinge_consensus_set_db for both DBs first)");
    if (band <= 0) band = (int32_t)trace_env("HINGE_TRACE_BAND", 128);
    if (band_max <= 0) band_max = (int32_t)std::max<long long>(trace_env("HINGE_TRACE_BAND_MAX", 1024), band);
    if (band < TRACE_BAND_MIN || (band % 8) != 0 || band_max < band || band_max > TRACE_BAND_LIMIT)
        return fail(ctx, HINGE_E_ARG, "hinge_trace_run: the band must be a multiple of 8 from 8 to 2048, and band_max no smaller");
    CnsState* s = ctx->cns;
    CK(hipSetDevice(ctx->device));
    if (!ctx->trace_st) ctx->trace_st = new TraceState();
    TraceState* t = ctx->trace_st;
    for (int64_t& v : t->stats) v = 0;
    *n_trace = 0;
    // ---- range checks, the segments of every placement: all before any launch ---------------------------------------------------
    std::vector<int> nseg((size_t)n);
    int64_t all_vals = 0;
    for (int64_t x = 0; x < n; x++) {
        const hinge_cns_alignment& r = placements[x];
        if (r.aread < 0 || r.aread >= s->n_seq[0] || r.bread < 0 || r.bread >= s->n_seq[1]) return fail(ctx, HINGE_E_RANGE, "hinge_trace_run: read id outside its DB");
        const int alen = s->h_rlen[0][(size_t)r.aread], blen = s->h_rlen[1][(size_t)r.bread];
        if (!(0 <= r.abpos && r.abpos < r.aepos && r.aepos <= alen && 0 <= r.bbpos && r.bbpos < r.bepos && r.bepos <= blen))
            return fail(ctx, HINGE_E_RANGE, "hinge_trace_run: placement coordinates outside their reads, or an empty stretch");
        nseg[(size_t)x] = trace_segments(r.abpos, r.aepos, tspace);
        all_vals += 2 * (int64_t)nseg[(size_t)x];
    }
    if (all_vals > trace_cap) return fail(ctx, HINGE_E_CAPACITY, "hinge_trace_run: the trace array must hold two values per trace-point segment of every placement");
    long long budget = std::max(1ll, trace_env("HINGE_TRACE_SCRATCH_MB", 4096)) << 20;
    budget = std::max(1ll, trace_env("HINGE_TRACE_SCRATCH_BYTES", budget));
    // ---- the rounds ---------------------------------------------------------------------------------------------------------------
    std::vector<int> st((size_t)n, TRACE_ST_POISON), fw((size_t)n, 0), df((size_t)n, 0);
    std::vector<std::vector<unsigned short>> tr((size_t)n);
    std::vector<int64_t> pending((size_t)n), next;
    for (int64_t x = 0; x < n; x++) pending[(size_t)x] = x;
    std::vector<TraceJob> jobs;
    std::vector<int64_t> job_of;
    std::vector<unsigned short> h_trace;
    std::vector<int> h_status, h_diffs;
    int W = band;
    for (int round = 0; round < TRACE_ROUNDS && !pending.empty(); round++) {
        t->stats[3] = round + 1;
        next.clear();
        const bool last = round + 1 == TRACE_ROUNDS || 2ll * W > band_max;   // (8 * 2^8 = 2048: the first clause never decides)
        size_t at = 0;
        while (at < pending.size()) {
            // one batch: placements whose direction scratch (alen x 2 W x 2 bits each) fits the budget; at least one
            jobs.clear(); job_of.clear();
            long long words = 0, vals = 0;
            for (; at < pending.size() && jobs.size() < (size_t)(1 << 20); at++) {
                const int64_t x = pending[at];
                const hinge_cns_alignment& r = placements[x];
                const int alen = r.aepos - r.abpos, blen = r.bepos - r.bbpos;
                fw[(size_t)x] = W;
                if (std::abs(blen - alen) > W) {          // decided from the coordinates alone
                    st[(size_t)x] = TRACE_ST_NO_PATH;
                    if (!last) next.push_back(x);
                    continue;
                }
                const long long w = trace_dir_words(alen, W);
                if (!jobs.empty() && (words + w) * (long long)sizeof(unsigned) > budget) break;
                TraceJob j;
                j.a = r.aread; j.b = r.bread; j.comp = r.comp ? 1 : 0; j.ab = r.abpos; j.ae = r.aepos; j.bb = r.bbpos; j.be = r.bepos;
                j.blen = s->h_rlen[1][(size_t)r.bread]; j.nseg = nseg[(size_t)x]; j.pad = 0; j.dir_off = words; j.trace_off = vals;
                words += w; vals += 2ll * j.nseg;
                jobs.push_back(j); job_of.push_back(x);
            }
            if (jobs.empty()) continue;
            int rc;
            if ((rc = trace_batch(ctx, jobs, words, vals, W, tspace, h_trace, h_status, h_diffs))) return rc;
            t->stats[0]++;
            t->stats[1] = std::max<int64_t>(t->stats[1], words * (int64_t)sizeof(unsigned));
            t->stats[2] += (int64_t)jobs.size();
            for (size_t k = 0; k < jobs.size(); k++) {
                const int64_t x = job_of[k];
                const int code = h_status[k];
                if (code < TRACE_ST_OK || code > TRACE_ST_STEPS) return fail(ctx, HINGE_E_DEVICE, "hinge_trace_run: a placement's status slot was never written");
                st[(size_t)x] = code; df[(size_t)x] = h_diffs[k];
                if (code == TRACE_ST_OK) {
                    const unsigned short* p = h_trace.data() + jobs[k].trace_off;
                    tr[(size_t)x].assign(p, p + 2 * jobs[k].nseg);
                    for (unsigned short v : tr[(size_t)x]) if (v == TRACE_POISON16) return fail(ctx, HINGE_E_DEVICE, "hinge_trace_run: a trace slot was never written");
                } else if ((code == TRACE_ST_TOUCHED || code == TRACE_ST_NO_PATH) && !last) next.push_back(x);
            }
        }
        std::sort(next.begin(), next.end());
        pending.swap(next);
        if (last) break;
        W *= 2;
    }
    // ---- results in the caller's order ------------------------------------------------------------------------------------------------
    int64_t off = 0;
    for (int64_t x = 0; x < n; x++) {
        hinge_cns_alignment o = placements[x];
        o.trace_off = off; o.tlen = 0;
        if (st[(size_t)x] == TRACE_ST_OK) {
            o.tlen = (int32_t)tr[(size_t)x].size();
            memcpy(trace + off, tr[(size_t)x].data(), sizeof(uint16_t) * tr[(size_t)x].size());
            off += o.tlen;
            if (fw[(size_t)x] != band) t->stats[4]++;
        } else t->stats[5]++;
        out_alns[x] = o;
        diffs[x] = st[(size_t)x] == TRACE_ST_OK ? df[(size_t)x] : 0;
        status[2 * x] = st[(size_t)x]; status[2 * x + 1] = fw[(size_t)x];
    }
    *n_trace = off;
    return HINGE_OK;
}

int hinge_trace_last_stats(hinge_ctx* ctx, int64_t* out) {
    if (!ctx || !ctx->trace_st || !out) return fail(ctx, HINGE_E_ARG, "hinge_trace_last_stats: no hinge_trace_run yet");
    for (int k = 0; k < 8; k++) out[k] = ctx->trace_st->stats[k];
    return HINGE_OK;
}

}  // extern "C"
