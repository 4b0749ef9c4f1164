// C ABI of `hinge paf2las` (include/hinge_hip.h, "hinge paf2las").  Included by hinge_capi.hip.
// Host work here: range checks, the widening rounds (W, 2 W, ... while it stays within band_max: four with the defaults, never more
// than TRACE_ROUNDS = the doublings from the smallest to the largest legal band), the batches of one
// round under the direction-scratch budget, the launches, the results back in the caller's order.  The kernels: trace_kernels.h.
constexpr int TRACE_ROUNDS = 9;

enum TraceMode { TRACE_MODE_RUN = 0, TRACE_MODE_REFINE = 1, TRACE_MODE_LOCAL = 2 };   // hinge_trace_run / _refine / _local

struct TraceState {
    DevBuf jobs, dirs, trace, status, diffs, cost, clip, score, best;
    size_t lds_attr = 0, lds_attr_local = 0;        // hipFuncAttributeMaxDynamicSharedMemorySize is per kernel: k_trace_fill, k_trace_fill_local
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hinge_trace_last_stats
};

static void trace_release(hinge_ctx* ctx) {
    TraceState* t = ctx->trace_st;
    if (!t) return;
    DevBuf* all[] = {&t->jobs, &t->dirs, &t->trace, &t->status, &t->diffs, &t->cost, &t->clip, &t->score, &t->best};
    for (DevBuf* b : all) release(*b);
    delete t;
    ctx->trace_st = nullptr;
}

static long long trace_env(const char* name, long long def) {
    const char* g = getenv(name);
    return (g && *g) ? atoll(g) : def;
}

// One batch: jobs[0..nj) (dir_off / trace_off laid out by the caller) at half-width W.  Results to the host vectors.
// TRACE_MODE_RUN: k_trace_fill, k_trace_walk; _REFINE: k_trace_clip in the walk's place, with the kept cells and the scores back as
// well; _LOCAL: k_trace_fill_local, k_trace_walk_local, the same results back as _REFINE.  ends: null for _RUN only.
static int trace_batch(hinge_ctx* ctx, const std::vector<TraceJob>& jobs, long long dir_words, long long n_vals, int W, int tspace, int mode, const hinge_trace_ends* ends,
                       std::vector<unsigned short>& h_trace, std::vector<int>& h_status, std::vector<int>& h_diffs, std::vector<int>& h_clip, std::vector<int>& h_score) {
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
    if (ends) {
        if ((rc = ensure(ctx, t->clip, sizeof(int) * 4 * nj))) return rc;
        if ((rc = ensure(ctx, t->score, sizeof(int) * nj))) return rc;
    }
    if (mode == TRACE_MODE_LOCAL && (rc = ensure(ctx, t->best, sizeof(int) * 3 * nj))) return rc;
    CK(hipMemcpyAsync(t->jobs.p, jobs.data(), sizeof(TraceJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    // poison: a slot no kernel wrote is seen as such, never as data (0xff bytes: status / diffs / cost -1, trace 0xffff)
    CK(hipMemsetAsync(t->trace.p, 0xff, sizeof(unsigned short) * (size_t)std::max<long long>(n_vals, 1), ctx->stream));
    CK(hipMemsetAsync(t->status.p, 0xff, sizeof(int) * nj, ctx->stream));
    CK(hipMemsetAsync(t->diffs.p, 0xff, sizeof(int) * nj, ctx->stream));
    CK(hipMemsetAsync(t->cost.p, 0xff, sizeof(int) * nj, ctx->stream));
    if (ends) {
        CK(hipMemsetAsync(t->clip.p, 0xff, sizeof(int) * 4 * nj, ctx->stream));
        CK(hipMemsetAsync(t->score.p, 0xff, sizeof(int) * nj, ctx->stream));
    }
    if (mode == TRACE_MODE_LOCAL) CK(hipMemsetAsync(t->best.p, 0xff, sizeof(int) * 3 * nj, ctx->stream));
    const size_t lds = trace_lds_bytes(W);
    if (mode == TRACE_MODE_LOCAL) {
        if (lds > 48 * 1024 && lds > t->lds_attr_local) {
            CK(hipFuncSetAttribute((const void*)k_trace_fill_local, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            t->lds_attr_local = lds;
        }
    } else if (lds > 48 * 1024 && lds > t->lds_attr) {
        CK(hipFuncSetAttribute((const void*)k_trace_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        t->lds_attr = lds;
    }
    CnsSeqs SA{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
    CnsSeqs SB{(const unsigned char*)s->bps[1].p, (const long long*)s->boff[1].p, (const int*)s->rlen[1].p};
    const int tmax = tspace <= 125 ? 255 : 65534;
    const unsigned walk_blocks = (unsigned)((nj + 63) / 64);
    if (mode == TRACE_MODE_LOCAL) {
        ProfScope _ps(ctx, KID_TRACE_FILL_LOCAL);
        hipLaunchKernelGGL(k_trace_fill_local, dim3((unsigned)nj), dim3(64), lds, ctx->stream, SA, SB, (const TraceJob*)t->jobs.p, (int)nj, W, (int)ends->match, (int)ends->diff,
                           (unsigned*)t->dirs.p, (int*)t->best.p);
    } else {
        ProfScope _ps(ctx, KID_TRACE_FILL);
        hipLaunchKernelGGL(k_trace_fill, dim3((unsigned)nj), dim3(64), lds, ctx->stream, SA, SB, (const TraceJob*)t->jobs.p, (int)nj, W, (unsigned*)t->dirs.p, (int*)t->cost.p);
    }
    if (mode == TRACE_MODE_LOCAL) {
        ProfScope _ps(ctx, KID_TRACE_WALK_LOCAL);
        hipLaunchKernelGGL(k_trace_walk_local, dim3(walk_blocks), dim3(64), 0, ctx->stream, (const TraceJob*)t->jobs.p, (int)nj, W, tspace, tmax, (int)ends->match, (int)ends->diff,
                           (int)ends->min_score, trace_local_margin(W), (const unsigned*)t->dirs.p, (const int*)t->best.p, (unsigned short*)t->trace.p, (int*)t->diffs.p,
                           (int*)t->status.p, (int*)t->clip.p, (int*)t->score.p);
    } else if (mode == TRACE_MODE_REFINE) {
        ProfScope _ps(ctx, KID_TRACE_CLIP);
        hipLaunchKernelGGL(k_trace_clip, dim3(walk_blocks), dim3(64), 0, ctx->stream, (const TraceJob*)t->jobs.p, (int)nj, W, tspace, tmax,
                           (int)ends->match, (int)ends->diff, (int)ends->min_score, (const unsigned*)t->dirs.p, (const int*)t->cost.p, (unsigned short*)t->trace.p, (int*)t->diffs.p,
                           (int*)t->status.p, (int*)t->clip.p, (int*)t->score.p);
    } else {
        ProfScope _ps(ctx, KID_TRACE_WALK);
        hipLaunchKernelGGL(k_trace_walk, dim3(walk_blocks), dim3(64), 0, ctx->stream, (const TraceJob*)t->jobs.p, (int)nj, W, tspace, tmax,
                           (const unsigned*)t->dirs.p, (const int*)t->cost.p, (unsigned short*)t->trace.p, (int*)t->diffs.p, (int*)t->status.p);
    }
    CK(hipGetLastError());
    h_trace.resize((size_t)std::max<long long>(n_vals, 1));
    h_status.resize(nj);
    h_diffs.resize(nj);
    if (n_vals) CK(hipMemcpyAsync(h_trace.data(), t->trace.p, sizeof(unsigned short) * (size_t)n_vals, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_status.data(), t->status.p, sizeof(int) * nj, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(h_diffs.data(), t->diffs.p, sizeof(int) * nj, hipMemcpyDeviceToHost, ctx->stream));
    if (ends) {
        h_clip.resize(4 * nj);
        h_score.resize(nj);
        CK(hipMemcpyAsync(h_clip.data(), t->clip.p, sizeof(int) * 4 * nj, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(h_score.data(), t->score.p, sizeof(int) * nj, hipMemcpyDeviceToHost, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));
    return HINGE_OK;
}

// hinge_trace_run (ends == nullptr), hinge_trace_refine and hinge_trace_local (ends: extend, match, diff, min_score, all resolved)
// share everything but the box a placement runs in, the kernels of a batch, what of a job's slots is a record's, and - local -
// that an EMPTY placement goes on to 2 W like a NO_PATH one (a diagonal off by more than W leaves nothing of it in the band).
struct TraceOut {                       // the caller's output arrays (score: hinge_trace_refine only)
    hinge_cns_alignment* alns;
    uint16_t* trace;
    int64_t trace_cap;
    int64_t* n_trace;
    int32_t *diffs, *status, *score;
};

static int trace_call(hinge_ctx* ctx, const char* who, int64_t n, const hinge_cns_alignment* placements, int32_t tspace, int32_t band, int32_t band_max,
                      int mode, const hinge_trace_ends* ends, const TraceOut& out) {
    hinge_cns_alignment* const out_alns = out.alns;
    uint16_t* const trace = out.trace;
    const int64_t trace_cap = out.trace_cap;
    int64_t* const n_trace = out.n_trace;
    int32_t *const diffs = out.diffs, *const status = out.status, *const score = out.score;
    auto me = [who](const char* what) { return std::string(who) + what; };      // error texts only
    if (!ctx || !ctx->cns || n < 0 || (n > 0 && (!placements || !out_alns || !diffs || !status || (ends && !score))) || !n_trace || trace_cap < 0 || (trace_cap > 0 && !trace) ||
        tspace <= 0 || tspace > 32767)
        return fail(ctx, HINGE_E_ARG, me(": bad arguments (call hinge_consensus_set_db for both DBs first)"));
    if (band <= 0) band = (int32_t)trace_env("HINGE_TRACE_BAND", 128);
    if (band_max <= 0) band_max = (int32_t)std::max<long long>(trace_env("HINGE_TRACE_BAND_MAX", 1024), band);
    if (band < TRACE_BAND_MIN || (band % 8) != 0 || band_max < band || band_max > TRACE_BAND_LIMIT)
        return fail(ctx, HINGE_E_ARG, me(": the band must be a multiple of 8 from 8 to 2048, and band_max no smaller"));
    CnsState* s = ctx->cns;
    CK(hipSetDevice(ctx->device));
    if (!ctx->trace_st) ctx->trace_st = new TraceState();
    TraceState* t = ctx->trace_st;
    for (int64_t& v : t->stats) v = 0;
    *n_trace = 0;
    // ---- range checks, the box and the segments of every placement: all before any launch -----------------------------------------
    std::vector<int> nseg((size_t)n);
    std::vector<hinge_cns_alignment> box;             // refine: the placements widened (B in its strand frame: its room is bbpos and blen - bepos there)
    if (ends) box.assign(placements, placements + n);
    int64_t all_vals = 0;
    for (int64_t x = 0; x < n; x++) {
        const hinge_cns_alignment& r = placements[x];
        if (r.aread < 0 || r.aread >= s->n_seq[0] || r.bread < 0 || r.bread >= s->n_seq[1]) return fail(ctx, HINGE_E_RANGE, me(": read id outside its DB"));
        const int alen = s->h_rlen[0][(size_t)r.aread], blen = s->h_rlen[1][(size_t)r.bread];
        if (!(0 <= r.abpos && r.abpos < r.aepos && r.aepos <= alen && 0 <= r.bbpos && r.bbpos < r.bepos && r.bepos <= blen))
            return fail(ctx, HINGE_E_RANGE, me(": placement coordinates outside their reads, or an empty stretch"));
        int ab = r.abpos, ae = r.aepos;
        if (ends) {
            hinge_cns_alignment& b = box[(size_t)x];
            const int e0 = std::min(ends->extend, std::min(r.abpos, r.bbpos)), e1 = std::min(ends->extend, std::min(alen - r.aepos, blen - r.bepos));
            b.abpos -= e0; b.bbpos -= e0; b.aepos += e1; b.bepos += e1;
            ab = b.abpos; ae = b.aepos;
        }
        nseg[(size_t)x] = trace_segments(ab, ae, tspace);
        all_vals += 2 * (int64_t)nseg[(size_t)x];
    }
    if (all_vals > trace_cap)
        return fail(ctx, HINGE_E_CAPACITY, me(ends ? ": the trace array must hold two values per trace-point segment of every widened placement" : ": the trace array must hold two values per trace-point segment of every placement"));
    const hinge_cns_alignment* run = ends ? box.data() : placements;
    long long budget = std::max(1ll, trace_env("HINGE_TRACE_SCRATCH_MB", 4096)) << 20;
    budget = std::max(1ll, trace_env("HINGE_TRACE_SCRATCH_BYTES", budget));
    const int st_last = ends ? TRACE_ST_EMPTY : TRACE_ST_STEPS;
    // ---- the rounds ---------------------------------------------------------------------------------------------------------------
    std::vector<int> st((size_t)n, TRACE_ST_POISON), fw((size_t)n, 0), df((size_t)n, 0), sc((size_t)n, 0);
    std::vector<std::vector<unsigned short>> tr((size_t)n);
    std::vector<int64_t> pending((size_t)n), next;
    for (int64_t x = 0; x < n; x++) pending[(size_t)x] = x;
    std::vector<TraceJob> jobs;
    std::vector<int64_t> job_of;
    std::vector<unsigned short> h_trace;
    std::vector<int> h_status, h_diffs, h_clip, h_score;
    std::vector<hinge_cns_alignment> kept;            // refine: the refined end points of the records
    if (ends) kept.assign(placements, placements + n);
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
                const hinge_cns_alignment& r = run[x];
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
            if ((rc = trace_batch(ctx, jobs, words, vals, W, tspace, mode, ends, h_trace, h_status, h_diffs, h_clip, h_score))) return rc;
            t->stats[0]++;
            t->stats[1] = std::max<int64_t>(t->stats[1], words * (int64_t)sizeof(unsigned));
            t->stats[2] += (int64_t)jobs.size();
            for (size_t k = 0; k < jobs.size(); k++) {
                const int64_t x = job_of[k];
                const int code = h_status[k];
                if (code < TRACE_ST_OK || code > st_last) return fail(ctx, HINGE_E_DEVICE, me(": a placement's status slot was never written"));
                st[(size_t)x] = code; df[(size_t)x] = h_diffs[k];
                if (code == TRACE_ST_OK) {
                    const TraceJob& j = jobs[k];
                    int first = 0, cnt = j.nseg;
                    if (ends) {                           // the kept cells -> coordinates; the kept segments among the box's slots
                        const int* c = h_clip.data() + 4 * k;
                        const int alen = j.ae - j.ab, blen = j.be - j.bb;
                        if (!(0 <= c[0] && c[0] < c[2] && c[2] <= alen && 0 <= c[1] && c[1] < c[3] && c[3] <= blen))
                            return fail(ctx, HINGE_E_DEVICE, me(": a placement's kept cells were never written, or lie outside its box"));
                        hinge_cns_alignment& o = kept[(size_t)x];
                        o.abpos = j.ab + c[0]; o.aepos = j.ab + c[2]; o.bbpos = j.bb + c[1]; o.bepos = j.bb + c[3];
                        first = o.abpos / tspace - j.ab / tspace;
                        cnt = trace_segments(o.abpos, o.aepos, tspace);
                        if (first + cnt > j.nseg) return fail(ctx, HINGE_E_DEVICE, me(": kept segments outside the placement's slots"));
                        sc[(size_t)x] = h_score[k];
                    }
                    const unsigned short* p = h_trace.data() + j.trace_off + 2 * first;
                    tr[(size_t)x].assign(p, p + 2 * cnt);
                    for (unsigned short v : tr[(size_t)x]) if (v == TRACE_POISON16) return fail(ctx, HINGE_E_DEVICE, me(": a trace slot was never written"));
                } else if ((code == TRACE_ST_TOUCHED || code == TRACE_ST_NO_PATH) && !last) next.push_back(x);
                else if (code == TRACE_ST_EMPTY && mode == TRACE_MODE_LOCAL && !last) { next.push_back(x); t->stats[7]++; }
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
        const bool rec = st[(size_t)x] == TRACE_ST_OK;
        hinge_cns_alignment o = (ends && rec) ? kept[(size_t)x] : placements[x];
        o.trace_off = off; o.tlen = 0;
        if (rec) {
            o.tlen = (int32_t)tr[(size_t)x].size();
            memcpy(trace + off, tr[(size_t)x].data(), sizeof(uint16_t) * tr[(size_t)x].size());
            off += o.tlen;
            if (fw[(size_t)x] != band) t->stats[4]++;
        } else {
            t->stats[5]++;
            if (st[(size_t)x] == TRACE_ST_EMPTY) t->stats[6]++;
        }
        out_alns[x] = o;
        diffs[x] = rec ? df[(size_t)x] : 0;
        if (score) score[x] = rec ? sc[(size_t)x] : 0;
        status[2 * x] = st[(size_t)x]; status[2 * x + 1] = fw[(size_t)x];
    }
    *n_trace = off;
    return HINGE_OK;
}

extern "C" {

int hinge_trace_run(hinge_ctx* ctx, int64_t n, const hinge_cns_alignment* placements, int32_t tspace, int32_t band, int32_t band_max, hinge_cns_alignment* out_alns,
                    uint16_t* trace, int64_t trace_cap, int64_t* n_trace, int32_t* diffs, int32_t* status) {
    return trace_call(ctx, "hinge_trace_run", n, placements, tspace, band, band_max, TRACE_MODE_RUN, nullptr, TraceOut{out_alns, trace, trace_cap, n_trace, diffs, status, nullptr});
}

int hinge_trace_refine(hinge_ctx* ctx, int64_t n, const hinge_cns_alignment* placements, int32_t tspace, int32_t band, int32_t band_max, const hinge_trace_ends* ends,
                       hinge_cns_alignment* out_alns, uint16_t* trace, int64_t trace_cap, int64_t* n_trace, int32_t* diffs, int32_t* status, int32_t* score) {
    hinge_trace_ends e = ends ? *ends : hinge_trace_ends{-1, 0, 0, 0};
    if (e.extend == -1) e.extend = (int32_t)trace_env("HINGE_TRACE_EXTEND", 50);
    if (e.match == 0) e.match = (int32_t)trace_env("HINGE_TRACE_MATCH", 1);
    if (e.diff == 0) e.diff = (int32_t)trace_env("HINGE_TRACE_DIFF", 2);
    if (e.min_score == 0) e.min_score = (int32_t)trace_env("HINGE_TRACE_MIN_SCORE", 1);
    if (e.extend < 0 || e.extend > 32767 || e.match < 1 || e.match > 15 || e.diff < 1 || e.diff > 15)
        return fail(ctx, HINGE_E_ARG, "hinge_trace_refine: extend must lie in 0..32767 (-1 = the default), match and diff in 1..15 (0 = the default)");
    return trace_call(ctx, "hinge_trace_refine", n, placements, tspace, band, band_max, TRACE_MODE_REFINE, &e, TraceOut{out_alns, trace, trace_cap, n_trace, diffs, status, score});
}

int hinge_trace_local(hinge_ctx* ctx, int64_t n, const hinge_cns_alignment* placements, int32_t tspace, int32_t band, int32_t band_max, const hinge_trace_ends* ends,
                      hinge_cns_alignment* out_alns, uint16_t* trace, int64_t trace_cap, int64_t* n_trace, int32_t* diffs, int32_t* status, int32_t* score) {
    hinge_trace_ends e = ends ? *ends : hinge_trace_ends{-1, 0, 0, 0};
    if (e.extend == -1) e.extend = (int32_t)trace_env("HINGE_TRACE_EXTEND", 50);
    if (e.match == 0) e.match = (int32_t)trace_env("HINGE_TRACE_MATCH", 1);
    if (e.diff == 0) e.diff = (int32_t)trace_env("HINGE_TRACE_DIFF", 2);
    if (e.min_score == 0) e.min_score = (int32_t)trace_env("HINGE_TRACE_MIN_SCORE", HINGE_TRACE_LOCAL_MIN_SCORE);
    if (e.extend < 0 || e.extend > 32767 || e.match < 1 || e.match > 15 || e.diff < 1 || e.diff > 15)
        return fail(ctx, HINGE_E_ARG, "hinge_trace_local: extend must lie in 0..32767 (-1 = the default), match and diff in 1..15 (0 = the default)");
    return trace_call(ctx, "hinge_trace_local", n, placements, tspace, band, band_max, TRACE_MODE_LOCAL, &e, TraceOut{out_alns, trace, trace_cap, n_trace, diffs, status, score});
}

int hinge_trace_last_stats(hinge_ctx* ctx, int64_t* out) {
    if (!ctx || !ctx->trace_st || !out) return fail(ctx, HINGE_E_ARG, "hinge_trace_last_stats: no hinge_trace_run yet");
    for (int k = 0; k < 8; k++) out[k] = ctx->trace_st->stats[k];
    return HINGE_OK;
}

}  // extern "C"
