// C ABI of `hinge draft` (include/hinge_hip.h, "hinge draft").  Included by hinge_capi.hip after consensus_capi.inc: the read DB
// with its bases is the one hinge_consensus_set_db uploaded (both slots = the read DB: a draft aligns reads with reads).
// Host work here: the segment table (shared with `hinge consensus`), job / ladder tables, buffer sizing, batching, launches.
// Which alignments, which ladders, which template: the caller's (hinge_amd/host/draft_main.cpp).
struct DraftState {
    DevBuf map_off, mapping, jobs, ladders, ents, dtab, tags, n_tags, cols, tbase, out, out_len, status, s2_far, mstate, mlink;
    size_t align_lds_attr = 0;
};

static void draft_release(hinge_ctx* ctx) {
    DraftState* d = ctx->draft;
    if (!d) return;
    DevBuf* all[] = {&d->map_off, &d->mapping, &d->jobs, &d->ladders, &d->ents, &d->dtab, &d->tags, &d->n_tags, &d->cols, &d->tbase, &d->out, &d->out_len, &d->status, &d->s2_far, &d->mstate, &d->mlink};
    for (DevBuf* b : all) release(*b);
    delete d;
    ctx->draft = nullptr;
}

// ---- hinge_draft_ladders: one batch of ladders - its tables in launch order, and what its buffers have to hold -------------------
// Routes (DESIGN.md 3.5).  A ladder with a LONG job - a member of 32768+ bases, or V / U + both staged sequences beyond the CU's
// 160 KB of LDS - has all its jobs aligned by k_draft_align_long; a ladder of 65+ members votes in k_draft_cns_deep.  The rest take
// k_draft_align / k_draft_cns exactly as before.  In a batch, the short ladders' jobs come first, then the long ones' (a kernel
// draws a contiguous range); the ladders of up to 64 members first, then the deep ones (out_len is put back in call order).
struct DraftBatch {
    std::vector<long long> h_boff;               // of the call: every read's first byte, the scratch budget, the band
    long long budget;
    int32_t band_tolerance;
    std::vector<DraftJob> jobs, jobs_long;       // of the batch, cleared with it
    std::vector<DraftLadder> lads, lads_deep;
    std::vector<char> lad_long, deep_long;
    std::vector<int64_t> src, src_deep;          // a ladder's place in the call, counted from the batch's first
    long long ent_tot, dtab_tot, tag_tot, col_tot, tb_tot, mem_tot;
    int lds_max, nc_max;
    size_t ns, nl64;                             // short jobs, ladders of up to 64 members (draft_batch_close)
    void clear() {
        jobs.clear(); jobs_long.clear(); lads.clear(); lads_deep.clear(); lad_long.clear(); deep_long.clear(); src.clear(); src_deep.clear();
        ent_tot = dtab_tot = tag_tot = col_tot = tb_tot = mem_tot = 0;
        lds_max = nc_max = 0;
        ns = nl64 = 0;
    }
};

static bool draft_seq_of(const CnsState* s, const hinge_draft_rung& r, DraftSeq* q) {
    if (r.read < 0 || r.read >= s->n_seq[1] || (r.strand != 0 && r.strand != 1)) return false;
    const int rl = s->h_rlen[1][(size_t)r.read];
    if (r.start < 0 || r.end < r.start || r.end > rl) return false;
    q->boff = 0; q->rlen = rl; q->strand = r.strand; q->start = r.start; q->len = r.end - r.start;
    return true;
}

// (a) One ladder (members rungs[0 .. n), `at` = its place in the batch, out_at / out_room = its output slot): validation, its job
// table, its share of the scratch.  Pure host work.  *fits = false (and nothing added) when a batch that already holds a ladder
// would outgrow the budget with this one.
static int draft_batch_add(hinge_ctx* ctx, DraftBatch& B, const hinge_draft_rung* rungs, int64_t n_rungs, int32_t template_rung, int64_t at, long long out_at,
                           long long out_room, bool* fits) {
    const CnsState* s = ctx->cns;
    const std::vector<long long>& h_boff = B.h_boff;
    const int32_t band_tolerance = B.band_tolerance;
    if (n_rungs < 1 || n_rungs > 65535)
        return fail(ctx, HINGE_E_CAPACITY, "hinge_draft_ladders: a ladder needs 1 .. 65535 members (the reference's vote counters are 16-bit, common.h)");
    const int n = (int)n_rungs;
    if (template_rung < 0 || template_rung >= n) return fail(ctx, HINGE_E_ARG, "hinge_draft_ladders: template member outside its ladder");
    DraftSeq T;
    if (!draft_seq_of(s, rungs[template_rung], &T)) return fail(ctx, HINGE_E_RANGE, "hinge_draft_ladders: a member lies outside its read");
    if (T.len >= (1 << 21)) return fail(ctx, HINGE_E_CAPACITY, "hinge_draft_ladders: a template of 2^21 or more bases (a tag holds its position in 21 bits)");
    T.boff = h_boff[(size_t)rungs[template_rung].read];
    long long e_l = 0, dt_l = 0, tg_l = 0, sumq = 0;
    int lds_l = 0;
    bool is_long = false;
    std::vector<DraftJob> mine((size_t)n);
    for (int m = 0; m < n; m++) {
        DraftJob& J = mine[(size_t)m];
        if (!draft_seq_of(s, rungs[m], &J.q)) return fail(ctx, HINGE_E_RANGE, "hinge_draft_ladders: a member lies outside its read");
        J.q.boff = h_boff[(size_t)rungs[m].read];
        J.t = T;
        J.max_d = (int)(0.3 * (J.q.len + J.t.len));                        // DW_banded.c:134
        // records of rounds 0 .. max_d - 1, min(d + 1, band + 1) each (closed form: the loop was 540 steps per job, 67 M per E. coli-sized call)
        const long long full = std::min<long long>(J.max_d, (long long)band_tolerance + 1);
        const long long cap = full * (full + 1) / 2 + (long long)(J.max_d - full) * ((long long)band_tolerance + 1);
        J.ent_cap = (int)std::min<long long>(cap, 0x7fffffffll);
        const int lds_j = (int)sizeof(int) * DraftCellsLds::scratch::words(J.max_d, J.q.len, J.t.len);     // what k_draft_align would keep in LDS
        if (J.q.len >= 32768 || lds_j > 160 * 1024) is_long = true;
        lds_l = std::max(lds_l, lds_j);
        sumq += J.q.len;
    }
    for (auto& J : mine) {            // offsets into the batch's buffers; a long job keeps its scratch behind its d table
        J.ent_off = B.ent_tot + e_l; J.dtab_off = B.dtab_tot + dt_l; J.tag_off = B.tag_tot + tg_l;
        e_l += (long long)(is_long ? DraftCellsHbm::REC_WORDS : DraftCellsLds::REC_WORDS) * J.ent_cap;
        dt_l += (long long)draft_dtab_words(J.max_d) + (is_long ? (long long)DraftCellsHbm::scratch::words(J.max_d, J.q.len, J.t.len) : 0ll);
        tg_l += (long long)J.q.len + J.t.len + 2;
    }
    const long long cols_l = 5ll * (T.len + 1 + sumq + 1);
    const long long mem_l = n > 64 ? (long long)(sizeof(DraftMember) + sizeof(unsigned)) / 4 * n : 0;   // k_draft_cns_deep's cursors
    const long long bytes = 4 * (B.ent_tot + e_l + B.dtab_tot + dt_l + B.tag_tot + tg_l + B.col_tot + cols_l + B.mem_tot + mem_l);
    *fits = at == 0 || bytes <= B.budget;
    if (!*fits) return HINGE_OK;
    if (!is_long) B.lds_max = std::max(B.lds_max, lds_l);
    DraftLadder L;
    std::vector<DraftJob>& jv = is_long ? B.jobs_long : B.jobs;
    L.job0 = (int)jv.size(); L.n = n; L.t_len = T.len + 1;
    L.col_off = B.col_tot; L.col_cap = (int)std::min<long long>(cols_l, 0x7fffffffll);
    L.tb_off = B.tb_tot; L.out_off = out_at;
    if (out_room < 2ll * L.t_len) return fail(ctx, HINGE_E_ARG, "hinge_draft_ladders: an output slot smaller than 2 * (template length + 1)");
    for (auto& J : mine) jv.push_back(J);
    if (n > 64) { B.lads_deep.push_back(L); B.deep_long.push_back(is_long); B.src_deep.push_back(at); B.nc_max = std::max(B.nc_max, (n + 63) / 64); }
    else { B.lads.push_back(L); B.lad_long.push_back(is_long); B.src.push_back(at); }
    B.ent_tot += e_l; B.dtab_tot += dt_l; B.tag_tot += tg_l; B.col_tot += cols_l; B.tb_tot += 2ll * L.t_len; B.mem_tot += mem_l;
    return HINGE_OK;
}

// the long ladders' jobs behind the short ones'; the deep ladders behind the rest
static void draft_batch_close(DraftBatch& B) {
    B.ns = B.jobs.size(); B.nl64 = B.lads.size();
    for (size_t i = 0; i < B.lads.size(); i++) if (B.lad_long[i]) B.lads[i].job0 += (int)B.ns;
    for (size_t i = 0; i < B.lads_deep.size(); i++) if (B.deep_long[i]) B.lads_deep[i].job0 += (int)B.ns;
    B.jobs.insert(B.jobs.end(), B.jobs_long.begin(), B.jobs_long.end());
    B.lads.insert(B.lads.end(), B.lads_deep.begin(), B.lads_deep.end());
    B.src.insert(B.src.end(), B.src_deep.begin(), B.src_deep.end());
}

// (b) the batch's buffers, and its tables on their way to the device
static int draft_batch_upload(hinge_ctx* ctx, const DraftBatch& B, long long out_bytes) {
    DraftState* d = ctx->draft;
    const size_t nj = B.jobs.size(), nl = B.lads.size();
    int rc;
    if ((rc = ensure(ctx, d->jobs, sizeof(DraftJob) * nj))) return rc;
    if ((rc = ensure(ctx, d->ladders, sizeof(DraftLadder) * nl))) return rc;
    if ((rc = ensure(ctx, d->ents, sizeof(unsigned) * (size_t)std::max(B.ent_tot, 1ll)))) return rc;
    if ((rc = ensure(ctx, d->dtab, sizeof(int) * (size_t)std::max(B.dtab_tot, 1ll)))) return rc;
    if ((rc = ensure(ctx, d->tags, sizeof(unsigned) * (size_t)std::max(B.tag_tot, 1ll)))) return rc;
    if ((rc = ensure(ctx, d->n_tags, sizeof(int) * nj))) return rc;
    if ((rc = ensure(ctx, d->cols, sizeof(unsigned) * (size_t)std::max(B.col_tot, 1ll)))) return rc;
    if ((rc = ensure(ctx, d->tbase, sizeof(int) * (size_t)std::max(B.tb_tot, 1ll)))) return rc;
    if ((rc = ensure(ctx, d->out, (size_t)std::max(out_bytes, 1ll)))) return rc;
    if ((rc = ensure(ctx, d->out_len, sizeof(int) * nl))) return rc;
    if (nl > B.nl64) {
        if ((rc = ensure(ctx, d->mstate, sizeof(DraftMember) * nj))) return rc;
        if ((rc = ensure(ctx, d->mlink, sizeof(unsigned) * nj))) return rc;
    }
    CK(hipMemcpyAsync(d->jobs.p, B.jobs.data(), sizeof(DraftJob) * nj, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(d->ladders.p, B.lads.data(), sizeof(DraftLadder) * nl, hipMemcpyHostToDevice, ctx->stream));
    return HINGE_OK;
}

// (c) the batch's launches: the two aligners over their job ranges, then the two consensus kernels over their ladder ranges
static int draft_batch_launch(hinge_ctx* ctx, const DraftBatch& B) {
    DraftState* d = ctx->draft;
    const CnsState* s = ctx->cns;
    const size_t ns = B.ns, nl64 = B.nl64, n_long = B.jobs.size() - ns, n_deep = B.lads.size() - nl64;
    const int lds_max = B.lds_max, band_tolerance = B.band_tolerance;
    int rc;
    if ((size_t)lds_max > 48 * 1024 && (size_t)lds_max > d->align_lds_attr) {
        CK(hipFuncSetAttribute((const void*)k_draft_align, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        d->align_lds_attr = (size_t)lds_max;
    }
    CK(hipMemsetAsync((int*)d->status.p + DRAFT_SLOT_ALIGN, 0, sizeof(int) * (DRAFT_SLOTS - DRAFT_SLOT_ALIGN), ctx->stream));     // the cursors
    if (ns) {
        ProfScope _ps(ctx, KID_DRAFT_ALIGN);
        // as many one-wavefront workgroups per CU as their LDS leaves room for (V / U + the staged sequences: ~9 KiB for 900-base members)
        const size_t per_cu = std::min<size_t>(32, std::max<size_t>(1, (size_t)(160 * 1024) / (size_t)std::max(lds_max, 1024)));
        const unsigned grid = (unsigned)std::min<size_t>(ns, (size_t)ctx->n_cu * per_cu);
        hipLaunchKernelGGL(k_draft_align, dim3(grid), dim3(64), (size_t)lds_max, ctx->stream, (const unsigned char*)s->bps[1].p, (const DraftJob*)d->jobs.p, (int)ns,
                           band_tolerance, (unsigned*)d->ents.p, (int*)d->dtab.p, (unsigned*)d->tags.p, (int*)d->n_tags.p, (int*)d->status.p);
    }
    if (n_long) {
        ProfScope _ps(ctx, KID_DRAFT_ALIGN_LONG);
        // no LDS: V / U and the sequences in HBM; one wavefront per job, as many as the chip holds
        const unsigned grid = (unsigned)std::min<size_t>(n_long, (size_t)ctx->n_cu * 32);
        hipLaunchKernelGGL(k_draft_align_long, dim3(grid), dim3(64), 0, ctx->stream, (const unsigned char*)s->bps[1].p, (const DraftJob*)d->jobs.p, (int)ns, (int)n_long,
                           band_tolerance, (unsigned*)d->ents.p, (int*)d->dtab.p, (unsigned*)d->tags.p, (int*)d->n_tags.p, (int*)d->status.p);
    }
    {
        // one-wavefront workgroups: every wavefront slot of the chip; k_draft_cns_deep: as many as its chunk masks leave LDS for
        // (5 x 8 bytes per 64 members: at most 40 KB at 65535 members, under the 48 KB a launch gets without an attribute)
        const unsigned grid = (unsigned)std::min<size_t>(nl64, (size_t)ctx->n_cu * 32);
        const size_t deep_lds = (size_t)5 * 8 * std::max(B.nc_max, 1);
        const size_t deep_per_cu = std::min<size_t>(32, (size_t)(160 * 1024) / (deep_lds + sizeof(int) * 2 * DRAFT_S2_LDS * 5));
        const unsigned grid_deep = (unsigned)std::min<size_t>(n_deep, (size_t)ctx->n_cu * deep_per_cu);
        if ((rc = ensure(ctx, d->s2_far, sizeof(int) * (size_t)std::max(grid, grid_deep) * 2 * 256 * 5))) return rc;
        if (nl64) {
            ProfScope _ps(ctx, KID_DRAFT_CNS);
            hipLaunchKernelGGL(k_draft_cns, dim3(grid), dim3(64), 0, ctx->stream, (const DraftJob*)d->jobs.p, (const DraftLadder*)d->ladders.p, (int)nl64, (const unsigned*)d->tags.p,
                               (const int*)d->n_tags.p, (unsigned*)d->cols.p, (int*)d->tbase.p, (char*)d->out.p, (int*)d->out_len.p, 1u, (int*)d->status.p, (int*)d->s2_far.p);
        }
        if (n_deep) {
            ProfScope _ps(ctx, KID_DRAFT_CNS_DEEP);
            hipLaunchKernelGGL(k_draft_cns_deep, dim3(grid_deep), dim3(64), deep_lds, ctx->stream, (const DraftJob*)d->jobs.p, (const DraftLadder*)d->ladders.p + nl64, (int)n_deep,
                               (const unsigned*)d->tags.p, (const int*)d->n_tags.p, (unsigned*)d->cols.p, (int*)d->tbase.p, (char*)d->out.p, (int*)d->out_len.p + nl64, 1u,
                               (int*)d->status.p, (int*)d->s2_far.p, (DraftMember*)d->mstate.p, (unsigned*)d->mlink.p);
        }
    }
    CK(hipGetLastError());
    return HINGE_OK;
}

extern "C" {

int hinge_draft_mappings(hinge_ctx* ctx, int64_t n_aln, const hinge_cns_alignment* alns, const uint16_t* trace, int64_t n_trace, int32_t tspace,
                         const int64_t* map_off, uint32_t* mapping) {
    if (!ctx || !ctx->cns || n_aln < 0 || (n_aln > 0 && (!alns || !map_off || !mapping)) || n_trace < 0 || (n_trace > 0 && !trace) || tspace <= 0)
        return fail(ctx, HINGE_E_ARG, "hinge_draft_mappings: bad arguments (call hinge_consensus_set_db for both slots first)");
    if (n_aln == 0) return HINGE_OK;
    for (int64_t i = 0; i < n_aln; i++)
        if (map_off[i + 1] - map_off[i] != (int64_t)alns[i].aepos - alns[i].abpos || map_off[i] < 0) return fail(ctx, HINGE_E_ARG, "hinge_draft_mappings: map_off does not follow aepos - abpos");
    CK(hipSetDevice(ctx->device));
    if (!ctx->draft) ctx->draft = new DraftState();
    DraftState* d = ctx->draft;
    CnsState* s = ctx->cns;
    s->ran = false;
    int rc;
    if ((rc = cns_realign_stage(ctx, n_aln, alns, trace, n_trace, tspace))) return rc;
    const size_t total = (size_t)map_off[n_aln];
    if ((rc = ensure(ctx, d->map_off, sizeof(long long) * (size_t)(n_aln + 1)))) return rc;
    if ((rc = ensure(ctx, d->mapping, sizeof(unsigned) * std::max<size_t>(total, 1)))) return rc;
    CK(hipMemcpyAsync(d->map_off.p, map_off, sizeof(int64_t) * (size_t)(n_aln + 1), hipMemcpyHostToDevice, ctx->stream));
    if (s->n_seg)
        hipLaunchKernelGGL(k_draft_map, dim3((unsigned)((s->n_seg + CNS_BLOCK - 1) / CNS_BLOCK)), dim3(CNS_BLOCK), 0, ctx->stream, (const CnsAln*)s->alns.p, (const CnsSeg*)s->segs.p,
                           (int)s->n_seg, (const int*)s->indels.p, (const int*)s->n_indel.p, (const long long*)d->map_off.p, (unsigned*)d->mapping.p);
    CK(hipGetLastError());
    int st = 0;
    CK(hipMemcpyAsync(&st, s->scal.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (total) CK(hipMemcpyAsync(mapping, d->mapping.p, sizeof(unsigned) * total, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if (st & CNS_ST_WAVES) return fail(ctx, HINGE_E_RANGE, "hinge draft: a trace-point segment needs more edit operations than its alignment's recorded diffs (the reference overruns its wave arrays here, LAInterface.cpp:3444-3466)");
    if (st & CNS_ST_INDELS) return fail(ctx, HINGE_E_RANGE, "hinge draft: a segment's indel list outgrew its slots");
    return HINGE_OK;
}

int hinge_draft_ladders(hinge_ctx* ctx, int64_t n_ladders, const int64_t* rung_off, const hinge_draft_rung* rungs, const int32_t* template_rung, int32_t band_tolerance,
                        const int64_t* out_off, char* out, int32_t* out_len) {
    if (!ctx || !ctx->cns || n_ladders < 0 || (n_ladders > 0 && (!rung_off || !rungs || !template_rung || !out_off || !out || !out_len)) || band_tolerance < 1)
        return fail(ctx, HINGE_E_ARG, "hinge_draft_ladders: bad arguments (call hinge_consensus_set_db first)");
    if (n_ladders == 0) return HINGE_OK;
    CK(hipSetDevice(ctx->device));
    if (!ctx->draft) ctx->draft = new DraftState();
    DraftState* d = ctx->draft;
    CnsState* s = ctx->cns;
    const int n_reads = s->n_seq[1];
    // Scratch of one batch of ladders (the aligner's (d, k) records dominate: ~280 KB per 900-base member at the reference's max_d =
    // 0.3 (q + t), a third of it touched).  Round 6: as much as HALF the free HBM (at most 96 GB) instead of 8 GB - an E. coli-sized
    // draft (5 000 ladders, 125 k member alignments, 35 GB) is then ONE batch: k_draft_cns, one wavefront per ladder and latency-bound,
    // has 5 000 wavefronts to hide its latencies behind instead of 1 000 (one per SIMD), and k_draft_align one tail instead of five.
    long long budget = 8ll << 30;
    {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::max(budget, std::min<long long>((long long)(fr / 2), 96ll << 30));
    }
    if (const char* g = getenv("HINGE_DRAFT_SCRATCH_GB")) budget = std::max(1ll, atoll(g)) << 30;
    int rc;
    if ((rc = ensure(ctx, d->status, sizeof(int) * DRAFT_SLOTS))) return rc;
    // the flags and the cursors of the four kernels that draw their work (DRAFT_SLOT_*); the cursors are cleared per batch
    CK(hipMemsetAsync(d->status.p, 0, sizeof(int) * DRAFT_SLOTS, ctx->stream));
    // the read's first byte lives in the device table; the jobs carry it so the kernels need one look-up less: fetch the host copy
    DraftBatch B;
    B.budget = budget; B.band_tolerance = band_tolerance;
    B.h_boff.resize((size_t)std::max(n_reads, 1));
    CK(hipMemcpy(B.h_boff.data(), s->boff[1].p, sizeof(long long) * (size_t)n_reads, hipMemcpyDeviceToHost));
    std::vector<int32_t> h_len;
    for (int64_t l0 = 0; l0 < n_ladders;) {
        // ---- one batch: ladders l0 .. l1 whose scratch fits the budget ------------------------------------------------------------
        B.clear();
        int64_t l1 = l0;
        for (; l1 < n_ladders; l1++) {
            bool fits = true;
            if ((rc = draft_batch_add(ctx, B, rungs + rung_off[l1], rung_off[l1 + 1] - rung_off[l1], template_rung[l1], l1 - l0, out_off[l1] - out_off[l0],
                                      out_off[l1 + 1] - out_off[l1], &fits))) return rc;
            if (!fits) break;
        }
        draft_batch_close(B);
        const size_t nl = B.lads.size();
        const long long out_bytes = out_off[l1] - out_off[l0];
        if ((rc = draft_batch_upload(ctx, B, out_bytes))) return rc;
        if ((rc = draft_batch_launch(ctx, B))) return rc;
        if (out_bytes) CK(hipMemcpyAsync(out + out_off[l0], d->out.p, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        h_len.resize(nl);
        CK(hipMemcpyAsync(h_len.data(), d->out_len.p, sizeof(int) * nl, hipMemcpyDeviceToHost, ctx->stream));
        int st = 0;
        CK(hipMemcpyAsync(&st, d->status.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < nl; i++) out_len[l0 + B.src[i]] = h_len[i];
        if (st & DRAFT_ST_CAP) return fail(ctx, HINGE_E_CAPACITY, "hinge draft: a ladder outgrew its buffers");
        if (st & DRAFT_ST_DELTA) return fail(ctx, HINGE_E_RANGE, "hinge draft: 255+ inserted bases in a row (the reference's alignment tags are undefined there, falcon.c:96)");
        if (st & DRAFT_ST_BASE) return fail(ctx, HINGE_E_UNDEFINED, "hinge draft: a ladder without a scoring column (the reference's assert, falcon.c:437)");
        l0 = l1;
    }
    return HINGE_OK;
}

}  // extern "C"
