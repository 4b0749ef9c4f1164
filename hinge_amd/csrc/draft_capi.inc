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
    if ((rc = ensure(ctx, d->status, 32))) return rc;
    // [0] status flags; cursors, cleared per batch: [1] k_draft_align's jobs, [2] k_draft_cns' ladders, [3] k_draft_align_long's jobs,
    // [4] k_draft_cns_deep's ladders
    CK(hipMemsetAsync(d->status.p, 0, 32, ctx->stream));
    // Routes (DESIGN.md 3.5).  A ladder with a LONG job - a member of 32768+ bases, or V / U + both staged sequences beyond the CU's
    // 160 KB of LDS - has all its jobs aligned by k_draft_align_long; a ladder of 65+ members votes in k_draft_cns_deep.  The rest take
    // k_draft_align / k_draft_cns exactly as before.  In a batch, the short ladders' jobs come first, then the long ones' (a kernel
    // draws a contiguous range); the ladders of up to 64 members first, then the deep ones (out_len is put back in call order).
    std::vector<DraftJob> jobs, jobs_long;
    std::vector<DraftLadder> lads, lads_deep;
    std::vector<char> lad_long, deep_long;
    std::vector<int64_t> src, src_deep;
    std::vector<int32_t> h_len;
    auto seq_of = [&](const hinge_draft_rung& r, DraftSeq* q) -> bool {
        if (r.read < 0 || r.read >= n_reads || (r.strand != 0 && r.strand != 1)) return false;
        const int rl = s->h_rlen[1][(size_t)r.read];
        if (r.start < 0 || r.end < r.start || r.end > rl) return false;
        q->boff = 0; q->rlen = rl; q->strand = r.strand; q->start = r.start; q->len = r.end - r.start;
        return true;
    };
    // the read's first byte lives in the device table; the jobs carry it so the kernels need one look-up less: fetch the host copy
    std::vector<long long> h_boff((size_t)std::max(n_reads, 1));
    CK(hipMemcpy(h_boff.data(), s->boff[1].p, sizeof(long long) * (size_t)n_reads, hipMemcpyDeviceToHost));
    for (int64_t l0 = 0; l0 < n_ladders;) {
        // ---- one batch: ladders l0 .. l1 whose scratch fits the budget ------------------------------------------------------------
        jobs.clear(); jobs_long.clear(); lads.clear(); lads_deep.clear(); lad_long.clear(); deep_long.clear(); src.clear(); src_deep.clear();
        long long ent_tot = 0, dtab_tot = 0, tag_tot = 0, col_tot = 0, tb_tot = 0, mem_tot = 0;
        int lds_max = 0, nc_max = 0;
        int64_t l1 = l0;
        for (; l1 < n_ladders; l1++) {
            const int64_t r0 = rung_off[l1], r1 = rung_off[l1 + 1];
            if (r1 - r0 < 1 || r1 - r0 > 65535)
                return fail(ctx, HINGE_E_CAPACITY, "hinge_draft_ladders: a ladder needs 1 .. 65535 members (the reference's vote counters are 16-bit, common.h)");
            const int n = (int)(r1 - r0);
            if (template_rung[l1] < 0 || template_rung[l1] >= n) return fail(ctx, HINGE_E_ARG, "hinge_draft_ladders: template member outside its ladder");
            DraftSeq T;
            if (!seq_of(rungs[r0 + template_rung[l1]], &T)) return fail(ctx, HINGE_E_RANGE, "hinge_draft_ladders: a member lies outside its read");
            if (T.len >= (1 << 21)) return fail(ctx, HINGE_E_CAPACITY, "hinge_draft_ladders: a template of 2^21 or more bases (a tag holds its position in 21 bits)");
            T.boff = h_boff[(size_t)rungs[r0 + template_rung[l1]].read];
            long long e_l = 0, dt_l = 0, tg_l = 0, sumq = 0;
            int lds_l = 0;
            bool is_long = false;
            std::vector<DraftJob> mine((size_t)n);
            for (int m = 0; m < n; m++) {
                DraftJob& J = mine[(size_t)m];
                if (!seq_of(rungs[r0 + m], &J.q)) return fail(ctx, HINGE_E_RANGE, "hinge_draft_ladders: a member lies outside its read");
                J.q.boff = h_boff[(size_t)rungs[r0 + m].read];
                J.t = T;
                J.max_d = (int)(0.3 * (J.q.len + J.t.len));                        // DW_banded.c:134
                // records of rounds 0 .. max_d - 1, min(d + 1, band + 1) each (closed form: the loop was 540 steps per job, 67 M per E. coli-sized call)
                const long long full = std::min<long long>(J.max_d, (long long)band_tolerance + 1);
                const long long cap = full * (full + 1) / 2 + (long long)(J.max_d - full) * ((long long)band_tolerance + 1);
                J.ent_cap = (int)std::min<long long>(cap, 0x7fffffffll);
                const int lds_j = (int)sizeof(int) * ((2 * J.max_d + 2) + draft_words(J.q.len) + draft_words(J.t.len));   // V, U (16-bit cells) + both sequences staged, 16 bases per word
                if (J.q.len >= 32768 || lds_j > 160 * 1024) is_long = true;
                lds_l = std::max(lds_l, lds_j);
                sumq += J.q.len;
            }
            for (auto& J : mine) {            // offsets into the batch's buffers; a long job: 2 words per record, V / U / sequences behind its d table
                J.ent_off = ent_tot + e_l; J.dtab_off = dtab_tot + dt_l; J.tag_off = tag_tot + tg_l;
                e_l += (is_long ? 2ll : 1ll) * J.ent_cap;
                dt_l += 2ll * (J.max_d + 1) + (is_long ? 2ll * (2 * J.max_d + 2) + draft_words(J.q.len) + draft_words(J.t.len) : 0ll);
                tg_l += (long long)J.q.len + J.t.len + 2;
            }
            const long long cols_l = 5ll * (T.len + 1 + sumq + 1);
            const long long mem_l = n > 64 ? (long long)(sizeof(DraftMember) + sizeof(unsigned)) / 4 * n : 0;   // k_draft_cns_deep's cursors
            const long long bytes = 4 * (ent_tot + e_l + dtab_tot + dt_l + tag_tot + tg_l + col_tot + cols_l + mem_tot + mem_l);
            if (l1 > l0 && bytes > budget) break;
            if (!is_long) lds_max = std::max(lds_max, lds_l);
            DraftLadder L;
            std::vector<DraftJob>& jv = is_long ? jobs_long : jobs;
            L.job0 = (int)jv.size(); L.n = n; L.t_len = T.len + 1;
            L.col_off = col_tot; L.col_cap = (int)std::min<long long>(cols_l, 0x7fffffffll);
            L.tb_off = tb_tot; L.out_off = out_off[l1] - out_off[l0];
            if (out_off[l1 + 1] - out_off[l1] < 2ll * L.t_len) return fail(ctx, HINGE_E_ARG, "hinge_draft_ladders: an output slot smaller than 2 * (template length + 1)");
            for (auto& J : mine) jv.push_back(J);
            if (n > 64) { lads_deep.push_back(L); deep_long.push_back(is_long); src_deep.push_back(l1 - l0); nc_max = std::max(nc_max, (n + 63) / 64); }
            else { lads.push_back(L); lad_long.push_back(is_long); src.push_back(l1 - l0); }
            ent_tot += e_l; dtab_tot += dt_l; tag_tot += tg_l; col_tot += cols_l; tb_tot += 2ll * L.t_len; mem_tot += mem_l;
        }
        // the long ladders' jobs behind the short ones'; the deep ladders behind the rest
        const size_t ns = jobs.size(), nl64 = lads.size();
        for (size_t i = 0; i < lads.size(); i++) if (lad_long[i]) lads[i].job0 += (int)ns;
        for (size_t i = 0; i < lads_deep.size(); i++) if (deep_long[i]) lads_deep[i].job0 += (int)ns;
        jobs.insert(jobs.end(), jobs_long.begin(), jobs_long.end());
        lads.insert(lads.end(), lads_deep.begin(), lads_deep.end());
        src.insert(src.end(), src_deep.begin(), src_deep.end());
        const size_t nj = jobs.size(), nl = lads.size(), n_long = nj - ns, n_deep = nl - nl64;
        const long long out_bytes = out_off[l1] - out_off[l0];
        if ((rc = ensure(ctx, d->jobs, sizeof(DraftJob) * nj))) return rc;
        if ((rc = ensure(ctx, d->ladders, sizeof(DraftLadder) * nl))) return rc;
        if ((rc = ensure(ctx, d->ents, sizeof(unsigned) * (size_t)std::max(ent_tot, 1ll)))) return rc;
        if ((rc = ensure(ctx, d->dtab, sizeof(int) * (size_t)std::max(dtab_tot, 1ll)))) return rc;
        if ((rc = ensure(ctx, d->tags, sizeof(unsigned) * (size_t)std::max(tag_tot, 1ll)))) return rc;
        if ((rc = ensure(ctx, d->n_tags, sizeof(int) * nj))) return rc;
        if ((rc = ensure(ctx, d->cols, sizeof(unsigned) * (size_t)std::max(col_tot, 1ll)))) return rc;
        if ((rc = ensure(ctx, d->tbase, sizeof(int) * (size_t)std::max(tb_tot, 1ll)))) return rc;
        if ((rc = ensure(ctx, d->out, (size_t)std::max(out_bytes, 1ll)))) return rc;
        if ((rc = ensure(ctx, d->out_len, sizeof(int) * nl))) return rc;
        if (n_deep) {
            if ((rc = ensure(ctx, d->mstate, sizeof(DraftMember) * nj))) return rc;
            if ((rc = ensure(ctx, d->mlink, sizeof(unsigned) * nj))) return rc;
        }
        CK(hipMemcpyAsync(d->jobs.p, jobs.data(), sizeof(DraftJob) * nj, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(d->ladders.p, lads.data(), sizeof(DraftLadder) * nl, hipMemcpyHostToDevice, ctx->stream));
        if ((size_t)lds_max > 48 * 1024 && (size_t)lds_max > d->align_lds_attr) {
            CK(hipFuncSetAttribute((const void*)k_draft_align, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
            d->align_lds_attr = (size_t)lds_max;
        }
        CK(hipMemsetAsync((int*)d->status.p + 1, 0, 16, ctx->stream));
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
            const size_t deep_lds = (size_t)5 * 8 * std::max(nc_max, 1);
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
        if (out_bytes) CK(hipMemcpyAsync(out + out_off[l0], d->out.p, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        h_len.resize(nl);
        CK(hipMemcpyAsync(h_len.data(), d->out_len.p, sizeof(int) * nl, hipMemcpyDeviceToHost, ctx->stream));
        int st = 0;
        CK(hipMemcpyAsync(&st, d->status.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < nl; i++) out_len[l0 + src[i]] = h_len[i];
        if (st & DRAFT_ST_CAP) return fail(ctx, HINGE_E_CAPACITY, "hinge draft: a ladder outgrew its buffers");
        if (st & DRAFT_ST_DELTA) return fail(ctx, HINGE_E_RANGE, "hinge draft: 255+ inserted bases in a row (the reference's alignment tags are undefined there, falcon.c:96)");
        if (st & DRAFT_ST_BASE) return fail(ctx, HINGE_E_UNDEFINED, "hinge draft: a ladder without a scoring column (the reference's assert, falcon.c:437)");
        l0 = l1;
    }
    return HINGE_OK;
}

}  // extern "C"
