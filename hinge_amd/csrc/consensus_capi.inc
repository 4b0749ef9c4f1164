// C ABI of `hinge consensus` (include/hinge_hip.h, "hinge consensus").  Included by hinge_capi.hip.
// Host work here: the segment table of the used alignments (computeTracePTS's loop bounds, LAInterface.cpp:3470-3500), buffer
// sizing, launches, getters.  Which alignments are used (the per-contig sort and remove_multialign's count, consensus.cpp:126-150)
// is the caller's: hinge_amd/host/consensus_main.cpp.
struct CnsState {
    DevBuf bps[2], boff[2], rlen[2];
    int n_seq[2] = {0, 0};
    std::vector<int32_t> h_rlen[2];
    std::vector<uint8_t> h_bps0;         // the draft's packed bases and offsets as given (hinge_seed_run builds its index from them)
    std::vector<int64_t> h_boff0;
    DevBuf alns, segs, trace, aln_slots, indels, n_indel, n_ins, col_base, cols, scratch, counts, cbase, packed, block_sum, contig_of_block, stats, out, scal;
    DevBuf tile_base, contig_of_tile, tile_ptr, tile_cursor, seg_order, halo;   // the LDS-tile vote
    size_t vote_lds_attr = 0;
    int64_t n_aln = 0, n_seg = 0, n_pos = 0;
    int n_blocks = 0;
    bool ran = false;
    std::vector<CnsAln> h_alns;
    std::vector<CnsSeg> h_segs;
    std::vector<long long> h_cbase;
    std::vector<int> h_first_block;
    std::vector<unsigned> h_block_off;
    std::vector<char> h_out;
    std::vector<CnsStats> h_stats;
    std::vector<CnsCols> h_cols;
    unsigned long long total = 0;
};

static void cns_release(hinge_ctx* ctx) {
    CnsState* s = ctx->cns;
    if (!s) return;
    DevBuf* all[] = {&s->bps[0], &s->bps[1], &s->boff[0], &s->boff[1], &s->rlen[0], &s->rlen[1], &s->alns, &s->segs, &s->trace, &s->aln_slots, &s->indels, &s->n_indel, &s->n_ins,
                     &s->col_base, &s->cols, &s->scratch, &s->counts, &s->cbase, &s->packed, &s->block_sum, &s->contig_of_block, &s->stats, &s->out, &s->scal,
                     &s->tile_base, &s->contig_of_tile, &s->tile_ptr, &s->tile_cursor, &s->seg_order, &s->halo};
    for (DevBuf* b : all) release(*b);
    delete s;
    ctx->cns = nullptr;
}

extern "C" {

int hinge_consensus_set_db(hinge_ctx* ctx, int32_t which, int32_t n, const int32_t* rlen, const int64_t* boff, const uint8_t* bps, int64_t bps_bytes) {
    if (!ctx || (which != 0 && which != 1) || n < 0 || (n > 0 && (!rlen || !boff)) || bps_bytes < 0 || (bps_bytes > 0 && !bps))
        return fail(ctx, HINGE_E_ARG, "hinge_consensus_set_db: bad arguments");
    for (int i = 0; i < n; i++)
        if (rlen[i] < 0 || boff[i] < 0 || boff[i] + ((int64_t)rlen[i] + 3) / 4 > bps_bytes) return fail(ctx, HINGE_E_RANGE, "hinge_consensus_set_db: a read's bases lie outside the .bps bytes");
    CK(hipSetDevice(ctx->device));
    if (!ctx->cns) ctx->cns = new CnsState();
    CnsState* s = ctx->cns;
    int rc;
    if ((rc = ensure(ctx, s->bps[which], (size_t)bps_bytes + CNS_BPS_SPARE))) return rc;     // (cns_window's loads end inside the spare bytes)
    if ((rc = ensure(ctx, s->boff[which], sizeof(long long) * (size_t)std::max(n, 1)))) return rc;
    if ((rc = ensure(ctx, s->rlen[which], sizeof(int) * (size_t)std::max(n, 1)))) return rc;
    if (bps_bytes) CK(hipMemcpyAsync(s->bps[which].p, bps, (size_t)bps_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (n) {
        static_assert(sizeof(long long) == sizeof(int64_t), "boff as long long");
        CK(hipMemcpyAsync(s->boff[which].p, boff, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(s->rlen[which].p, rlen, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    CK(hipStreamSynchronize(ctx->stream));
    s->n_seq[which] = n;
    s->h_rlen[which].assign(rlen, rlen + n);
    if (which == 0) {
        s->h_bps0.clear();
        s->h_boff0.clear();
        if (bps_bytes) s->h_bps0.assign(bps, bps + bps_bytes);
        if (n) s->h_boff0.assign(boff, boff + n);
    }
    s->ran = false;
    return HINGE_OK;
}

}  // extern "C"

// The realignment stage shared by `hinge consensus` and `hinge draft`: the segment table of the given alignments, its upload, and
// k_cns_realign - afterwards s->indels / n_indel / n_ins hold every segment's indel list (status word in s->scal, not yet read).
static int cns_realign_stage(hinge_ctx* ctx, int64_t n_aln, const hinge_cns_alignment* alns, const uint16_t* trace, int64_t n_trace, int32_t tspace) {
    CnsState* s = ctx->cns;
    const int n_contigs = s->n_seq[0];
    // ---- the alignments (host: range checks, where each one's segments start - a trace of tlen values has tlen / 2 segments);
    //      the segment table itself is made on the device from the uploaded trace (k_cns_segments) -----------------------------
    s->h_alns.resize((size_t)n_aln);
    s->h_segs.clear();
    long long n_seg = 0;
    for (int64_t x = 0; x < n_aln; x++) {
        const hinge_cns_alignment& r = alns[x];
        if (r.aread < 0 || r.aread >= n_contigs || r.bread < 0 || r.bread >= s->n_seq[1]) return fail(ctx, HINGE_E_RANGE, "hinge_consensus_run: read id outside its DB");
        const int alen = s->h_rlen[0][(size_t)r.aread], blen = s->h_rlen[1][(size_t)r.bread];
        if (r.tlen < 0 || r.trace_off < 0 || r.trace_off + r.tlen > n_trace) return fail(ctx, HINGE_E_RANGE, "hinge_consensus_run: trace outside the trace array");
        if (!(0 <= r.abpos && r.abpos <= r.aepos && r.aepos <= alen && 0 <= r.bbpos && r.bbpos <= r.bepos && r.bepos <= blen))
            return fail(ctx, HINGE_E_RANGE, "hinge_consensus_run: alignment coordinates outside their reads");
        CnsAln& a = s->h_alns[(size_t)x];
        a.a = r.aread; a.b = r.bread; a.comp = r.comp ? 1 : 0; a.ab = r.abpos; a.ae = r.aepos; a.bb = r.bbpos; a.be = r.bepos; a.blen = blen;
        a.seg0 = (int)n_seg;
        a.nseg = std::max(r.tlen / 2, 1);      // (computeTracePTS: one segment per (diffs, advance) pair; an alignment without pairs is one segment)
        a.dcap = 0; a.tlen = r.tlen; a.toff = r.trace_off;
        n_seg += a.nseg;
        if (n_seg >= 0x7fff0000ll) return fail(ctx, HINGE_E_CAPACITY, "hinge_consensus_run: more than 2^31 trace-point segments in one call: split the alignments");
    }
    s->n_aln = n_aln;
    s->n_seg = n_seg;
    int rc;
    if ((rc = ensure(ctx, s->alns, sizeof(CnsAln) * (size_t)std::max<int64_t>(n_aln, 1)))) return rc;
    if ((rc = ensure(ctx, s->segs, sizeof(CnsSeg) * (size_t)std::max<int64_t>(s->n_seg, 1)))) return rc;
    if ((rc = ensure(ctx, s->trace, sizeof(uint16_t) * (size_t)std::max<int64_t>(n_trace, 1)))) return rc;
    if ((rc = ensure(ctx, s->aln_slots, sizeof(unsigned) * (size_t)std::max<int64_t>(n_aln, 1)))) return rc;
    if ((rc = ensure(ctx, s->n_indel, sizeof(int) * (size_t)std::max<int64_t>(s->n_seg, 1)))) return rc;
    if ((rc = ensure(ctx, s->n_ins, sizeof(int) * (size_t)std::max<int64_t>(s->n_seg, 1)))) return rc;
    if ((rc = ensure(ctx, s->scal, 64))) return rc;
    CK(hipMemsetAsync(s->scal.p, 0, 64, ctx->stream));     // ints: [0] status, [2..3] total of the calls (64-bit), [4..5] the tile scan's total, [8] widest row, [9] largest dcap, [10..11] indel slots (64-bit)
    if (n_aln) CK(hipMemcpyAsync(s->alns.p, s->h_alns.data(), sizeof(CnsAln) * (size_t)n_aln, hipMemcpyHostToDevice, ctx->stream));
    if (n_trace) CK(hipMemcpyAsync(s->trace.p, trace, sizeof(uint16_t) * (size_t)n_trace, hipMemcpyHostToDevice, ctx->stream));
    int width_max = 4, dcap_max = 0;
    unsigned long long out_total = 0;
    if (n_aln) {
        int* scal = (int*)s->scal.p;
        const unsigned galn = (unsigned)((n_aln + CNS_BLOCK - 1) / CNS_BLOCK);
        hipLaunchKernelGGL(k_cns_segments, dim3(galn), dim3(CNS_BLOCK), 0, ctx->stream, (CnsAln*)s->alns.p, (int)n_aln, (const unsigned short*)s->trace.p, (int)tspace,
                           (const int*)s->rlen[0].p, (CnsSeg*)s->segs.p, (unsigned*)s->aln_slots.p, scal + 8, scal);
        hipLaunchKernelGGL(k_cns_scan, dim3(1), dim3(1024), 0, ctx->stream, (unsigned*)s->aln_slots.p, (int)n_aln, (unsigned long long*)(scal + 10));
        hipLaunchKernelGGL(k_cns_seg_offsets, dim3(galn), dim3(CNS_BLOCK), 0, ctx->stream, (const CnsAln*)s->alns.p, (int)n_aln, (const unsigned*)s->aln_slots.p, (CnsSeg*)s->segs.p);
        CK(hipGetLastError());
        int h[12];
        CK(hipMemcpyAsync(h, s->scal.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));     // (the one host round trip of the stage: the launch shape and the buffer sizes below depend on the trace)
        if (h[0] & CNS_ST_TRACE) return fail(ctx, HINGE_E_RANGE, "hinge_consensus_run: trace points inconsistent with the alignment's coordinates");
        width_max = std::max(h[8], 4); dcap_max = h[9];
        memcpy(&out_total, &h[10], sizeof(out_total));
        if (out_total >= 0xffff0000ull) return fail(ctx, HINGE_E_CAPACITY, "hinge_consensus_run: more than 2^32 indel slots in one call: split the alignments");
    }
    if ((rc = ensure(ctx, s->indels, sizeof(int) * (size_t)std::max<unsigned long long>(out_total, 1)))) return rc;
    // lanes of k_cns_realign and their private wave storage (cells_max ints each, capped at HINGE_CNS_SCRATCH_GB, default 8)
    long long scratch_cap = 8ll << 30;
    if (const char* g = getenv("HINGE_CNS_SCRATCH_GB")) scratch_cap = std::max(1ll, atoll(g)) << 30;
    const long long cells_max = cns_cells(dcap_max, width_max);      // per lane: rows -2 .. dcap_max of width_max cells (one shape for the launch)
    // as many workgroups as are RESIDENT at once (round 6: the kernel's 20 KiB of staged bases and its 70 VGPRs leave seven per CU; a
    // grid of eight per CU ran its last eighth as a second round behind the grid-stride loops of the first seven)
    static int per_cu = 0;
    if (per_cu == 0) {
        int nb = 0;
        per_cu = (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_cns_realign, CNS_BLOCK, 0) == hipSuccess && nb > 0) ? nb : 6;
        if (const char* g = getenv("HINGE_CNS_WGS_PER_CU")) per_cu = std::max(1, atoi(g));
    }
    long long want_blocks = std::max<long long>(1, std::min<long long>((s->n_seg + CNS_BLOCK - 1) / CNS_BLOCK, (long long)ctx->n_cu * per_cu));
    while (want_blocks > 1 && want_blocks * CNS_BLOCK * cells_max * (long long)sizeof(int) > scratch_cap) want_blocks /= 2;
    if (want_blocks * CNS_BLOCK * cells_max * (long long)sizeof(int) > scratch_cap) return fail(ctx, HINGE_E_CAPACITY, "hinge_consensus_run: one workgroup's wave storage exceeds the scratch budget (HINGE_CNS_SCRATCH_GB)");
    if ((rc = ensure(ctx, s->scratch, (size_t)(want_blocks * CNS_BLOCK * cells_max) * sizeof(int)))) return rc;
    if (s->n_seg) {
        CnsSeqs SA{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
        CnsSeqs SB{(const unsigned char*)s->bps[1].p, (const long long*)s->boff[1].p, (const int*)s->rlen[1].p};
        ProfScope _ps(ctx, KID_CNS_REALIGN);
        hipLaunchKernelGGL(k_cns_realign, dim3((unsigned)want_blocks), dim3(CNS_BLOCK), 0, ctx->stream, SA, SB, (const CnsAln*)s->alns.p, (const CnsSeg*)s->segs.p,
                           (int)s->n_seg, (int*)s->scratch.p, width_max, dcap_max + 3, (int*)s->indels.p, (int*)s->n_indel.p, (int*)s->n_ins.p, (int*)s->scal.p);
        CK(hipGetLastError());
    }
    return HINGE_OK;
}

extern "C" {

int hinge_consensus_run(hinge_ctx* ctx, int64_t n_aln, const hinge_cns_alignment* alns, const uint16_t* trace, int64_t n_trace, int32_t tspace) {
    if (!ctx || !ctx->cns || n_aln < 0 || (n_aln > 0 && !alns) || n_trace < 0 || (n_trace > 0 && !trace) || tspace <= 0)
        return fail(ctx, HINGE_E_ARG, "hinge_consensus_run: bad arguments (call hinge_consensus_set_db for both DBs first)");
    CnsState* s = ctx->cns;
    CK(hipSetDevice(ctx->device));
    s->ran = false;
    const int n_contigs = s->n_seq[0];
    int rc;
    if ((rc = cns_realign_stage(ctx, n_aln, alns, trace, n_trace, tspace))) return rc;
    // ---- contig position space, blocks of k_cns_call / k_cns_emit -------------------------------------------------------
    s->h_cbase.assign((size_t)n_contigs + 1, 0);
    for (int c = 0; c < n_contigs; c++) s->h_cbase[(size_t)c + 1] = s->h_cbase[(size_t)c] + s->h_rlen[0][(size_t)c];
    s->n_pos = s->h_cbase[(size_t)n_contigs];
    const long long per_block = (long long)CNS_BLOCK * CNS_CALL_ITEMS;
    std::vector<int2> cob;   // per block: (contig, the contig's first block)
    s->h_first_block.assign((size_t)n_contigs + 1, 0);
    for (int c = 0; c < n_contigs; c++) {
        const int fb = (int)cob.size();
        s->h_first_block[(size_t)c] = fb;
        const long long nb = (s->h_rlen[0][(size_t)c] + per_block - 1) / per_block;
        for (long long b = 0; b < nb; b++) cob.push_back(make_int2(c, fb));
    }
    s->n_blocks = (int)cob.size();
    s->h_first_block[(size_t)n_contigs] = s->n_blocks;
    // tiles of the LDS vote (k_cns_vote_tiles): a multiple of tspace positions each
    const int tile = cns_tile_len(tspace);
    std::vector<int> tile_base((size_t)n_contigs + 1, 0), cot;
    std::vector<int> votes_of_contig((size_t)std::max(n_contigs, 1), 0);
    for (int64_t x = 0; x < n_aln; x++) votes_of_contig[(size_t)alns[x].aread]++;
    bool tiled = tile <= CNS_TILE_MAX && !(getenv("HINGE_CNS_VOTE_GLOBAL") && atoi(getenv("HINGE_CNS_VOTE_GLOBAL")) != 0);
    for (int c = 0; c < n_contigs; c++) {
        tile_base[(size_t)c + 1] = tile_base[(size_t)c] + (s->h_rlen[0][(size_t)c] + tile - 1) / tile;
        for (int t = tile_base[(size_t)c]; t < tile_base[(size_t)c + 1]; t++) cot.push_back(c);
        if (votes_of_contig[(size_t)c] >= 65536) tiled = false;     // (16-bit counters)
    }
    const int n_tiles = tile_base[(size_t)n_contigs];
    const size_t plane = (size_t)std::max<int64_t>(s->n_pos, 1);
    if ((rc = ensure(ctx, s->col_base, sizeof(int) * (size_t)std::max<int64_t>(s->n_seg, 1)))) return rc;
    if ((rc = ensure(ctx, s->cols, sizeof(CnsCols) * (size_t)std::max<int64_t>(n_aln, 1)))) return rc;
    if ((rc = ensure(ctx, s->counts, sizeof(int) * 9 * plane))) return rc;
    if ((rc = ensure(ctx, s->cbase, sizeof(long long) * ((size_t)n_contigs + 1)))) return rc;
    if ((rc = ensure(ctx, s->packed, sizeof(unsigned) * plane))) return rc;
    if ((rc = ensure(ctx, s->block_sum, sizeof(unsigned) * (size_t)std::max(s->n_blocks, 1)))) return rc;
    if ((rc = ensure(ctx, s->contig_of_block, sizeof(int2) * (size_t)std::max(s->n_blocks, 1)))) return rc;
    if ((rc = ensure(ctx, s->stats, sizeof(CnsStats) * (size_t)std::max(n_contigs, 1)))) return rc;
    if ((rc = ensure(ctx, s->out, 2 * plane + 16))) return rc;
    if (tiled) {
        if ((rc = ensure(ctx, s->tile_base, sizeof(int) * ((size_t)n_contigs + 1)))) return rc;
        if ((rc = ensure(ctx, s->contig_of_tile, sizeof(int) * (size_t)std::max(n_tiles, 1)))) return rc;
        if ((rc = ensure(ctx, s->tile_ptr, sizeof(unsigned) * ((size_t)n_tiles + 1)))) return rc;
        if ((rc = ensure(ctx, s->tile_cursor, sizeof(unsigned) * ((size_t)n_tiles + 1)))) return rc;
        if ((rc = ensure(ctx, s->seg_order, sizeof(int) * (size_t)std::max<int64_t>(s->n_seg, 1)))) return rc;
        if ((rc = ensure(ctx, s->halo, sizeof(int) * 4 * (size_t)std::max(n_tiles, 1)))) return rc;
        CK(hipMemcpyAsync(s->tile_base.p, tile_base.data(), sizeof(int) * ((size_t)n_contigs + 1), hipMemcpyHostToDevice, ctx->stream));
        if (n_tiles) CK(hipMemcpyAsync(s->contig_of_tile.p, cot.data(), sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemsetAsync(s->tile_ptr.p, 0, sizeof(unsigned) * ((size_t)n_tiles + 1), ctx->stream));
        CK(hipMemsetAsync(s->halo.p, 0, sizeof(int) * 4 * (size_t)std::max(n_tiles, 1), ctx->stream));
    }
    CK(hipMemcpyAsync(s->cbase.p, s->h_cbase.data(), sizeof(long long) * ((size_t)n_contigs + 1), hipMemcpyHostToDevice, ctx->stream));
    if (s->n_blocks) CK(hipMemcpyAsync(s->contig_of_block.p, cob.data(), sizeof(int2) * (size_t)s->n_blocks, hipMemcpyHostToDevice, ctx->stream));
    unsigned long long scal_h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // The vote, the calls and the results.  A second pass only where the tile vote reports CNS_ST_VOTE16 (an inserted-base counter stood
    // at 0xffff: tens of thousands of inserted bases at one position): the planes are zeroed and k_cns_vote votes with its int32 counters.
    for (int pass = 0;; pass++) {
        if (!tiled || s->n_seg == 0) CK(hipMemsetAsync(s->counts.p, 0, sizeof(int) * 9 * plane, ctx->stream));   // (the tile vote stores every position itself)
        CK(hipMemsetAsync(s->stats.p, 0, sizeof(CnsStats) * (size_t)std::max(n_contigs, 1), ctx->stream));
        unsigned long long* total = (unsigned long long*)((char*)s->scal.p + 8);
        CnsSeqs SA{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
        CnsSeqs SB{(const unsigned char*)s->bps[1].p, (const long long*)s->boff[1].p, (const int*)s->rlen[1].p};
        if (s->n_seg) {
            if (pass == 0) {
                ProfScope _ps(ctx, KID_CNS_COLUMNS);
                hipLaunchKernelGGL(k_cns_columns, dim3((unsigned)((n_aln + CNS_BLOCK - 1) / CNS_BLOCK)), dim3(CNS_BLOCK), 0, ctx->stream, (const CnsAln*)s->alns.p, (int)n_aln,
                                   (const CnsSeg*)s->segs.p, (const int*)s->indels.p, (const int*)s->n_indel.p, (const int*)s->n_ins.p, (int*)s->col_base.p, (CnsCols*)s->cols.p, 100);
            }
            if (tiled) {
                const size_t lds = sizeof(unsigned) * 5 * ((size_t)tile + 1);
                if (lds > 48 * 1024 && lds > s->vote_lds_attr) {
                    CK(hipFuncSetAttribute((const void*)k_cns_vote_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                    s->vote_lds_attr = lds;
                }
                ProfScope _ps(ctx, KID_CNS_VOTE);
                const unsigned galn = (unsigned)((n_aln + CNS_BLOCK - 1) / CNS_BLOCK);
                hipLaunchKernelGGL(k_cns_tile_count, dim3(galn), dim3(CNS_BLOCK), 0, ctx->stream, (const CnsAln*)s->alns.p, (int)n_aln, (const CnsSeg*)s->segs.p,
                                   (const int*)s->tile_base.p, tile, (unsigned*)s->tile_ptr.p);
                hipLaunchKernelGGL(k_cns_scan, dim3(1), dim3(1024), 0, ctx->stream, (unsigned*)s->tile_ptr.p, n_tiles + 1, total + 1);
                CK(hipMemcpyAsync(s->tile_cursor.p, s->tile_ptr.p, sizeof(unsigned) * ((size_t)n_tiles + 1), hipMemcpyDeviceToDevice, ctx->stream));
                hipLaunchKernelGGL(k_cns_tile_fill, dim3(galn), dim3(CNS_BLOCK), 0, ctx->stream, (const CnsAln*)s->alns.p, (int)n_aln, (const CnsSeg*)s->segs.p,
                                   (const int*)s->tile_base.p, tile, (unsigned*)s->tile_cursor.p, (int*)s->seg_order.p);
                hipLaunchKernelGGL(k_cns_vote_tiles, dim3((unsigned)n_tiles), dim3(CNS_BLOCK), lds, ctx->stream, SB, (const CnsAln*)s->alns.p, (const CnsSeg*)s->segs.p,
                                   (const int*)s->indels.p, (const int*)s->n_indel.p, (const int*)s->col_base.p, (const CnsCols*)s->cols.p, (const long long*)s->cbase.p,
                                   (const int*)s->tile_base.p, (const int*)s->contig_of_tile.p, (const unsigned*)s->tile_ptr.p, (const int*)s->seg_order.p, tile,
                                   (int*)s->counts.p, (long long)plane, (int*)s->halo.p, (int*)s->scal.p);
            } else {
                ProfScope _ps(ctx, KID_CNS_VOTE);
                hipLaunchKernelGGL(k_cns_vote, dim3((unsigned)((s->n_seg + CNS_BLOCK - 1) / CNS_BLOCK)), dim3(CNS_BLOCK), 0, ctx->stream, SB, (const CnsAln*)s->alns.p,
                                   (const CnsSeg*)s->segs.p, (int)s->n_seg, (const int*)s->indels.p, (const int*)s->n_indel.p, (const int*)s->col_base.p, (const CnsCols*)s->cols.p,
                                   (const long long*)s->cbase.p, (int*)s->counts.p, (long long)plane);
            }
        }
        if (s->n_blocks) {
            ProfScope _ps(ctx, KID_CNS_CALL);
            hipLaunchKernelGGL(k_cns_call, dim3((unsigned)s->n_blocks), dim3(CNS_BLOCK), 0, ctx->stream, SA, (const int*)s->counts.p, (long long)plane, (long long)s->n_pos,
                               (const int2*)s->contig_of_block.p, (const long long*)s->cbase.p, (unsigned*)s->packed.p, (unsigned*)s->block_sum.p, (CnsStats*)s->stats.p,
                               (tiled && s->n_seg) ? (const int*)s->halo.p : (const int*)nullptr, (const int*)s->tile_base.p, tile);
            hipLaunchKernelGGL(k_cns_scan, dim3(1), dim3(1024), 0, ctx->stream, (unsigned*)s->block_sum.p, s->n_blocks, total);
            hipLaunchKernelGGL(k_cns_emit, dim3((unsigned)s->n_blocks), dim3(CNS_BLOCK), 0, ctx->stream, (const unsigned*)s->packed.p, (const int2*)s->contig_of_block.p,
                               (const long long*)s->cbase.p, (const unsigned*)s->block_sum.p, (char*)s->out.p);
        }
        CK(hipGetLastError());
        // results to the host: the strings, the block offsets (where a contig's string starts), statistics, chop offsets
        CK(hipMemcpyAsync(scal_h, s->scal.p, 64, hipMemcpyDeviceToHost, ctx->stream));
        s->h_block_off.assign((size_t)s->n_blocks + 1, 0);
        if (s->n_blocks) CK(hipMemcpyAsync(s->h_block_off.data(), s->block_sum.p, sizeof(unsigned) * (size_t)s->n_blocks, hipMemcpyDeviceToHost, ctx->stream));
        s->h_stats.assign((size_t)std::max(n_contigs, 1), CnsStats{});
        if (n_contigs) CK(hipMemcpyAsync(s->h_stats.data(), s->stats.p, sizeof(CnsStats) * (size_t)n_contigs, hipMemcpyDeviceToHost, ctx->stream));
        s->h_cols.assign((size_t)std::max<int64_t>(n_aln, 1), CnsCols{});
        if (n_aln) CK(hipMemcpyAsync(s->h_cols.data(), s->cols.p, sizeof(CnsCols) * (size_t)n_aln, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        if (!(tiled && ((int)(scal_h[0] & 0xffffffffu) & CNS_ST_VOTE16))) break;
        tiled = false;
    }
    const int st = (int)(scal_h[0] & 0xffffffffu);
    if (st & CNS_ST_WAVES) return fail(ctx, HINGE_E_RANGE, "hinge consensus: a trace-point segment needs more edit operations than its alignment's recorded diffs (the reference overruns its wave arrays here, LAInterface.cpp:3444-3466)");
    if (st & CNS_ST_INDELS) return fail(ctx, HINGE_E_RANGE, "hinge consensus: a segment's indel list outgrew its slots");
    s->total = scal_h[1];
    s->h_block_off[(size_t)s->n_blocks] = (unsigned)s->total;
    s->h_out.resize((size_t)s->total);
    if (s->total) CK(hipMemcpy(s->h_out.data(), s->out.p, (size_t)s->total, hipMemcpyDeviceToHost));
    s->ran = true;
    return HINGE_OK;
}

int hinge_consensus_get_contig(hinge_ctx* ctx, int32_t contig, char* out, int64_t cap, int64_t* len, hinge_cns_stats* stats) {
    if (!ctx || !ctx->cns || !ctx->cns->ran || contig < 0 || contig >= ctx->cns->n_seq[0] || !len) return fail(ctx, HINGE_E_ARG, "hinge_consensus_get_contig: no results / bad contig");
    CnsState* s = ctx->cns;
    const unsigned lo = s->h_block_off[(size_t)s->h_first_block[(size_t)contig]], hi = s->h_block_off[(size_t)s->h_first_block[(size_t)contig + 1]];
    *len = (int64_t)(hi - lo);
    if (out) {
        if (cap < *len) return fail(ctx, HINGE_E_CAPACITY, "hinge_consensus_get_contig: buffer too small");
        memcpy(out, s->h_out.data() + lo, (size_t)(hi - lo));
    }
    if (stats) {
        const CnsStats& t = s->h_stats[(size_t)contig];
        stats->sum_coverage = t.sum_cov; stats->good_bases = t.good; stats->insertions = t.insertions; stats->deletions = t.deletions;
        stats->low_coverage_bases = t.low_cov; stats->consensus_length = t.clen; stats->contig_length = s->h_rlen[0][(size_t)contig];
    }
    return HINGE_OK;
}

int hinge_consensus_get_offsets(hinge_ctx* ctx, int32_t* offsets) {
    if (!ctx || !ctx->cns || !ctx->cns->ran || !offsets) return fail(ctx, HINGE_E_ARG, "hinge_consensus_get_offsets: no results");
    for (int64_t x = 0; x < ctx->cns->n_aln; x++) offsets[x] = ctx->cns->h_cols[(size_t)x].offset;
    return HINGE_OK;
}

int hinge_consensus_get_indels(hinge_ctx* ctx, int64_t aln, int32_t* out, int64_t cap, int64_t* n) {
    if (!ctx || !ctx->cns || !ctx->cns->ran || aln < 0 || aln >= ctx->cns->n_aln || !n) return fail(ctx, HINGE_E_ARG, "hinge_consensus_get_indels: no results / bad alignment");
    CnsState* s = ctx->cns;
    CK(hipSetDevice(ctx->device));
    const CnsAln& a = s->h_alns[(size_t)aln];
    if (s->h_segs.size() != (size_t)s->n_seg) {   // (the table lives on the device: fetched for this accessor only)
        s->h_segs.resize((size_t)s->n_seg);
        if (s->n_seg) CK(hipMemcpy(s->h_segs.data(), s->segs.p, sizeof(CnsSeg) * (size_t)s->n_seg, hipMemcpyDeviceToHost));
    }
    std::vector<int> cnt((size_t)a.nseg);
    CK(hipMemcpy(cnt.data(), (const int*)s->n_indel.p + a.seg0, sizeof(int) * (size_t)a.nseg, hipMemcpyDeviceToHost));
    int64_t tot = 0;
    for (int c : cnt) tot += c;
    *n = tot;
    if (!out) return HINGE_OK;
    if (cap < tot) return fail(ctx, HINGE_E_CAPACITY, "hinge_consensus_get_indels: buffer too small");
    int64_t at = 0;
    for (int k = 0; k < a.nseg; k++) {
        const CnsSeg& g = s->h_segs[(size_t)(a.seg0 + k)];
        if (cnt[(size_t)k]) CK(hipMemcpy(out + at, (const int*)s->indels.p + g.out_off, sizeof(int) * (size_t)cnt[(size_t)k], hipMemcpyDeviceToHost));
        at += cnt[(size_t)k];
    }
    return HINGE_OK;
}

}  // extern "C"
